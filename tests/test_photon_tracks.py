"""Photon tracks recorded on the device (chr_propagate_tracked, chr_tracks_*,
chroma.gpu.tracks.PhotonTracks), as far as they can be checked without a GPU:
the entry points' refusals (all made before a device is touched), the calls on
a NULL handle and on the empty handle of a 0-photon call, and the host
reshaping of PhotonTracks on a hand-made record buffer."""
import ctypes

import numpy as np
import pytest

CHR_OK, CHR_ERR_INVALID = 0, 1
NAMES = ('chr_propagate_tracked', 'chr_tracks_info', 'chr_tracks_entry_counts', 'chr_tracks_device',
         'chr_tracks_copy', 'chr_tracks_free', 'chr_tracks_unpack')


# ------------------------------------------------------------------ entry points
def _call(nphotons=10, true_nphotons=None, ncopies=1, rng_nslots=64 * 64, ntpb=64, max_blocks=64, max_steps=10,
          null=(), out=None):
    """chr_propagate_tracked with made-up device addresses: every refusal comes
    before the first dereference or launch, so none of them is ever used."""
    from chroma.gpu import _native
    fake = 0x1000
    ph = _native.PhotonsDesc(*[fake] * 9)
    if 'photon_t' in null:
        ph.d_t = None
    out = ctypes.c_void_p(0xdead) if out is None else out
    true_nphotons = nphotons // ncopies if true_nphotons is None else true_nphotons
    rc = _native.lib().chr_propagate_tracked(
        None if 'g' in null else fake, None if 'ph' in null else ctypes.byref(ph), nphotons, true_nphotons, ncopies,
        None if 'rng' in null else fake, rng_nslots, ntpb, max_blocks, max_steps, 0, 0, 0,
        None if 'out' in null else ctypes.byref(out), None, None)
    return rc, out


def test_entry_points_are_exported():
    from chroma.gpu import _native
    lib = ctypes.CDLL(_native.library_path())
    for name in NAMES:
        assert name in _native.EXPORTED, name
        assert hasattr(lib, name), name
    res, args = _native._SIGNATURES['chr_propagate_tracked']
    assert len(args) == 16 and args[12] is ctypes.c_uint64          # capacity_hint is 64-bit
    assert _native._SIGNATURES['chr_tracks_copy'][1] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                         ctypes.c_void_p]


def test_python_surface():
    from chroma import gpu
    from chroma.gpu import tracks
    assert gpu.PhotonTracks is tracks.PhotonTracks
    assert gpu.GPUPhotons.device_tracking is True
    assert callable(gpu.GPUPhotons.propagate_tracks)
    for name in ('steps', 'flat', 'track', 'device', 'close'):
        assert callable(getattr(gpu.PhotonTracks, name))


def test_refuses_null_out():
    from chroma.gpu import _native
    rc, _ = _call(null=('out',))
    assert rc == CHR_ERR_INVALID
    assert b'out' in _native.lib().chr_last_error()


@pytest.mark.parametrize('null', ['g', 'ph', 'photon_t', 'rng'])
def test_refuses_null_arguments(null):
    from chroma.gpu import _native
    rc, out = _call(null=(null,))
    assert rc == CHR_ERR_INVALID and not out.value          # no handle is left
    assert b'null' in _native.lib().chr_last_error()


def test_refuses_bad_shapes():
    from chroma.gpu import _native
    rc, out = _call(rng_nslots=64 * 64 - 1)                  # ntpb * max_blocks > rng_nslots
    assert rc == CHR_ERR_INVALID and not out.value
    assert b'rng_states' in _native.lib().chr_last_error()
    rc, out = _call(nphotons=10, true_nphotons=4, ncopies=2)
    assert rc == CHR_ERR_INVALID and not out.value
    assert b'true_nphotons' in _native.lib().chr_last_error()
    assert _call(nphotons=10, true_nphotons=10, ncopies=0)[0] == CHR_ERR_INVALID
    rc, out = _call(max_steps=-1)
    assert rc == CHR_ERR_INVALID and not out.value
    assert b'max_steps' in _native.lib().chr_last_error()
    assert _call(ntpb=0)[0] == CHR_ERR_INVALID
    assert _call(max_blocks=0)[0] == CHR_ERR_INVALID


def test_null_handle():
    from chroma.gpu import _native
    lib = _native.lib()
    n32, n64 = ctypes.c_uint32(), ctypes.c_uint64()
    counts = np.zeros(4, np.uint64)
    assert lib.chr_tracks_info(None, ctypes.byref(n32), ctypes.byref(n64), ctypes.byref(n32)) == CHR_ERR_INVALID
    assert b'null handle' in lib.chr_last_error()
    assert lib.chr_tracks_entry_counts(None, counts.ctypes.data) == CHR_ERR_INVALID
    assert lib.chr_tracks_device(None, 0, None, None) == CHR_ERR_INVALID
    assert lib.chr_tracks_copy(None, 0, None, None) == CHR_ERR_INVALID
    assert lib.chr_tracks_free(None) == CHR_OK               # as chr_bvh_result_free


def test_no_photons_gives_an_empty_handle():
    """nphotons == 0: a handle with entry 0 alone, no records, nothing launched
    (the addresses are made up); the order argument is checked on it."""
    from chroma.gpu import _native
    from chroma.gpu.tracks import PhotonTracks
    lib = _native.lib()
    rc, out = _call(nphotons=0)
    assert rc == CHR_OK and out.value not in (None, 0, 0xdead)
    tracks = PhotonTracks(out, np.zeros(0, np.uint32))
    assert (tracks.nentries, tracks.nrecords, tracks.nphotons) == (1, 0, 0)
    assert tracks.step_counts.tolist() == [0]
    ids, photons = tracks.steps()
    assert len(ids) == len(photons) == 1 and ids[0].dtype == np.uint32 and len(ids[0]) == len(photons[0]) == 0
    offsets, flat = tracks.flat()
    assert offsets.tolist() == [0] and len(flat) == 0
    for order in (-1, 2, 7):
        assert lib.chr_tracks_copy(out, order, None, None) == CHR_ERR_INVALID
        assert b'order' in lib.chr_last_error()
        assert lib.chr_tracks_device(out, order, None, None) == CHR_ERR_INVALID
    rec, off = ctypes.c_void_p(1), ctypes.c_void_p(1)
    assert lib.chr_tracks_device(out, 1, ctypes.byref(rec), ctypes.byref(off)) == CHR_OK
    assert not rec.value and not off.value
    soff = np.full(2, 9, np.uint64)
    assert lib.chr_tracks_copy(out, 0, None, soff.ctypes.data) == CHR_OK and soff.tolist() == [0, 0]
    tracks.close()
    tracks.close()                                            # idempotent
    # arrays of no photons have no address: not a refusal (the other arguments still are)
    rc, empty = _call(nphotons=0, null=('photon_t',))
    assert rc == CHR_OK and empty.value and lib.chr_tracks_free(empty) == CHR_OK
    assert _call(nphotons=0, null=('rng',))[0] == CHR_ERR_INVALID
    assert _call(nphotons=0, null=('ph',))[0] == CHR_ERR_INVALID
    with pytest.raises(ValueError):
        tracks.device(0)


# ------------------------------------------------------------------ host reshaping
def _made_tracks():
    """true_nphotons = 3, ncopies = 2 (ids 0..5, clones interleaved in the first
    queue); entry 1 = the first queue again, then 4, 2, 1 survivors."""
    queues = [[0, 3, 1, 4, 2, 5], [0, 3, 1, 4, 2, 5], [3, 1, 2, 5], [1, 5], [5]]
    rows = []
    for k, q in enumerate(queues):
        for pid in q:
            f = (np.arange(2, 14) + 100.0 * pid + 0.25 * k).astype(np.float32)
            row = np.zeros(16, np.uint32)
            row[0], row[1], row[14], row[15] = pid, 0x10 * k + pid, np.int32(-1 if k == 0 else 7 * pid + k).view(np.uint32), k
            row[2:14] = f.view(np.uint32)
            rows.append(row)
    evidx = np.array([7, 8, 9, 17, 18, 19], np.uint32)      # distinct for the copies: gathered by id
    return np.array(rows), [len(q) for q in queues], queues, evidx


def _expect(pid, k):
    f = (np.arange(2, 14) + 100.0 * pid + 0.25 * k).astype(np.float32)
    return dict(pos=f[0:3], dir=f[3:6], pol=f[6:9], wavelengths=f[9], t=f[10], weights=f[11], flags=0x10 * k + pid,
                last_hit_triangles=-1 if k == 0 else 7 * pid + k)


def _check_row(photons, j, pid, k, evidx):
    for name, want in _expect(pid, k).items():
        assert np.array_equal(getattr(photons, name)[j], want), (name, pid, k)
    assert photons.evidx[j] == evidx[pid]


def test_host_reshaping_steps():
    from chroma.gpu.tracks import PhotonTracks
    rec, counts, queues, evidx = _made_tracks()
    tracks = PhotonTracks.from_host(rec, counts, evidx, nphotons=6)
    assert (tracks.nentries, tracks.nrecords, tracks.nphotons) == (5, 19, 6)
    assert tracks.step_counts.tolist() == counts
    ids, photons = tracks.steps()
    assert len(ids) == len(photons) == 5
    for k, q in enumerate(queues):
        assert ids[k].dtype == np.uint32 and ids[k].tolist() == q
        p = photons[k]
        assert p.pos.shape == (len(q), 3) and p.pos.dtype == np.float32 and p.pos.flags['C_CONTIGUOUS']
        assert p.flags.dtype == np.uint32 and p.last_hit_triangles.dtype == np.int32 and p.evidx.dtype == np.uint32
        for j, pid in enumerate(q):
            _check_row(p, j, pid, k, evidx)
    assert (photons[0].evidx[1], photons[0].evidx[0]) == (17, 7)      # id 3 is a copy: evidx[3], not evidx[0]


def test_host_reshaping_flat_and_track():
    from chroma.gpu.tracks import PhotonTracks
    rec, counts, queues, evidx = _made_tracks()
    lengths = [2, 4, 3, 3, 2, 5]                    # entries each id is queued in
    for given in (False, True):
        kw = {}
        if given:       # the photon-major buffer as the device writes it: record (id, k) at offsets[id] + k
            off = np.concatenate([[0], np.cumsum(lengths)])
            flat_rec = np.zeros_like(rec)
            for row in rec:
                flat_rec[off[row[0]] + row[15]] = row
            kw = dict(flat_records=flat_rec, flat_offsets=off)
        tracks = PhotonTracks.from_host(rec, counts, evidx, nphotons=6, **kw)
        offsets, photons = tracks.flat()
        assert offsets.dtype == np.int64 and np.diff(offsets).tolist() == lengths and len(photons) == 19
        for pid in range(6):
            tr = tracks.track(pid)
            assert len(tr) == lengths[pid]
            for k in range(lengths[pid]):
                _check_row(tr, k, pid, k, evidx)
                _check_row(photons, offsets[pid] + k, pid, k, evidx)
        with pytest.raises(IndexError):
            tracks.track(6)


def test_simulation_splits_flat_tracks_by_event():
    """Simulation._emit's slicing: an event's (offsets, Photons) from the batch's
    photon-major tracks, and one Photons per photon between consecutive offsets."""
    from chroma.gpu.tracks import PhotonTracks
    from chroma.sim import _event_tracks_flat, _track_list
    rec, counts, queues, evidx = _made_tracks()
    flat = PhotonTracks.from_host(rec, counts, evidx, nphotons=6).flat()
    lengths = [2, 4, 3, 3, 2, 5]
    for start, end in ((0, 2), (2, 5), (5, 6), (3, 3)):
        offsets, photons = _event_tracks_flat(flat, start, end)
        assert offsets.tolist() == np.concatenate([[0], np.cumsum(lengths[start:end])]).tolist()
        assert len(photons) == sum(lengths[start:end])
        tracks = _track_list(offsets, photons)
        assert [len(t) for t in tracks] == lengths[start:end]
        for i, t in enumerate(tracks):
            for k in range(len(t)):
                _check_row(t, k, start + i, k, evidx)
        if tracks:
            assert np.array_equal(np.concatenate([t.t for t in tracks]), photons.t)
