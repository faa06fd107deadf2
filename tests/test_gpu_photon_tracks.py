"""Photon tracks recorded on the device (GPUPhotons.propagate_tracks,
chr_propagate_tracked) against the CPU oracle's tracked mode and, word for
word, against the host-driven chunk loop (GPUPhotons.device_tracking cleared:
GPUPhotons._propagate_tracked, the path tests/test_gpu_tracking.py pinned to
the oracle before the tracks moved to the device).

The oracle's result of a case is computed once per module and shared; so is
each path's GPU run of a case.
"""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
import scenes
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEAD = 0x800F      # NO_HIT | BULK_ABSORB | SURFACE_DETECT | SURFACE_ABSORB | NAN_ABORT (device bit 15)
FIELDS = ('pos', 'dir', 'pol', 'wavelengths', 't', 'flags', 'last_hit_triangles', 'weights', 'evidx')


@pytest.fixture(scope='module')
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from chroma.gpu import create_cuda_context
    return create_cuda_context()


_geo, _want, _runs = {}, {}, {}


def _geometry(name, small_detector=None, small_packed=None):
    if name not in _geo:
        from chroma import gpu, loader
        from chroma.gpu.packing import PackedGeometry
        if name == 'small':
            geo, packed = small_detector, small_packed
        else:
            geo = loader.create_geometry_from_obj(scenes.physics_scene())
            packed = PackedGeometry(geo)
        _geo[name] = (geo, packed, gpu.GPUGeometry(geo))
    return _geo[name]


def _outside_photons(n):
    """Born outside the world looking away: every one ends NO_HIT at step 1."""
    from chroma.event import Photons
    pos = np.tile(np.array([0.0, 0.0, 5000.0], np.float32), (n, 1))
    pos[:, 0] = np.arange(n)
    dir = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (n, 1))
    pol = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (n, 1))
    return Photons(pos, dir, pol, np.full(n, 400.0, np.float32))


# geometry, photons, seed, ntpb, max_blocks, max_steps, scatter_first, ncopies, use_weights
# (the six parameter sets of tests/test_gpu_tracking.py's CASES, its early-break case, use_weights on the scene)
CASES = {
    'chunks': ('small', 5000, 41, 64, 32, 12, 0, 1, False),          # cap 2048, a multiple of 64: the split step
    'ragged': ('small', 5000, 42, 100, 41, 12, 0, 1, False),         # cap 4100: the chunk launches
    'scatter_first': ('scene', 6000, 43, 64, 64, 12, 1, 1, False),
    'ncopies': ('scene', 3000, 44, 64, 64, 12, 0, 2, False),
    'one_step': ('scene', 3000, 45, 64, 64, 1, 0, 1, False),
    'zero_steps': ('scene', 3000, 45, 64, 64, 0, 0, 1, False),
    'break': ('small', 2000, 46, 64, 32, 12, 0, 1, False),           # 1500 isotropic + 500 that miss
    'weights': ('scene', 3000, 48, 64, 64, 12, 0, 1, True),
}


def _case_photons(case):
    from chroma.event import Photons
    from chroma.photon_source import isotropic
    name, n, seed = CASES[case][:3]
    if case == 'break':
        return Photons.join([isotropic(1500, seed=46), _outside_photons(500)])
    return isotropic(n, seed=seed) if name == 'small' else scenes.photon_sources(n, seed=seed)


def _oracle_case(case, packed):
    """(photons, (ids, steps, final, rng states)) of the oracle's tracked run, once."""
    if case not in _want:
        name, n, seed, ntpb, max_blocks, max_steps, scatter_first, ncopies, use_weights = CASES[case]
        photons = _case_photons(case)
        want = oracle.propagate_tracked(packed, photons, seed, ntpb * max_blocks, ntpb, max_blocks, max_steps,
                                        use_weights=use_weights, scatter_first=scatter_first, ncopies=ncopies)
        ids = want[0]
        assert len(ids[0]) == n * ncopies
        if case in ('chunks', 'ragged'):
            assert len(ids[1]) > ntpb * max_blocks and len(ids) > 3, 'step 1 must take several chunks'
        if case == 'break':
            assert 3 <= len(ids) < 13 and ((want[2].flags & DEAD) != 0).all()
        if ncopies > 1:
            assert (ids[1] >= n).sum() == n * (ncopies - 1) and ids[1][1] == n
        _want[case] = (photons, want)
    return _want[case]


def _words(photons):
    return {f: np.ascontiguousarray(getattr(photons, f)).view(np.uint32) for f in FIELDS}


def _gpu_case(case, path, small_detector, small_packed, capacity_hint=0):
    """One GPU run of a case, once per (case, path): 'host' = device_tracking
    cleared through propagate(track=True), 'device' = the same call with it
    set, 'tracks' = propagate_tracks (the PhotonTracks is kept)."""
    key = (case, path, capacity_hint)
    if key not in _runs:
        from chroma import gpu
        name, n, seed, ntpb, max_blocks, max_steps, scatter_first, ncopies, use_weights = CASES[case]
        geo, packed, gg = _geometry(name, small_detector, small_packed)
        rng = gpu.get_rng_states(ntpb * max_blocks, seed=seed)
        gp = gpu.GPUPhotons(_case_photons(case), ncopies=ncopies)
        kw = dict(nthreads_per_block=ntpb, max_blocks=max_blocks, max_steps=max_steps, use_weights=use_weights,
                  scatter_first=scatter_first)
        tracks = None
        if path == 'tracks':
            tracks = gp.propagate_tracks(gg, rng, capacity_hint=capacity_hint, **kw)
            ids, steps = tracks.steps()
        else:
            saved = gpu.GPUPhotons.device_tracking
            gpu.GPUPhotons.device_tracking = path == 'device'
            try:
                ids, steps = gp.propagate(gg, rng, track=True, **kw)
            finally:
                gpu.GPUPhotons.device_tracking = saved
        _runs[key] = SimpleNamespace(ids=ids, steps=steps, final=gp.get(), rng=rng.get().reshape(-1), tracks=tracks,
                                     gp=gp, stats=getattr(gp, 'last_stats', None))
    return _runs[key]


def _as_gpu(photons):
    return SimpleNamespace(get=lambda: photons)


def _assert_same_words(a, b, label):
    assert len(a.ids) == len(b.ids) == len(a.steps) == len(b.steps), label
    for k in range(len(a.ids)):
        assert a.ids[k].dtype == b.ids[k].dtype == np.uint32
        assert np.array_equal(a.ids[k], b.ids[k]), '%s: entry %d ids' % (label, k)
        wa, wb = _words(a.steps[k]), _words(b.steps[k])
        for f in FIELDS:
            assert wa[f].shape == wb[f].shape and np.array_equal(wa[f], wb[f]), '%s: entry %d %s' % (label, k, f)
    wa, wb = _words(a.final), _words(b.final)
    for f in FIELDS:
        assert np.array_equal(wa[f], wb[f]), '%s: final %s' % (label, f)
    assert np.array_equal(a.rng, b.rng), label + ': RNG slot states'


# ------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize('case', sorted(CASES))
def test_tracks_against_oracle(cuda, small_detector, small_packed, case):
    name, n, seed, ntpb, max_blocks, max_steps = CASES[case][:6]
    packed = _geometry(name, small_detector, small_packed)[1]
    photons, (o_ids, o_steps, final, st) = _oracle_case(case, packed)
    run = _gpu_case(case, 'tracks', small_detector, small_packed)
    assert len(run.ids) == len(run.steps) == len(o_ids), '%s: %d entries, oracle %d' % (case, len(run.ids), len(o_ids))
    for k in range(len(o_ids)):
        assert run.ids[k].dtype == np.uint32
        assert np.array_equal(run.ids[k], o_ids[k]), '%s: entry %d ids differ' % (case, k)
        _compare(o_steps[k], _as_gpu(run.steps[k]), '%s entry %d' % (case, k))
    _compare(final, run.gp, case + ' final')
    assert np.array_equal(run.rng, st), 'RNG slot states differ'
    # the handle and the stats
    tr, stats = run.tracks, run.stats
    assert tr.nentries == len(o_ids) and tr.nphotons == len(final)
    assert tr.step_counts.tolist() == [len(q) for q in o_ids]
    assert tr.nrecords == int(tr.step_counts.sum())
    assert stats.steps_run + 1 == tr.nentries
    assert stats.host_syncs <= stats.steps_run + 2
    if max_steps == 0:
        assert tr.nentries == 1 and np.array_equal(st, oracle.rng_init(ntpb * max_blocks, seed=seed))
    if case == 'chunks':
        assert stats.trace_launches == stats.steps_run          # every step the split trace + shade launch
        assert stats.launches == stats.steps_run
    if case == 'ragged':
        assert stats.trace_launches == 0 and stats.launches > stats.steps_run       # chunk launches


# ------------------------------------------------------------------ against the host-driven loop, word for word
@pytest.mark.parametrize('case', ['chunks', 'ragged', 'ncopies', 'weights'])
def test_tracks_equal_host_loop(cuda, small_detector, small_packed, case):
    host = _gpu_case(case, 'host', small_detector, small_packed)
    device = _gpu_case(case, 'device', small_detector, small_packed)
    assert len(host.ids) > 2 and len(host.ids[1]) == len(host.ids[0])
    _assert_same_words(host, device, case)
    if case == 'weights':
        assert (host.final.weights != 1.0).any()


# ------------------------------------------------------------------ photon-major order
@pytest.mark.parametrize('case', ['chunks', 'ncopies'])
def test_photon_major_order(cuda, small_detector, small_packed, case):
    name, n, seed, ntpb, max_blocks, max_steps = CASES[case][:6]
    packed = _geometry(name, small_detector, small_packed)[1]
    photons, (o_ids, o_steps, final, st) = _oracle_case(case, packed)
    run = _gpu_case(case, 'tracks', small_detector, small_packed)
    tr = run.tracks
    offsets, flat = tr.flat()
    nph = tr.nphotons
    counts = np.zeros(nph, np.int64)
    for q in o_ids:
        counts += np.bincount(q, minlength=nph)
    assert offsets.dtype == np.int64 and len(offsets) == nph + 1
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(counts)]))
    assert counts.min() >= 1                                      # every photon of the first queue
    # a photon alive at max_steps was queued into every step: max_steps + 1 records, as has every photon of
    # the last step's queue (the scene's run reaches max_steps: 13 entries, as tests/test_gpu_tracking.py demands)
    alive = (final.flags & DEAD) == 0
    assert (counts[alive] == max_steps + 1).all() and counts.max() <= max_steps + 1
    if case == 'ncopies':
        assert len(o_ids) == max_steps + 1 and len(o_ids[-1]) > 0
    if len(o_ids) == max_steps + 1:
        assert (counts[o_ids[-1]] == max_steps + 1).all()
    # record j of photon i is that photon's state in entry j (the step-major entries, checked against the oracle above)
    wf = _words(flat)
    for k in range(len(run.ids)):
        ws = _words(run.steps[k])
        at = offsets[run.ids[k].astype(np.int64)] + k
        for f in FIELDS:
            assert np.array_equal(wf[f][at], ws[f]), '%s: entry %d %s' % (case, k, f)
    rec, off = tr.records(1)
    assert np.array_equal(rec[:, 0], np.repeat(np.arange(nph, dtype=np.uint32), counts))
    assert np.array_equal(rec[:, 15], np.concatenate([np.arange(c, dtype=np.uint32) for c in counts]))
    one = tr.track(int(np.argmax(counts)))
    assert len(one) == counts.max() and one.flags[0] == 0
    # the device views are the buffers chr_tracks_copy downloads
    for order in (0, 1):
        d_rec, d_off = tr.device(order)
        h_rec, h_off = tr.records(order)
        assert np.array_equal(d_rec.get().reshape(-1, 16), h_rec) and np.array_equal(d_off.get(), h_off)


def test_simulation_flat_tracks(cuda, small_detector, small_packed):
    """Each event's photon_tracks_flat is its photon_tracks back to back, and the
    events are what the host-driven loop gives (device_tracking cleared)."""
    from chroma import gpu
    from chroma.photon_source import isotropic
    from chroma.sim import Simulation
    sizes = (700, 200, 300)

    def events():
        return [isotropic(sizes[0], seed=50), _outside_photons(sizes[1]), isotropic(sizes[2], seed=51)]

    out = {}
    saved = gpu.GPUPhotons.device_tracking
    try:
        for flag in (False, True):
            gpu.GPUPhotons.device_tracking = flag
            sim = Simulation(small_detector, seed=7, photon_tracking=True, nthreads_per_block=64, max_blocks=32)
            out[flag] = list(sim.simulate(events(), keep_photons_end=True, max_steps=10)), sim.rng_states.get()
    finally:
        gpu.GPUPhotons.device_tracking = saved
    (old, rng_old), (new, rng_new) = out[False], out[True]
    assert np.array_equal(rng_old, rng_new)
    for e, (a, b) in enumerate(zip(old, new)):
        assert a.photon_tracks_flat is None
        offsets, flat = b.photon_tracks_flat
        assert len(b.photon_tracks) == len(a.photon_tracks) == sizes[e] and len(offsets) == sizes[e] + 1
        lengths = [len(t) for t in b.photon_tracks]
        assert min(lengths) >= 2 and (e == 1) == (max(lengths) == 2)
        assert np.array_equal(np.diff(offsets), lengths) and offsets[0] == 0 and offsets[-1] == len(flat)
        wf = _words(flat)
        for f in FIELDS:
            joined = np.concatenate([np.ascontiguousarray(getattr(t, f)).view(np.uint32) for t in b.photon_tracks])
            assert np.array_equal(joined, wf[f]), f
            parent = np.concatenate([np.atleast_1d(getattr(t, f)).reshape((-1, 3) if f in ('pos', 'dir', 'pol') else (-1,))
                                     for t in a.photon_tracks])
            assert np.array_equal(np.ascontiguousarray(parent).view(np.uint32), wf[f]), f
        for f in FIELDS:
            assert np.array_equal(_words(a.photons_end)[f], _words(b.photons_end)[f]), f


# ------------------------------------------------------------------ growth
def test_capacity_growth(cuda, small_detector, small_packed):
    """capacity_hint = 1: the first allocation is raised to entry 0 and the
    buffer then grows at every step; the records are those of the default hint."""
    default = _gpu_case('chunks', 'tracks', small_detector, small_packed)
    grown = _gpu_case('chunks', 'tracks', small_detector, small_packed, capacity_hint=1)
    assert grown.tracks.nentries == default.tracks.nentries > 3
    assert grown.tracks.nrecords == default.tracks.nrecords == int(grown.tracks.step_counts.sum())
    for order in (0, 1):
        (ra, oa), (rb, ob) = default.tracks.records(order), grown.tracks.records(order)
        assert np.array_equal(ra, rb) and np.array_equal(oa, ob)
    _assert_same_words(default, grown, 'capacity_hint=1')


# ------------------------------------------------------------------ edges
@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_few_photons(cuda, small_detector, small_packed, n):
    from chroma import gpu
    from chroma.photon_source import isotropic
    geo, packed, gg = _geometry('small', small_detector, small_packed)
    photons = isotropic(n, seed=52)
    o_ids, o_steps, final, st = oracle.propagate_tracked(packed, photons, 52, 64 * 4, 64, 4, 6)
    runs = []
    saved = gpu.GPUPhotons.device_tracking
    try:
        for flag in (False, True):
            gpu.GPUPhotons.device_tracking = flag
            rng = gpu.get_rng_states(64 * 4, seed=52)
            gp = gpu.GPUPhotons(photons)
            ids, steps = gp.propagate(gg, rng, nthreads_per_block=64, max_blocks=4, max_steps=6, track=True)
            runs.append(SimpleNamespace(ids=ids, steps=steps, final=gp.get(), rng=rng.get().reshape(-1)))
    finally:
        gpu.GPUPhotons.device_tracking = saved
    _assert_same_words(runs[0], runs[1], '%d photons' % n)
    assert len(runs[1].ids) == len(o_ids)
    for k in range(len(o_ids)):
        assert np.array_equal(runs[1].ids[k], o_ids[k])
        _compare(o_steps[k], _as_gpu(runs[1].steps[k]), '%d photons entry %d' % (n, k))
    assert np.array_equal(runs[1].rng, st)


def test_no_photons(cuda, small_detector, small_packed):
    from chroma import gpu
    from chroma.event import Photons
    geo, packed, gg = _geometry('small', small_detector, small_packed)
    rng = gpu.get_rng_states(64 * 4, seed=53)
    before = rng.get().copy()
    gp = gpu.GPUPhotons(Photons())
    tracks = gp.propagate_tracks(gg, rng, nthreads_per_block=64, max_blocks=4, max_steps=6)
    assert (tracks.nentries, tracks.nrecords, tracks.nphotons) == (1, 0, 0)
    assert tracks.last_stats.launches == 0 and tracks.last_stats.steps_run == 0 and tracks.last_stats.host_syncs == 0
    ids, steps = tracks.steps()
    assert len(ids) == 1 and len(ids[0]) == 0 and len(steps[0]) == 0
    assert tracks.flat()[0].tolist() == [0]
    assert np.array_equal(rng.get(), before)


def test_second_tracked_propagate(cuda, small_detector, small_packed):
    """Non-fresh flags: a second tracked propagate of the same GPUPhotons.  Entry
    0 carries the flags the photons had, the dead ones are in the first queue
    (entries 0 and 1) and in no later entry; both paths give the same words."""
    from chroma import gpu
    from chroma.photon_source import isotropic
    geo, packed, gg = _geometry('small', small_detector, small_packed)
    photons = isotropic(3000, seed=54)
    runs = []
    saved = gpu.GPUPhotons.device_tracking
    try:
        for flag in (False, True):
            gpu.GPUPhotons.device_tracking = flag
            rng = gpu.get_rng_states(64 * 32, seed=54)
            gp = gpu.GPUPhotons(photons)
            kw = dict(nthreads_per_block=64, max_blocks=32, max_steps=2, track=True)
            gp.propagate(gg, rng, **kw)
            between = gp.get()
            ids, steps = gp.propagate(gg, rng, **kw)
            runs.append(SimpleNamespace(ids=ids, steps=steps, final=gp.get(), rng=rng.get().reshape(-1),
                                        between=between))
    finally:
        gpu.GPUPhotons.device_tracking = saved
    _assert_same_words(runs[0], runs[1], 'second propagate')
    new = runs[1]
    dead = (new.between.flags & DEAD) != 0
    assert dead.any() and (~dead).any() and len(new.ids) == 3
    assert np.array_equal(new.ids[0], np.arange(3000, dtype=np.uint32)) and np.array_equal(new.ids[1], new.ids[0])
    assert np.array_equal(new.steps[0].flags, new.between.flags) and (new.steps[0].flags != 0).any()
    for f in FIELDS:      # the dead ones are not stepped: entry 1 shows them as they were
        assert np.array_equal(_words(new.steps[1])[f][dead], _words(new.between)[f][dead]), f
    assert not dead[new.ids[2]].any() and len(new.ids[2]) > 0


# ------------------------------------------------------------------ untracked runs are left alone
def test_untracked_runs_unchanged(cuda, small_detector, small_packed, tmp_path):
    """propagate(track=False) before and after a tracked call in this process,
    and in a process that never made one: the same words.  The tracked driver
    shares chr_propagate's buffer context and must leave nothing behind in it."""
    from photon_tracks_child import FIELDS as CHILD_FIELDS, untracked_run
    geo, packed, gg = _geometry('small', small_detector, small_packed)
    before = untracked_run(gg)
    _runs.pop(('chunks', 'tracks', 7), None)
    run = _gpu_case('chunks', 'tracks', small_detector, small_packed, capacity_hint=7)     # a tracked call, now
    assert run.tracks.nentries > 3
    after = untracked_run(gg)
    out = str(tmp_path / 'fresh.npz')
    env = dict(os.environ)
    env.pop('CHROMA_AMD_LIB', None)
    r = subprocess.run([sys.executable, os.path.join(HERE, 'photon_tracks_child.py'), out], env=env, timeout=300,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    fresh = np.load(out)
    assert (before['flags'] != 0).any()
    for f in CHILD_FIELDS + ('rng',):
        assert np.array_equal(before[f], fresh[f]), 'before a tracked call: ' + f
        assert np.array_equal(after[f], fresh[f]), 'after a tracked call: ' + f
