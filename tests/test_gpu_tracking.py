"""Photon tracking on the HIP path against the CPU oracle's tracked mode.

GPUPhotons.propagate(track=True) drives the C-ABI chunk entry
(chr_propagate_chunk) from Python with caller-allocated queues and scratch,
one step per host step; Simulation(photon_tracking=True) turns its step
snapshots into per-photon tracks.  The expected output is
oracle.propagate_tracked (pinned on the CPU by tests/test_oracle_tracked.py):
ids bit-equal, photon snapshots under the parity contract of
tests/test_gpu_parity.py, final photons and RNG slot states equal.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
import scenes
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

DEAD = 0x800F      # NO_HIT | BULK_ABSORB | SURFACE_DETECT | SURFACE_ABSORB | NAN_ABORT (device bit 15)


@pytest.fixture(scope='module')
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from chroma.gpu import create_cuda_context
    return create_cuda_context()


_cache = {}


def _geometry(name, small_detector=None, small_packed=None):
    """(geometry, packed, GPUGeometry) of 'small' (the 2-PMT detector) or
    'scene' (scenes.physics_scene()), built once per module."""
    if name not in _cache:
        from chroma import gpu, loader
        from chroma.gpu.packing import PackedGeometry
        if name == 'small':
            geo, packed = small_detector, small_packed
        else:
            geo = loader.create_geometry_from_obj(scenes.physics_scene())
            packed = PackedGeometry(geo)
        _cache[name] = (geo, packed, gpu.GPUGeometry(geo))
    return _cache[name]


def _photons(name, n, seed):
    from chroma.photon_source import isotropic
    return isotropic(n, seed=seed) if name == 'small' else scenes.photon_sources(n, seed=seed)


def _outside_photons(n):
    """Born outside the world looking away: every one ends NO_HIT at step 1."""
    from chroma.event import Photons
    pos = np.tile(np.array([0.0, 0.0, 5000.0], np.float32), (n, 1))
    pos[:, 0] = np.arange(n)
    dir = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (n, 1))
    pol = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (n, 1))
    return Photons(pos, dir, pol, np.full(n, 400.0, np.float32))


def _as_gpu(photons):
    return SimpleNamespace(get=lambda: photons)


def _check_tracked(got, want, label):
    ids, steps = got
    o_ids, o_steps = want
    assert len(ids) == len(steps) == len(o_ids), '%s: %d entries, oracle %d' % (label, len(ids), len(o_ids))
    for k in range(len(o_ids)):
        assert ids[k].dtype == np.uint32
        assert np.array_equal(ids[k], o_ids[k]), '%s: step %d ids differ' % (label, k)
        _compare(o_steps[k], _as_gpu(steps[k]), '%s step %d' % (label, k))


# (geometry, photons, seed, ntpb, max_blocks, max_steps, scatter_first, ncopies, entries the oracle must give)
CASES = {
    # cap 2048: step 1 is three chunks, later steps fewer
    'chunks': ('small', 5000, 41, 64, 32, 12, 0, 1, None),
    # a chunk size that is no multiple of 64
    'ragged': ('small', 5000, 42, 100, 41, 12, 0, 1, None),
    # scatter_first on the first pass only
    'scatter_first': ('scene', 6000, 43, 64, 64, 12, 1, 1, 13),
    # clones interleaved in the first queue, ids beyond true_nphotons
    'ncopies': ('scene', 3000, 44, 64, 64, 12, 0, 2, 13),
    'one_step': ('scene', 3000, 45, 64, 64, 1, 0, 1, 2),
    'zero_steps': ('scene', 3000, 45, 64, 64, 0, 0, 1, 1),
}


def _oracle_case(case, packed):
    name, n, seed, ntpb, max_blocks, max_steps, scatter_first, ncopies, entries = CASES[case]
    photons = _photons(name, n, seed)
    want = oracle.propagate_tracked(packed, photons, seed, ntpb * max_blocks, ntpb, max_blocks, max_steps,
                                    scatter_first=scatter_first, ncopies=ncopies)
    ids = want[0]
    if entries is not None:
        assert len(ids) == entries, (case, len(ids))
    if max_steps >= 1:
        cap = ntpb * max_blocks
        assert len(ids[1]) == n * ncopies
        if case in ('chunks', 'ragged'):
            assert len(ids[1]) > cap and len(ids) > 3, 'step 1 must take several chunks'
        if ncopies > 1:
            assert (ids[1] >= n).sum() == n * (ncopies - 1) and ids[1][1] == n
    return photons, want


@pytest.mark.parametrize('case', sorted(CASES))
def test_tracked_propagate_parity(cuda, small_detector, small_packed, case):
    from chroma import gpu
    name, n, seed, ntpb, max_blocks, max_steps, scatter_first, ncopies, _ = CASES[case]
    geo, packed, gg = _geometry(name, small_detector, small_packed)
    photons, (o_ids, o_steps, final, st) = _oracle_case(case, packed)
    rng = gpu.get_rng_states(ntpb * max_blocks, seed=seed)
    gp = gpu.GPUPhotons(photons, ncopies=ncopies)
    got = gp.propagate(gg, rng, nthreads_per_block=ntpb, max_blocks=max_blocks, max_steps=max_steps,
                       scatter_first=scatter_first, track=True)
    _check_tracked(got, (o_ids, o_steps), case)
    _compare(final, gp, case + ' final')
    assert np.array_equal(rng.get().reshape(-1), st), 'RNG slot states differ'
    if max_steps == 0:
        assert np.array_equal(st, oracle.rng_init(ntpb * max_blocks, seed=seed))
        assert (final.flags == 0).all()


def _break_case(packed):
    """Nobody is left alive before max_steps: photons that all miss (step 1)
    mixed into the 2-PMT detector's isotropic ones, which are all absorbed or
    lost within a few steps.  Chosen with the oracle: the list must be shorter
    than max_steps + 1 and at least 3 long."""
    from chroma.event import Photons
    from chroma.photon_source import isotropic
    photons = Photons.join([isotropic(1500, seed=46), _outside_photons(500)])
    want = oracle.propagate_tracked(packed, photons, 46, 64 * 32, 64, 32, 12)
    ids = want[0]
    assert 3 <= len(ids) < 13, len(ids)
    assert ((want[2].flags & DEAD) != 0).all(), 'the run must end with nobody alive'
    return photons, want


def test_tracked_propagate_ends_early(cuda, small_detector, small_packed):
    """The reference's `break` (photon.py:285-286)."""
    from chroma import gpu
    geo, packed, gg = _geometry('small', small_detector, small_packed)
    photons, (o_ids, o_steps, final, st) = _break_case(packed)
    rng = gpu.get_rng_states(64 * 32, seed=46)
    gp = gpu.GPUPhotons(photons)
    got = gp.propagate(gg, rng, nthreads_per_block=64, max_blocks=32, max_steps=12, track=True)
    _check_tracked(got, (o_ids, o_steps), 'break')
    _compare(final, gp, 'break final')
    assert np.array_equal(rng.get().reshape(-1), st)


def test_tracked_equals_untracked_single_step(cuda):
    """max_steps = 1 with N >= nthreads_per_block*128 queued: the untracked
    path takes one single step too, so both paths (chr_propagate_chunk driven
    from Python, chr_propagate's own loop) must leave identical photons and RNG
    slot states, word for word."""
    from chroma import gpu
    geo, packed, gg = _geometry('scene')
    photons = scenes.photon_sources(9000, seed=47)
    assert len(photons) >= 64 * 128
    out = []
    for track in (True, False):
        rng = gpu.get_rng_states(64 * 64, seed=47)
        gp = gpu.GPUPhotons(photons)
        gp.propagate(gg, rng, nthreads_per_block=64, max_blocks=64, max_steps=1, track=track)
        out.append((gp.get(), rng.get().reshape(-1)))
    (a, ra), (b, rb) = out
    for f in oracle.HostPhotons.FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), f
    assert np.array_equal(ra, rb)
    assert (a.flags != 0).any()


def test_propagate_chunk_argument_checks(cuda, small_detector, small_packed):
    from chroma import gpu
    from chroma.gpu import _native, gpuarray as ga
    from chroma.gpu.tools import current_stream
    from chroma.photon_source import isotropic
    geo, packed, gg = _geometry('small', small_detector, small_packed)
    n = 256
    photons = isotropic(n, seed=48)
    gp = gpu.GPUPhotons(photons)
    rng = gpu.get_rng_states(n, seed=48)
    rng0 = rng.get().copy()
    qin = ga.to_gpu(np.arange(n, dtype=np.uint32))
    header = np.zeros(n + 1, np.uint32)
    header[0] = 1
    qout = ga.to_gpu(header)
    scratch = ga.zeros(int(_native.lib().chr_propagate_scratch_words(n)), np.uint32)
    desc = gp._desc()

    def chunk(queue_in, queue_out, scr, nslots, nthreads):
        _native.call('chr_propagate_chunk', ctypes.c_void_p(gg.gpudata), ctypes.byref(desc), rng.gpudata, nslots, 0,
                     nthreads, queue_in, queue_out, 1, 0, 0, scr, current_stream())

    with pytest.raises(_native.NativeError):
        chunk(None, qout.gpudata, scratch.gpudata, n, n)
    with pytest.raises(_native.NativeError):
        chunk(qin.gpudata, None, scratch.gpudata, n, n)
    with pytest.raises(_native.NativeError):
        chunk(qin.gpudata, qout.gpudata, None, n, n)
    with pytest.raises(_native.NativeError):
        chunk(qin.gpudata, qout.gpudata, scratch.gpudata, n - 1, n)      # nthreads > rng_nslots
    chunk(qin.gpudata, qout.gpudata, scratch.gpudata, n, 0)              # no-op
    got = gp.get()
    assert (got.flags == 0).all() and np.array_equal(got.pos, photons.pos)
    assert np.array_equal(qout.get(), header)
    assert np.array_equal(rng.get(), rng0)


SIM_EVENTS = (1500, 400, 700)      # the second event: photons that all die at step 1


def _sim_case(packed, seed, ntpb, max_blocks, max_steps):
    from chroma.event import Photons
    from chroma.photon_source import isotropic
    events = [isotropic(SIM_EVENTS[0], seed=50), _outside_photons(SIM_EVENTS[1]), isotropic(SIM_EVENTS[2], seed=51)]
    joined = Photons.join(events)
    joined.evidx[:] = np.repeat(np.arange(3), SIM_EVENTS)
    joined.last_hit_triangles[:] = -1      # Simulation uploads flags only
    joined.weights[:] = 1.0
    want = oracle.propagate_tracked(packed, joined, seed, ntpb * max_blocks, ntpb, max_blocks, max_steps)
    ids, steps = want[0], want[1]
    bounds = np.cumsum((0,) + SIM_EVENTS)
    lo, hi = bounds[1], bounds[2]
    assert ((steps[1].flags[(ids[1] >= lo) & (ids[1] < hi)] & DEAD) != 0).all()
    assert len(ids) > 3
    assert not ((ids[2] >= lo) & (ids[2] < hi)).any() and ((ids[2] >= hi).any() and (ids[2] < lo).any())
    return events, joined, want, bounds


def test_simulation_photon_tracks(cuda, small_detector, small_packed):
    """Simulation(photon_tracking=True): per photon, the input, then one entry
    per step it entered (the tracked oracle run of the joined batch split at
    the event bounds), ending at its photons_end state.  Every photon is in the
    first queue, so no track is empty: that branch of Simulation._emit is
    unreachable for an event that has photons."""
    from chroma.sim import Simulation
    seed, ntpb, max_blocks, max_steps = 7, 64, 32, 10
    events, joined, (o_ids, o_steps, final, st), bounds = _sim_case(small_packed, seed, ntpb, max_blocks, max_steps)
    sim = Simulation(small_detector, seed=seed, photon_tracking=True, nthreads_per_block=ntpb, max_blocks=max_blocks)
    out = list(sim.simulate(events, keep_photons_end=True, max_steps=max_steps))
    assert len(out) == 3
    assert np.array_equal(sim.rng_states.get().reshape(-1), st)
    fields = ('pos', 'dir', 'pol', 'wavelengths', 't', 'last_hit_triangles', 'flags', 'weights')
    for e, ev in enumerate(out):
        lo, hi = int(bounds[e]), int(bounds[e + 1])
        assert len(ev.photon_tracks) == hi - lo
        # the oracle's track of every photon of the event: (entry, position in entry)
        where = [[] for _ in range(hi - lo)]
        for k, q in enumerate(o_ids):
            for j in np.flatnonzero((q >= lo) & (q < hi)):
                where[int(q[j]) - lo].append((k, int(j)))
        want = oracle.HostPhotons(joined)
        for f in want.FIELDS:      # per event: all track entries of all its photons, back to back
            setattr(want, f, np.concatenate([np.stack([getattr(o_steps[k], f)[j] for k, j in w]) for w in where]))
        lengths = [len(w) for w in where]
        assert [len(np.atleast_1d(tr.t)) for tr in ev.photon_tracks] == lengths
        assert min(lengths) >= 2 and (e == 1) == (max(lengths) == 2)
        got = SimpleNamespace(**{f: np.concatenate([np.atleast_1d(getattr(tr, f)).reshape(
            (-1, 3) if f in ('pos', 'dir', 'pol') else (-1,)) for tr in ev.photon_tracks]) for f in fields})
        got.evidx = np.concatenate([np.atleast_1d(tr.evidx) for tr in ev.photon_tracks])
        _compare(want, _as_gpu(got), 'event %d tracks' % e)
        first = np.cumsum([0] + lengths[:-1])
        last = np.cumsum(lengths) - 1
        # starts at the input photon, ends at photons_end
        assert np.array_equal(got.pos[first], events[e].pos) and (got.flags[first] == 0).all()
        assert np.array_equal(got.t[first], events[e].t)
        for f in fields:
            a, b = getattr(got, f)[last], getattr(ev.photons_end, f)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f
        end = oracle.HostPhotons(joined)
        for f in end.FIELDS:
            setattr(end, f, getattr(final, f)[lo:hi])
        _compare(end, _as_gpu(ev.photons_end), 'event %d photons_end' % e)
