"""The DAQ of all events of a batch in one call (chr_daq_acquire_events through
GPUDaq.acquire_events and Simulation.daq_events) against the CPU oracle run
event by event, and against the GPU's own per-event loop: every channel word
and every RNG slot state, bit for bit."""
import numpy as np
import pytest

import oracle
from test_daq_events import BOUNDS, SIZES, oracle_events

pytestmark = pytest.mark.gpu

MAXBITS = np.float32(1e9).view(np.uint32)


@pytest.fixture(scope='module')
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from chroma.gpu import create_cuda_context
    return create_cuda_context()


@pytest.fixture
def daq_detector(small_detector):
    saved = small_detector.time_cdf, small_detector.charge_cdf
    small_detector.set_time_dist_gaussian(1.2, -6.0, 6.0)
    small_detector.set_charge_dist_gaussian(1.0, 0.1, 0.5, 1.5)
    yield small_detector
    small_detector.time_cdf, small_detector.charge_cdf = saved


def _rows(chans):
    """(time words, charge words, histories, f32 charges as words) of a GPUEventChannels, (nevents, nchannels) each"""
    shape = (chans.nevents, chans.nchannels)
    return (chans.time_int.get().reshape(shape), chans.q_int.get().reshape(shape), chans.flags.get().reshape(shape),
            chans.q.get().view(np.uint32).reshape(shape))


def _check_rows(got, want, unit, label):
    t, q, fl = want
    assert np.array_equal(got[0], t), label + ': earliest time words differ'
    assert np.array_equal(got[1], q), label + ': charge words differ'
    assert np.array_equal(got[2], fl), label + ': channel histories differ'
    # every row is converted (each is its own ndaq = 1 acquisition)
    assert np.array_equal(got[3], (q.astype(np.float32) * np.float32(unit)).view(np.uint32)), \
        label + ': converted charges differ'


def _check_channels(channels, want, unit):
    t, q, fl = want
    assert len(channels) == len(t)
    for e, ch in enumerate(channels):
        assert np.array_equal(ch.t.view(np.uint32), t[e]) and np.array_equal(ch.flags, fl[e])
        assert np.array_equal(ch.q.view(np.uint32), (q[e].astype(np.float32) * np.float32(unit)).view(np.uint32))
        assert np.array_equal(ch.hit, t[e].view(np.float32) < 1e8)
        assert ch.t.base is None and ch.q.base is None and ch.flags.base is None     # the event owns its rows


def _photon_words(gp):
    got = gp.get()
    return [np.asarray(getattr(got, f)).copy() for f in ('t', 'flags', 'last_hit_triangles', 'weights', 'pos')]


@pytest.mark.parametrize('ntpb,max_blocks,weight', [
    (64, 8, 1.0),          # cap = 512: a slot takes up to four photons of the 2000-photon event
    (64, 1024, 0.5)])      # cap above every event, global weight 0.5
def test_made_records(cuda, daq_detector, ntpb, max_blocks, weight):
    from chroma import gpu
    from test_gpu_daq import _made_records
    photons, kind = _made_records(daq_detector)
    host = oracle.HostPhotons(photons)
    nslots = 64 * 1024
    gdet = gpu.GPUDetector(daq_detector)
    gp = gpu.GPUPhotons(photons, copy_flags=True, copy_triangles=True, copy_weights=True)
    before = _photon_words(gp)
    st = oracle.rng_init(nslots, seed=5)
    t, q, fl, _ = oracle_events(daq_detector, host, st, nslots, BOUNDS, ntpb, max_blocks, weight)
    assert all((q[e] > 0).any() for e in np.flatnonzero(SIZES >= 63))
    assert (t[SIZES == 0] == MAXBITS).all()

    rng = gpu.get_rng_states(nslots, seed=5)
    daq = gpu.GPUDaq(gdet)
    chans = daq.acquire_events(gp, rng, BOUNDS, nthreads_per_block=ntpb, max_blocks=max_blocks, weight=weight)
    assert len(chans) == len(SIZES)
    _check_rows(_rows(chans), (t, q, fl), gdet.charge_unit, 'against the oracle')
    assert np.array_equal(rng.get().reshape(-1), st), 'RNG slot states differ from the oracle'
    _check_channels(chans.get(), (t, q, fl), gdet.charge_unit)
    for a, b in zip(before, _photon_words(gp)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), 'the DAQ changed the photons'

    # the GPU's own per-event loop, from fresh states of the same seed
    rng2 = gpu.get_rng_states(nslots, seed=5)
    daq2 = gpu.GPUDaq(gdet)
    loop = []
    for start, n in zip(BOUNDS[:-1], SIZES):
        daq2.begin_acquire()
        daq2.acquire(gp, rng2, nthreads_per_block=ntpb, max_blocks=max_blocks, start_photon=int(start),
                     nphotons=int(n), weight=weight)
        words = (daq2.earliest_time_int_gpu.get(), daq2.channel_q_int_gpu.get(), daq2.channel_history_gpu.get())
        ch = daq2.end_acquire().get()
        loop.append(words + (ch.q.view(np.uint32),))
    want = tuple(np.array([r[k] for r in loop]) for k in range(4))
    for got, w, name in zip(_rows(chans), want, ('time words', 'charge words', 'histories', 'charges')):
        assert np.array_equal(got, w), name + ' differ from the per-event loop'
    assert np.array_equal(rng.get(), rng2.get()), 'RNG slot states differ from the per-event loop'


def test_groups_of_three(cuda, daq_detector):
    """The events in the groups Simulation would make under a budget of three
    events' rows: the same rows and RNG states as in one call."""
    from chroma import gpu
    from chroma.sim import daq_event_groups
    from test_gpu_daq import _made_records
    photons, kind = _made_records(daq_detector)
    host = oracle.HostPhotons(photons)
    nslots = 64 * 1024
    gdet = gpu.GPUDetector(daq_detector)
    gp = gpu.GPUPhotons(photons, copy_flags=True, copy_triangles=True, copy_weights=True)
    st = oracle.rng_init(nslots, seed=5)
    t, q, fl, _ = oracle_events(daq_detector, host, st, nslots, BOUNDS, 64, 8)
    groups = daq_event_groups(BOUNDS, gdet.nchannels, 16 * gdet.nchannels * 3 + 5)
    assert [b - a for a, b in groups] == [3, 3, 2]
    rng = gpu.get_rng_states(nslots, seed=5)
    daq = gpu.GPUDaq(gdet)
    parts, channels = [], []
    for a, b in groups:
        chans = daq.acquire_events(gp, rng, BOUNDS[a:b + 1], nthreads_per_block=64, max_blocks=8)
        parts.append(_rows(chans))
        channels += chans.get()
    got = tuple(np.concatenate([p[k] for p in parts]) for k in range(4))
    _check_rows(got, (t, q, fl), gdet.charge_unit, 'groups of three')
    _check_channels(channels, (t, q, fl), gdet.charge_unit)
    assert np.array_equal(rng.get().reshape(-1), st)


def test_after_propagate(cuda, daq_detector, small_packed):
    """What a real propagate leaves, as test_daq_parity, in nine uneven events."""
    from chroma import gpu
    from chroma.photon_source import isotropic
    from test_gpu_parity import _run_both, _compare
    photons = isotropic(20000, seed=31)
    nslots = 64 * 1024
    gp, host, rng, st, _ = _run_both(daq_detector, small_packed, photons, nslots, 64, 1024, 100, seed=5)
    _compare(host, gp, 'propagate before DAQ')
    bounds = np.array([0, 1, 700, 700, 5000, 5063, 9000, 9001, 15000, 20000], np.int64)
    gdet = gpu.GPUDetector(daq_detector)
    for ntpb, max_blocks in ((64, 1024), (64, 16)):      # cap above every event; cap 1024 below four of them
        t, q, fl, _ = oracle_events(daq_detector, host, st, nslots, bounds, ntpb, max_blocks)
        assert (q.sum(axis=1) > 0).sum() >= 2 and (t[2] == MAXBITS).all()
        chans = gpu.GPUDaq(gdet).acquire_events(gp, rng, bounds, nthreads_per_block=ntpb, max_blocks=max_blocks)
        _check_rows(_rows(chans), (t, q, fl), gdet.charge_unit, 'after a propagate, cap %d' % (ntpb * max_blocks))
        assert np.array_equal(rng.get().reshape(-1), st)


def _same_photons(a, b):
    if a is None or b is None:
        return a is None and b is None
    return len(a) == len(b) and all(
        np.array_equal(np.asarray(getattr(a, f)).view(np.uint32), np.asarray(getattr(b, f)).view(np.uint32))
        for f in ('pos', 'dir', 'pol', 'wavelengths', 't', 'flags', 'last_hit_triangles', 'weights', 'evidx',
                  'channel') if hasattr(a, f) or hasattr(b, f))


def test_simulation_end_to_end(cuda, daq_detector):
    """Simulation(run_daq=True) over several batches, batched against per-event DAQ."""
    from chroma.photon_source import isotropic
    from chroma.sim import Simulation
    r = np.random.RandomState(3)
    sizes = r.randint(0, 3001, 40)
    sizes[[3, 17, 18]] = 0
    sizes[-1] = 1500
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    source = isotropic(int(cuts[-1]), seed=77)
    runs = []
    for batched in (True, False):
        sim = Simulation(daq_detector, seed=23, nthreads_per_block=64, max_blocks=256)
        sim.daq_events = batched
        sim.daq_group_bytes = 16 * 2 * 4            # groups of four events on the 2-PMT detector
        evs = list(sim.simulate((source[a:b] for a, b in zip(cuts[:-1], cuts[1:])), run_daq=True,
                                photons_per_batch=20000, max_steps=100))
        assert sim.last_pipeline[0] >= 3, 'several batches'
        runs.append((evs, sim.rng_states.get()))
    (evs_a, rng_a), (evs_b, rng_b) = runs
    assert len(evs_a) == len(evs_b) == 40
    nhit = 0
    for e, (a, b) in enumerate(zip(evs_a, evs_b)):
        assert np.array_equal(a.channels.hit, b.channels.hit), e
        assert np.array_equal(a.channels.t.view(np.uint32), b.channels.t.view(np.uint32)), e
        assert np.array_equal(a.channels.q.view(np.uint32), b.channels.q.view(np.uint32)), e
        assert np.array_equal(a.channels.flags, b.channels.flags), e
        assert _same_photons(a.flat_hits, b.flat_hits), e
        assert sorted(a.hits) == sorted(b.hits) and all(_same_photons(a.hits[c], b.hits[c]) for c in a.hits), e
        nhit += int(a.channels.hit.sum())
        if sizes[e] == 0:
            assert not a.channels.hit.any() and (a.channels.q == 0).all()
    assert nhit > 20
    assert np.array_equal(rng_a, rng_b), 'final rng_states differ'


def test_native_calls_do_not_scale_with_events(cuda):
    """One-photon events on the one-channel box detector: the batched DAQ is
    one native call per group, however many events the group holds."""
    from chroma.gpu import _native
    from test_gpu_daq import _box_sim, _one_photon
    sim = _box_sim()
    assert sim.daq_events
    calls = []

    def hook(name, fn):
        if name.startswith('chr_daq'):
            calls.append(name)
        return fn()

    counts = {}
    for nevents in (250, 1000):
        del calls[:]
        saved, _native.call_hook = _native.call_hook, hook
        try:
            evs = list(sim.simulate((_one_photon(100.0) for _ in range(nevents)), run_daq=True))
        finally:
            _native.call_hook = saved
        assert len(evs) == nevents and all(ev.channels is not None and len(ev.channels.t) == 1 for ev in evs)
        assert sum(bool(ev.channels.hit[0]) for ev in evs) > nevents // 10
        counts[nevents] = list(calls)
    assert counts[1000] == counts[250] == ['chr_daq_acquire_events']


def test_many_daqs_are_not_batched(cuda, daq_detector):
    from chroma import gpu
    from test_gpu_daq import _made_records
    photons, kind = _made_records(daq_detector)
    gdet = gpu.GPUDetector(daq_detector)
    gp = gpu.GPUPhotons(photons, copy_flags=True, copy_triangles=True, copy_weights=True)
    rng = gpu.get_rng_states(64 * 64, seed=5)
    with pytest.raises(ValueError):
        gpu.GPUDaq(gdet, ndaq=5).acquire_events(gp, rng, BOUNDS)
