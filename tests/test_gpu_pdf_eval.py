"""The likelihood layer on the device: GPUDaq.acquire_events_many
(chr_daq_acquire_events_many) against the CPU oracle run event by event and
against the GPU's own begin / acquire / end loop, bit for bit; Simulation's
eval_pdf / create_pdf with the copies batched (pdf_rows) against the per-copy
loop and the documented sequence done by hand; setup_kernel / eval_kernel; and
chroma.likelihood.Likelihood end to end."""
import numpy as np
import pytest

import oracle
from test_daq_events import BOUNDS, SIZES
from test_pdf_eval import (EVAL_K, EVAL_MAX_BLOCKS, EVAL_NREPS, EVAL_NTPB, EVAL_SEED, EVAL_TRANGE, EVAL_TWIDTH,
                           MANY_CASES, eval_sources, expected_float_charges, oracle_events_many)

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


def _rows(chans, nevents):
    """(time words, charge words as f32 bits, histories) of acquire_events_many's GPUChannels, one row per event"""
    return (chans.t.get().view(np.uint32).reshape(nevents, -1), chans.q.get().view(np.uint32).reshape(nevents, -1),
            chans.flags.get().reshape(nevents, -1))


def _photon_words(gp):
    got = gp.get()
    return [np.asarray(getattr(got, f)).copy() for f in ('t', 'flags', 'last_hit_triangles', 'weights', 'pos')]


def _check_many(daq, chans, want, unit, nevents, label):
    t, q, fl = want
    nch = daq.nchannels
    assert chans.ndaq == nevents * daq.ndaq and chans.stride == nch and len(chans.t) == t.size
    got_t, got_q, got_fl = _rows(chans, nevents)
    assert np.array_equal(got_t, t), label + ': earliest time words differ'
    assert np.array_equal(got_fl, fl), label + ': channel histories differ'
    assert np.array_equal(got_q, expected_float_charges(q, nch, unit).view(np.uint32)), label + ': charges differ'
    q_int = daq._event_rows[1][:q.size].get().reshape(nevents, -1)
    assert np.array_equal(q_int, q), label + ': charge words differ'


# ------------------------------------------------------------------ 1. the made records
@pytest.mark.parametrize('ndaq,ntpb,max_blocks,weight', MANY_CASES)
def test_made_records(cuda, daq_detector, ndaq, ntpb, max_blocks, weight):
    from chroma import gpu
    from test_gpu_daq import _made_records
    photons, kind = _made_records(daq_detector)
    host = oracle.HostPhotons(photons)
    nslots = 64 * 1024
    nevents = len(SIZES)
    gdet = gpu.GPUDetector(daq_detector)
    gp = gpu.GPUPhotons(photons, copy_flags=True, copy_triangles=True, copy_weights=True)
    before = _photon_words(gp)
    st = oracle.rng_init(nslots, seed=5)
    normal = np.zeros(2 * nslots, np.uint32)
    t, q, fl, _, _ = oracle_events_many(daq_detector, host, st, normal, nslots, BOUNDS, ndaq, ntpb, max_blocks, weight)
    assert all((q[e] > 0).any() for e in np.flatnonzero(SIZES >= 63)) and (t[SIZES == 0] == MAXBITS).all()

    rng = gpu.get_rng_states(nslots, seed=5)
    daq = gpu.GPUDaq(gdet, ndaq=ndaq)
    chans = daq.acquire_events_many(gp, rng, BOUNDS, nthreads_per_block=ntpb, max_blocks=max_blocks, weight=weight)
    _check_many(daq, chans, (t, q, fl), gdet.charge_unit, nevents, 'against the oracle')
    assert np.array_equal(rng.get().reshape(-1), st), 'RNG slot states differ from the oracle'
    assert np.array_equal(rng.normal_cache.get(), normal), 'normal cache differs from the oracle'
    for a, b in zip(before, _photon_words(gp)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), 'the DAQ changed the photons'

    # the GPU's own per-event loop, from fresh states of the same seed
    rng2 = gpu.get_rng_states(nslots, seed=5)
    daq2 = gpu.GPUDaq(gdet, ndaq=ndaq)
    loop = []
    for start, n in zip(BOUNDS[:-1], SIZES):
        daq2.begin_acquire()
        daq2.acquire(gp, rng2, nthreads_per_block=ntpb, max_blocks=max_blocks, start_photon=int(start),
                     nphotons=int(n), weight=weight)
        q_int = daq2.channel_q_int_gpu.get()
        ch = daq2.end_acquire()
        loop.append((ch.t.get().view(np.uint32), ch.q.get().view(np.uint32), ch.flags.get(), q_int))
    want = tuple(np.array([r[k] for r in loop]) for k in range(4))
    for got, w, name in zip(_rows(chans, nevents), want, ('time words', 'charges', 'histories')):
        assert np.array_equal(got, w), name + ' differ from the per-event loop'
    assert np.array_equal(daq._event_rows[1][:q.size].get().reshape(nevents, -1), want[3])
    assert np.array_equal(rng.get(), rng2.get()), 'RNG slot states differ from the per-event loop'
    assert np.array_equal(rng.normal_cache.get(), rng2.normal_cache.get()), 'normal cache differs from the loop'


def test_one_daq_is_refused(cuda, daq_detector):
    from chroma import gpu
    from test_gpu_daq import _made_records
    photons, kind = _made_records(daq_detector)
    gdet = gpu.GPUDetector(daq_detector)
    gp = gpu.GPUPhotons(photons, copy_flags=True, copy_triangles=True, copy_weights=True)
    rng = gpu.get_rng_states(64 * 64, seed=5)
    with pytest.raises(ValueError):
        gpu.GPUDaq(gdet, ndaq=1).acquire_events_many(gp, rng, BOUNDS)
    chans = gpu.GPUDaq(gdet, ndaq=3).acquire_events_many(gp, rng, BOUNDS[:1])       # no event: nothing to do
    assert chans.ndaq == 0 and len(chans.t) == 0


# ------------------------------------------------------------------ 2. after a real propagate
def test_after_propagate(cuda, daq_detector, small_packed):
    """What a real propagate leaves (test_daq_parity's 20,000 isotropic photons), in three events."""
    from chroma import gpu
    from chroma.photon_source import isotropic
    from test_gpu_parity import _run_both, _compare
    photons = isotropic(20000, seed=31)
    nslots = 64 * 1024
    gp, host, rng, st, _ = _run_both(daq_detector, small_packed, photons, nslots, 64, 1024, 100, seed=5)
    _compare(host, gp, 'propagate before DAQ')
    bounds = np.array([0, 700, 9001, 20000], np.int64)
    gdet = gpu.GPUDetector(daq_detector)
    normal = np.zeros(2 * nslots, np.uint32)
    daq = gpu.GPUDaq(gdet, ndaq=5)
    for ntpb, max_blocks in ((64, 1024), (64, 16)):
        t, q, fl, _, _ = oracle_events_many(daq_detector, host, st, normal, nslots, bounds, 5, ntpb, max_blocks)
        assert (q.reshape(3, 5, -1).sum(axis=2) > 0).all()
        chans = daq.acquire_events_many(gp, rng, bounds, nthreads_per_block=ntpb, max_blocks=max_blocks)
        _check_many(daq, chans, (t, q, fl), gdet.charge_unit, 3, 'after a propagate, %d blocks' % max_blocks)
        assert np.array_equal(rng.get().reshape(-1), st)
        assert np.array_equal(rng.normal_cache.get(), normal)


# ------------------------------------------------------------------ 3. eval_pdf three ways
def _eval_sim(detector, pdf_rows, group_bytes):
    from chroma.sim import Simulation
    sim = Simulation(detector, seed=EVAL_SEED, nthreads_per_block=EVAL_NTPB, max_blocks=EVAL_MAX_BLOCKS)
    sim.pdf_rows = pdf_rows
    sim.daq_group_bytes = group_bytes
    return sim


def _observed(sim, sources):
    ev, = sim.simulate([sources[0]], run_daq=True, max_steps=100)
    return ev.channels


def _eval_state(sim, result):
    p = sim.gpu_pdf
    return dict(hitcount=p.eval_hitcount_gpu.get(), bincount=p.eval_bincount_gpu.get(),
                nearest=p.nearest_mc_gpu.get().view(np.uint32), rng=sim.rng_states.get(),
                normal=sim.rng_states.normal_cache.get(), result=[np.asarray(r).copy() for r in result])


def _eval_by_hand(sim, channels, sources, ndaq):
    """the sequence eval_pdf documents, call by call"""
    from chroma import gpu
    kw = dict(nthreads_per_block=sim.nthreads_per_block, max_blocks=sim.max_blocks)
    pdf = sim.gpu_pdf
    pdf.setup_pdf_eval(channels.hit, channels.t, channels.q, EVAL_TWIDTH, EVAL_TRANGE, 1, (-0.5, 49.5),
                       min_bin_content=EVAL_K, time_only=True)
    pdf.clear_pdf_eval()
    daq = gpu.GPUDaq(sim.gpu_geometry, ndaq)
    for src in sources:
        n = len(src)
        gp = gpu.GPUPhotons(src, ncopies=EVAL_NREPS)
        gp.propagate(sim.gpu_geometry, sim.rng_states, max_steps=100, use_weights=False, **kw)
        for c in range(EVAL_NREPS):
            daq.begin_acquire()
            daq.acquire(gp, sim.rng_states, start_photon=c * n, nphotons=n, **kw)
            pdf.accumulate_pdf_eval(daq.end_acquire())
    return pdf.get_pdf_eval()


@pytest.mark.parametrize('ndaq', [5, 1])
def test_eval_pdf_three_ways(cuda, daq_detector, ndaq):
    """pdf_rows True (copies in groups of 2 + 1), False, and the documented
    sequence by hand: the same accumulator words, results, rng_states and
    normal cache.  The seeds are those of tests/test_pdf_eval.py, for which the
    oracle puts channel 0 above min_bin_content and channel 1 below it."""
    from chroma.sim import pdf_copy_groups
    sources = eval_sources()
    nch = 2
    budget = 16 * ndaq * nch * 2 + 9
    assert pdf_copy_groups(EVAL_NREPS, ndaq, nch, budget) == [(0, 2), (2, 3)]
    runs = []
    for how in ('rows', 'loop', 'hand'):
        sim = _eval_sim(daq_detector, how == 'rows', budget)
        channels = _observed(sim, sources)
        assert channels.hit.all()
        if how == 'hand':
            result = _eval_by_hand(sim, channels, sources, ndaq)
        else:
            result = sim.eval_pdf(channels, iter(sources), EVAL_TWIDTH, EVAL_TRANGE, 1, (-0.5, 49.5),
                                  min_bin_content=EVAL_K, nreps=EVAL_NREPS, ndaq=ndaq, max_steps=100)
        runs.append(_eval_state(sim, result))
    rows, loop, hand = runs
    for other, name in ((loop, 'the per-copy loop'), (hand, 'the sequence by hand')):
        for key in ('hitcount', 'bincount', 'nearest', 'rng', 'normal'):
            assert np.array_equal(rows[key], other[key]), '%s differs from %s' % (key, name)
        for a, b in zip(rows['result'], other['result']):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), 'the result differs from %s' % name
    hitcount, value, uncert = rows['result']
    assert (hitcount == len(sources) * EVAL_NREPS * ndaq).all() and (value > 0).all() and np.isfinite(value).all()
    if ndaq == 5:
        assert (rows['bincount'] >= EVAL_K).any() and (rows['bincount'] < EVAL_K).any(), rows['bincount']
        assert (rows['normal'] != 0).any()


# ------------------------------------------------------------------ 4. native calls per source
def test_native_calls_do_not_scale_with_nreps(cuda, daq_detector):
    from chroma.gpu import _native
    sources = eval_sources()[:2]
    sim = _eval_sim(daq_detector, True, 64 << 20)
    channels = _observed(sim, sources)
    calls = []

    def hook(name, fn):
        if name.startswith('chr_daq') or name.startswith('chr_pdf'):
            calls.append(name)
        return fn()

    lists = {}
    for ndaq in (5, 1):
        for nreps in (4, 16):
            del calls[:]
            saved, _native.call_hook = _native.call_hook, hook
            try:
                hitcount, _, _ = sim.eval_pdf(channels, iter(sources), EVAL_TWIDTH, EVAL_TRANGE, 1, (-0.5, 49.5),
                                              min_bin_content=EVAL_K, nreps=nreps, ndaq=ndaq, max_steps=100)
            finally:
                _native.call_hook = saved
            assert (hitcount == len(sources) * nreps * ndaq).all()
            lists[ndaq, nreps] = list(calls)
    acquire = {5: 'chr_daq_acquire_events_many', 1: 'chr_daq_acquire_events'}
    for ndaq in (5, 1):
        assert lists[ndaq, 4] == lists[ndaq, 16] == len(sources) * [
            acquire[ndaq], 'chr_pdf_accumulate_bincount', 'chr_pdf_accumulate_nearest']


# ------------------------------------------------------------------ 5. create_pdf
def test_create_pdf(cuda, daq_detector):
    from chroma import gpu
    sources = eval_sources()
    binning = (50, (-0.5, 49.5), 5, (-0.5, 999.5))
    budget = 16 * 2 * 2 + 9                       # copies in groups of 2 + 1
    runs = []
    for how in ('rows', 'loop', 'hand'):
        sim = _eval_sim(daq_detector, how == 'rows', budget)
        if how == 'hand':
            kw = dict(nthreads_per_block=sim.nthreads_per_block, max_blocks=sim.max_blocks)
            sim.gpu_pdf.setup_pdf(2, *binning)
            for src in sources:
                gp = gpu.GPUPhotons(src, ncopies=EVAL_NREPS)
                gp.propagate(sim.gpu_geometry, sim.rng_states, max_steps=100, **kw)
                for c in range(EVAL_NREPS):
                    sim.gpu_daq.begin_acquire()
                    sim.gpu_daq.acquire(gp, sim.rng_states, start_photon=c * len(src), nphotons=len(src), **kw)
                    sim.gpu_pdf.add_hits_to_pdf(sim.gpu_daq.end_acquire())
            hitcount, pdf = sim.gpu_pdf.get_pdfs()
        else:
            hitcount, pdf = sim.create_pdf(iter(sources), *binning, nreps=EVAL_NREPS)
        assert sim.gpu_pdf.events_in_histogram == len(sources) * EVAL_NREPS
        runs.append((hitcount, pdf, sim.rng_states.get(), sim))
    for other in runs[1:]:
        for a, b in zip(runs[0][:3], other[:3]):
            assert np.array_equal(a, b)
    hitcount, pdf, _, sim = runs[0]
    # the reference's own check (test/test_pdf.py testSimPDF)
    assert pdf.shape == (2, 50, 5) and (hitcount > 0).any() and (pdf > 0).any()
    assert all(hitcount[i] == pdf[i].sum() for i in range(len(hitcount)))
    # the same configuration again adds to the histogram, a changed one starts again
    again, pdf2 = sim.create_pdf(iter(sources[:1]), *binning, nreps=EVAL_NREPS)
    assert (again >= hitcount).all() and again.sum() > hitcount.sum() and (pdf2 >= pdf).all()
    assert sim.gpu_pdf.events_in_histogram == (len(sources) + 1) * EVAL_NREPS
    fresh, pdf3 = sim.create_pdf(iter(sources[:1]), 20, (-0.5, 49.5), 5, (-0.5, 999.5), nreps=EVAL_NREPS)
    assert pdf3.shape == (2, 20, 5) and fresh.sum() <= 2 * EVAL_NREPS and fresh.sum() == pdf3.sum()
    assert sim.gpu_pdf.events_in_histogram == EVAL_NREPS


# ------------------------------------------------------------------ 6. the kernel estimator
def test_kernel_estimator_matches_the_loop_by_hand(cuda, daq_detector):
    from chroma import gpu
    sources = eval_sources()
    trange, qrange, nreps, ndaq = (-0.5, 49.5), (-0.5, 9.5), 2, 2

    def by_hand(sim, srcs, accumulate):
        kw = dict(nthreads_per_block=sim.nthreads_per_block, max_blocks=sim.max_blocks)
        for src in srcs:
            gp = gpu.GPUPhotons(src, ncopies=nreps)
            gp.propagate(sim.gpu_geometry, sim.rng_states, max_steps=100, **kw)
            for c in range(nreps):
                for _ in range(ndaq):
                    sim.gpu_daq.begin_acquire()
                    sim.gpu_daq.acquire(gp, sim.rng_states, start_photon=c * len(src), nphotons=len(src), **kw)
                    accumulate(sim.gpu_daq.end_acquire())

    runs = []
    for hand in (False, True):
        sim = _eval_sim(daq_detector, True, 64 << 20)
        channels = _observed(sim, sources)
        k = sim.gpu_pdf_kernel
        if hand:
            k.setup_moments(2, trange, qrange, time_only=True)
            by_hand(sim, sources[:2], k.accumulate_moments)
            k.compute_bandwidth(channels.hit, channels.t, channels.q, scale_factor=2.0)
            k.setup_kernel(channels.hit, channels.t, channels.q)
            k.clear_kernel()
            by_hand(sim, sources[1:], k.accumulate_kernel)
            result = k.get_kernel_eval()
        else:
            sim.setup_kernel(channels, iter(sources[:2]), trange, qrange, nreps=nreps, ndaq=ndaq, scale_factor=2.0)
            result = sim.eval_kernel(channels, iter(sources[1:]), trange, qrange, nreps=nreps, ndaq=ndaq)
        runs.append((result, k.inv_time_bandwidths_gpu.get(), sim.rng_states.get(), channels))
    (res_a, bw_a, rng_a, channels), (res_b, bw_b, rng_b, _) = runs
    assert np.array_equal(bw_a.view(np.uint32), bw_b.view(np.uint32)) and np.array_equal(rng_a, rng_b)
    for a, b in zip(res_a, res_b):
        assert np.asarray(a).dtype == np.asarray(b).dtype and np.asarray(a).tobytes() == np.asarray(b).tobytes()
    hitcount, value, _ = res_a
    assert (hitcount[channels.hit] > 0).all() and np.isfinite(value[channels.hit]).all()
    assert (value[channels.hit] > 0).all()


# ------------------------------------------------------------------ 7. Likelihood end to end
def _flash(n, t0, seed):
    """n photons from the middle of test_gpu_daq._box_sim's 10 mm box, straight at its +z face, at time t0"""
    from chroma.event import Photons
    r = np.random.RandomState(seed)
    pos = np.zeros((n, 3), np.float32)
    dir = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    phi = r.uniform(0, 2 * np.pi, n).astype(np.float32)
    pol = np.zeros_like(pos)
    pol[:, 0], pol[:, 1] = np.cos(phi), np.sin(phi)
    return Photons(pos=pos, dir=dir, pol=pol, t=np.full(n, t0, np.float32), wavelengths=np.full(n, 400.0, np.float32))


def test_likelihood_prefers_the_true_time(cuda):
    """A 200-photon flash at 100 ns is likelier given sources at 100 ns than given
    sources at 130 ns: 25 sigma of the 1.2 ns time spread away, so none of their
    simulated times comes near the observed one and the adaptive bin widens to
    tens of ns.  Only the sign is asserted.  For these seeds the CPU oracle,
    run through the same sequence, gives an observed time of 96.26 ns and NLLs
    of 1.57 (40 nearest times within 2.4 ns) against 4.11 (within 30.6 ns)."""
    from chroma.likelihood import Likelihood
    from test_gpu_daq import _box_sim
    sim = _box_sim()                                  # seed 17
    ev, = sim.simulate([_flash(200, 100.0, seed=1)], run_daq=True)
    assert ev.channels.hit.all() and abs(float(ev.channels.t[0]) - 100.0) < 8.0
    lik = Likelihood(sim, ev)
    nevals, nreps, ndaq = 4, 2, 5
    nll = {}
    for t0 in (100.0, 130.0):
        sources = (_flash(200, t0, seed=10 + i) for i in range(nevals))
        nll[t0] = lik.eval(sources, nevals, nreps=nreps, ndaq=ndaq)
        assert isinstance(nll[t0], float) and np.isfinite(nll[t0])
    assert nll[100.0] < nll[130.0], nll
