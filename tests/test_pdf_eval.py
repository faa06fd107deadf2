"""The likelihood layer (Simulation.eval_pdf / create_pdf / setup_kernel /
eval_kernel, chroma.likelihood.Likelihood) and the batched ndaq > 1 DAQ under
it (chr_daq_acquire_events_many, chr_pdf_bin_hits_rows), as far as they can be
checked without a GPU: the entry point's refusals (all made before a device is
touched), the copy grouping, that stacked DAQ rows accumulate as the rows one
after another do (on the oracle), that the events tests/test_gpu_pdf_eval.py
feeds the kernel exercise what it can get wrong, and Likelihood's arithmetic
over a stub simulation."""
import ctypes

import numpy as np
import pytest

import oracle
from test_daq_events import BOUNDS, SIZES

CHR_OK, CHR_ERR_INVALID = 0, 1
# (ndaq, nthreads_per_block, max_blocks, global weight) of the GPU test on the made records: ndaq below, at
# and above the workgroup; chains of up to ceil(2000 / 3) = 667 positions; n_e below max_blocks; a weight
MANY_CASES = [(2, 32, 1024, 1.0), (5, 64, 16, 1.0), (64, 64, 16, 1.0), (65, 64, 16, 1.0), (150, 64, 3, 0.5)]


# ------------------------------------------------------------------ entry points
def _call(bounds, nphotons=3000, nevents=None, rng_nslots=64 * 1024, ndaq=5, ntpb=64, max_blocks=1024, null=(),
          cdf_len=51, nchannels=2):
    """chr_daq_acquire_events_many with made-up device addresses: every refusal
    comes before the first dereference or launch, so none of them is ever used.
    The accepted calls the refusals are set against all have nevents = 0, which
    returns after the last check and before the first launch."""
    from chroma.gpu import _native
    from chroma.gpu.daq import _DetectorDesc
    fake = 0x1000
    arg = lambda name: None if name in null else fake      # noqa: E731
    ph = _native.PhotonsDesc(*[fake] * 9)
    if 'photon_t' in null:
        ph.d_t = None
    det = _DetectorDesc(arg('s2c'), arg('time_cdf_x'), fake, fake, fake, nchannels, cdf_len, 51, 1.5 / 2 ** 16)
    bounds = np.ascontiguousarray(bounds, np.int64)
    nevents = len(bounds) - 1 if nevents is None else nevents
    return _native.lib().chr_daq_acquire_events_many(
        None if 'ph' in null else ctypes.byref(ph), nphotons, None if 'bounds' in null else bounds.ctypes.data,
        nevents, arg('rng'), rng_nslots, arg('normal'), 0x4, arg('solid_map'),
        None if 'det' in null else ctypes.byref(det), arg('time_int'), arg('q_int'), arg('history'), arg('q'), ndaq,
        ctypes.c_float(1.0), ntpb, max_blocks, None)


def _last_error():
    from chroma.gpu import _native
    return _native.lib().chr_last_error()


def test_entry_points_are_exported_and_declared():
    from chroma.gpu import _native
    from test_native_abi import declared_symbols
    lib = ctypes.CDLL(_native.library_path())
    for name in ('chr_daq_acquire_events_many', 'chr_pdf_bin_hits_rows'):
        assert name in _native.EXPORTED and name in declared_symbols() and hasattr(lib, name)


def test_no_events_is_ok():
    assert _call([0]) == CHR_OK
    assert _call([7]) == CHR_OK


@pytest.mark.parametrize('null', ['ph', 'photon_t', 'bounds', 'rng', 'normal', 'solid_map', 'det', 's2c', 'time_int',
                                  'q_int', 'history', 'q'])
def test_refuses_null_arguments(null):
    assert _call([0]) == CHR_OK                                   # the call that is refused below, accepted
    assert _call([0], null=(null,)) == CHR_ERR_INVALID
    assert b'null' in _last_error()


def test_refuses_missing_cdfs():
    assert _call([0], null=('time_cdf_x',)) == CHR_ERR_INVALID and b'CDF' in _last_error()
    assert _call([0], cdf_len=1) == CHR_ERR_INVALID and b'CDF' in _last_error()


def test_refuses_one_daq_and_wide_blocks():
    assert _call([0], ndaq=2, ntpb=1024) == CHR_OK
    for ndaq in (1, 0, -3):
        assert _call([0], ndaq=ndaq) == CHR_ERR_INVALID and b'ndaq' in _last_error()
    assert _call([0], ntpb=1025) == CHR_ERR_INVALID and b'1024' in _last_error()
    assert _call([0], ntpb=0) == CHR_ERR_INVALID
    assert _call([0], max_blocks=0) == CHR_ERR_INVALID
    assert _call([0], nchannels=0) == CHR_ERR_INVALID


def test_refuses_bad_bounds():
    assert _call([0, 10, 9, 20], nevents=0) == CHR_OK
    assert _call([0, 10, 9, 20]) == CHR_ERR_INVALID and b'decrease' in _last_error()
    assert _call([-1, 10]) == CHR_ERR_INVALID and b'outside' in _last_error()       # below the first photon
    assert _call([0, 10, 3001]) == CHR_ERR_INVALID and b'outside' in _last_error()  # beyond the photon count
    assert _call([0, 3001, 3000]) == CHR_ERR_INVALID                                # beyond it in the middle
    assert _call([0], nevents=-1) == CHR_ERR_INVALID


def test_refuses_too_few_rng_slots():
    # the slots of the per-event launches: nthreads_per_block * min(max_blocks, largest event)
    big = [0, 2000]
    assert _call(big, nevents=0, rng_nslots=1) == CHR_OK          # no event: nothing draws (and nothing is launched)
    assert _call(big, rng_nslots=64 * 2000 - 1, ntpb=64, max_blocks=4096) == CHR_ERR_INVALID
    assert b'rng states' in _last_error()
    assert _call(big, rng_nslots=64 * 8 - 1, ntpb=64, max_blocks=8) == CHR_ERR_INVALID
    assert b'rng states' in _last_error()


def test_refuses_more_than_2_to_31_words():
    assert _call([0], ndaq=2 ** 30 + 1) == CHR_OK
    assert _call([0, 0], nevents=1, ndaq=2 ** 30 + 1, rng_nslots=0) == CHR_ERR_INVALID     # 1 x (2^30 + 1) x 2
    assert b'2^31' in _last_error()


# ------------------------------------------------------------------ grouping
def test_copy_group_arithmetic():
    from chroma.sim import Simulation, pdf_copy_groups
    # the reference's likelihood point on the 10,055-channel detector: 16 copies of 50 DAQ copies
    per = Simulation.daq_group_bytes // (16 * 50 * 10055)
    assert per == 8 and pdf_copy_groups(16, 50, 10055, Simulation.daq_group_bytes) == [(0, 8), (8, 16)]
    assert pdf_copy_groups(16, 1, 10055, Simulation.daq_group_bytes) == [(0, 16)]
    # a budget below one copy's rows still gives groups of one
    assert pdf_copy_groups(3, 50, 29007, 1000) == [(0, 1), (1, 2), (2, 3)]
    # the GPU test's 2 + 1
    assert pdf_copy_groups(3, 5, 2, 16 * 5 * 2 * 2 + 7) == [(0, 2), (2, 3)]
    assert pdf_copy_groups(3, 1, 2, 16 * 2 * 2) == [(0, 2), (2, 3)]
    # every copy once, in order
    for nreps in (1, 4, 16, 17):
        for budget in (1, 16 * 5 * 2 * 3, 64 << 20):
            groups = pdf_copy_groups(nreps, 5, 2, budget)
            assert [c for a, b in groups for c in range(a, b)] == list(range(nreps))
    assert pdf_copy_groups(0, 5, 2, 64 << 20) == []


# ------------------------------------------------------------------ stacked rows, on the oracle
def _accumulate(event_hit, event_time, mc, ndaq, k, w, tr, hc, bc, near):
    nhit = int(event_hit.sum())
    c2h = np.maximum(0, np.cumsum(event_hit) - 1).astype(np.uint32)
    h2c = np.flatnonzero(event_hit).astype(np.uint32)
    queues = np.ones(nhit * (ndaq + 1), np.uint32)
    oracle.pdf_accumulate_bincount(event_hit, event_time, mc, ndaq, hc, bc, queues, w, tr, k, c2h)
    oracle.pdf_accumulate_nearest(h2c, queues, event_time, mc, ndaq, near, k)


def test_stacked_rows_accumulate_as_rows_in_order():
    """accumulate_pdf_eval over nrows * ndaq stacked copies against nrows
    accumulations of ndaq copies in order: hitcount, bincount and the nearest
    tables word for word (bincount_kernel walks the copies serially per
    channel; the k smallest of a union are the k smallest of the parts' k
    smallest)."""
    n, w, tr = 60, 2.0, (-10.0, 100.0)
    crossed = nans = 0
    for nrows, ndaq, k, nan, seed in ((16, 1, 10, False, 1), (7, 5, 10, False, 2), (7, 5, 10, True, 3),
                                      (16, 50, 320, False, 4), (9, 3, 4, False, 5)):
        r = np.random.default_rng(seed)
        event_hit = (r.random(n) < 0.7).astype(np.uint32)
        event_time = r.uniform(0, 90, n).astype(np.float32)
        # per channel a spread from well inside the minimum bin to far outside it, 90 % of the copies hit
        sigma = r.uniform(0.3, 12.0, n)
        mc = (event_time + r.normal(size=(nrows * ndaq, n)) * sigma).astype(np.float32)
        mc[r.random(mc.shape) < 0.1] = 1e9
        if nan:
            mc[r.random(mc.shape) < 0.05] = np.nan
            nans += int(np.isnan(mc).sum() > 0)
        nhit = int(event_hit.sum())
        rows = (np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.full(nhit * k, 1e9, np.float32))
        for i in range(nrows):
            _accumulate(event_hit, event_time, mc[i * ndaq:(i + 1) * ndaq].reshape(-1), ndaq, k, w, tr, *rows)
        stacked = (np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.full(nhit * k, 1e9, np.float32))
        _accumulate(event_hit, event_time, mc.reshape(-1), nrows * ndaq, k, w, tr, *stacked)
        label = '%d x %d, k = %d' % (nrows, ndaq, k)
        assert np.array_equal(rows[0], stacked[0]) and rows[0].max() > 0, label + ': hitcount'
        assert np.array_equal(rows[1], stacked[1]), label + ': bincount'
        assert np.array_equal(rows[2].view(np.uint32), stacked[2].view(np.uint32)), label + ': nearest tables'
        hit = event_hit != 0
        crossed += int((rows[1][hit] >= k).any() and (rows[1][hit] < k).any())
        assert (rows[2] < 1e8).any()
    assert crossed >= 1, 'no case has bin counts on both sides of min_bin_content'
    assert nans >= 1, 'no case holds NaN times'


# ------------------------------------------------------------------ the GPU test's inputs, on the oracle
def oracle_events_many(detector, host, st, normal, nslots, bounds, ndaq, ntpb, max_blocks, weight=1.0):
    """oracle.daq(raw=True, ndaq=ndaq) per event [bounds[e], bounds[e+1]), in
    order, on the one state array `st` and normal cache `normal`: rows of (time
    words, charge words, histories), each (nevents, ndaq * nchannels), and the
    states and caches after every event."""
    from chroma.gpu.detector import cdf_arrays
    nch = int(detector.num_channels())
    unit = np.float32(detector.charge_cdf[0][-1] / 2 ** 16)
    rows, states, normals = [], [], []
    for start, end in zip(bounds[:-1], bounds[1:]):
        rows.append(oracle.daq(host, detector.solid_id, detector.solid_id_to_channel_index,
                               cdf_arrays(detector.time_cdf), cdf_arrays(detector.charge_cdf), unit, st, nslots,
                               normal_cache=normal, start=int(start), n=int(end - start), ndaq=ndaq, nchannels=nch,
                               global_weight=weight, nthreads_per_block=ntpb, max_blocks=max_blocks, raw=True))
        states.append(st.copy())
        normals.append(normal.copy())
    t, q, fl = (np.array([r[k] for r in rows]) for k in range(3))
    return t, q, fl, states, normals


def expected_float_charges(q, nchannels, unit):
    """What chr_daq_end after begin_acquire's fill leaves of the charge words `q`
    (rows of ndaq * nchannels): the first nchannels of a row converted, the rest 0."""
    out = np.zeros(q.shape, np.float32)
    out[:, :nchannels] = q[:, :nchannels].astype(np.float32) * np.float32(unit)
    return out


@pytest.mark.parametrize('ndaq,ntpb,max_blocks,weight', MANY_CASES)
def test_made_events_exercise_the_many_kernel(small_detector, ndaq, ntpb, max_blocks, weight):
    from test_gpu_daq import _made_records, N_MADE
    saved = small_detector.time_cdf, small_detector.charge_cdf
    small_detector.set_time_dist_gaussian(1.2, -6.0, 6.0)
    small_detector.set_charge_dist_gaussian(1.0, 0.1, 0.5, 1.5)
    try:
        photons, kind = _made_records(small_detector)
        assert BOUNDS[-1] < N_MADE and BOUNDS[0] > 0
        host = oracle.HostPhotons(photons)
        nch = int(small_detector.num_channels())
        nslots = 64 * 1024
        st = oracle.rng_init(nslots, seed=5)
        normal = np.zeros(2 * nslots, np.uint32)
        before = st.copy()
        t, q, fl, states, normals = oracle_events_many(small_detector, host, st, normal, nslots, BOUNDS, ndaq, ntpb,
                                                       max_blocks, weight)
        maxbits = np.float32(1e9).view(np.uint32)
        changed = np.zeros(nslots, np.int64)
        for e, n in enumerate(SIZES):
            moved = (states[e].reshape(6, nslots) != before.reshape(6, nslots)).any(axis=0)
            changed += moved
            slot = np.flatnonzero(moved)
            # only slots tid + ntpb * b with tid < min(ntpb, ndaq) and b < min(max_blocks, n_e) draw
            assert (slot % ntpb < min(ntpb, ndaq)).all() and (slot // ntpb < min(max_blocks, n)).all()
            if n == 0:
                assert not moved.any() and (t[e] == maxbits).all() and (q[e] == 0).all() and (fl[e] == 0).all()
            if n >= 63:
                assert (q[e] > 0).any() and (t[e] < maxbits).any() and (fl[e] != 0).any()
            before = states[e]
        assert (SIZES == 0).any() and (SIZES < max_blocks).any()
        # a slot draws in two or more events: its state and cache are carried
        assert (changed >= 2).any()
        # the normal cache is non-empty between events
        assert any((nc[:nslots] == 1).any() for nc in normals[:-1])
        # a block chain (positions b, b + max_blocks, ...) holds two or more detected photons of one event
        chained = False
        for start, end in zip(BOUNDS[:-1], BOUNDS[1:]):
            idx, _ = oracle.hits(host, small_detector.solid_id, small_detector.solid_id_to_channel_index,
                                 start=int(start), n=int(end - start))
            per_block = np.bincount((idx - start) % max_blocks, minlength=max_blocks)
            chained |= bool((per_block >= 2).any())
        assert chained == (max_blocks < SIZES.max())
        # a work-item takes a second copy i = tid + ntpb: the copies beyond ntpb hold hits
        if ndaq > ntpb:
            assert (q[:, ntpb * nch:] > 0).any()
        # every copy of a row is used
        assert all((q[:, i * nch:(i + 1) * nch] > 0).any() for i in range(ndaq))
    finally:
        small_detector.time_cdf, small_detector.charge_cdf = saved


def test_cases_cover_what_they_claim():
    assert any(n > t for n, t, _, _ in MANY_CASES) and any(n == t for n, t, _, _ in MANY_CASES)
    assert any(n < t for n, t, _, _ in MANY_CASES) and any(w != 1.0 for _, _, _, w in MANY_CASES)
    assert max(-(-int(SIZES.max()) // b) for _, _, b, _ in MANY_CASES) == 667
    assert sum(b < SIZES.max() for _, _, b, _ in MANY_CASES) >= 2


# ------------------------------------------------------------------ eval_pdf's sequence, on the oracle
# tests/test_gpu_pdf_eval.py::test_eval_pdf_three_ways: Simulation(seed, 64 x 256 slots) on the 2-PMT detector,
# the observed event simulated from the first of three 2000-photon isotropic sources, then eval_pdf over the
# three with nreps = 3, min_bin_content = 4 and the minimum bin width below
EVAL_SEED, EVAL_SOURCE_SEEDS, EVAL_NTPB, EVAL_MAX_BLOCKS = 23, (101, 102, 103), 64, 256
EVAL_NREPS, EVAL_K, EVAL_TWIDTH, EVAL_TRANGE = 3, 4, 0.2, (-0.5, 999.5)
# with these the oracle puts 7 of channel 0's 45 simulated times (ndaq = 5) inside the minimum bin and none of
# channel 1's, whose nearest are 0.101 and 0.106 away against the half width of 0.1


def eval_sources():
    from chroma.photon_source import isotropic
    return [isotropic(2000, seed=s) for s in EVAL_SOURCE_SEEDS]


def oracle_eval_pdf(detector, packed, ndaq, max_steps=100):
    """Simulation.eval_pdf's documented sequence on the oracle, after the
    simulate(run_daq=True) of the first source that makes the observed event:
    dict of the observed (hit, t, q) and the accumulators."""
    from chroma.gpu.detector import cdf_arrays
    nslots = EVAL_NTPB * EVAL_MAX_BLOCKS
    nch = int(detector.num_channels())
    unit = np.float32(detector.charge_cdf[0][-1] / 2 ** 16)
    st = oracle.rng_init(nslots, seed=EVAL_SEED)
    normal = np.zeros(2 * nslots, np.uint32)
    sources = eval_sources()

    def daq(host, start, n, copies):
        return oracle.daq(host, detector.solid_id, detector.solid_id_to_channel_index, cdf_arrays(detector.time_cdf),
                          cdf_arrays(detector.charge_cdf), unit, st, nslots, normal_cache=normal, start=start, n=n,
                          ndaq=copies, nchannels=nch, nthreads_per_block=EVAL_NTPB, max_blocks=EVAL_MAX_BLOCKS)

    host = oracle.HostPhotons(sources[0])
    oracle.propagate(packed, host, st, nslots, EVAL_NTPB, EVAL_MAX_BLOCKS, max_steps)
    t, q, _ = daq(host, 0, len(host), 1)
    hit = (t < 1e8).astype(np.uint32)
    nhit = int(hit.sum())
    acc = (np.zeros(nch, np.uint32), np.zeros(nch, np.uint32), np.full(max(1, nhit * EVAL_K), 1e9, np.float32))
    for src in sources:
        host = oracle._replicated(src, EVAL_NREPS)
        oracle.propagate(packed, host, st, nslots, EVAL_NTPB, EVAL_MAX_BLOCKS, max_steps, ncopies=EVAL_NREPS)
        for c in range(EVAL_NREPS):
            mc, _, _ = daq(host, c * len(src), len(src), ndaq)
            _accumulate(hit, t, mc, ndaq, EVAL_K, EVAL_TWIDTH, EVAL_TRANGE, *acc)
    return dict(hit=hit, t=t, q=q, hitcount=acc[0], bincount=acc[1], nearest=acc[2], rng=st, normal=normal)


@pytest.mark.parametrize('ndaq', [5, 1])
def test_eval_pdf_seeds_put_bin_counts_on_both_sides(small_detector, small_packed, ndaq):
    saved = small_detector.time_cdf, small_detector.charge_cdf
    small_detector.set_time_dist_gaussian(1.2, -6.0, 6.0)
    small_detector.set_charge_dist_gaussian(1.0, 0.1, 0.5, 1.5)
    try:
        got = oracle_eval_pdf(small_detector, small_packed, ndaq)
    finally:
        small_detector.time_cdf, small_detector.charge_cdf = saved
    assert got['hit'].all(), 'the observed event hits both channels'
    assert (got['hitcount'] > 0).all()
    if ndaq == 5:
        assert (got['bincount'] >= EVAL_K).any() and (got['bincount'] < EVAL_K).any(), got['bincount']
        assert (got['nearest'] < 1e8).any()


# ------------------------------------------------------------------ Likelihood over a stub simulation
class _Channels(object):
    def __init__(self, hit):
        self.hit = np.array(hit, dtype=bool)
        self.t = np.where(self.hit, 100.0, 1e9).astype(np.float32)
        self.q = self.hit.astype(np.float32)


class _Event(object):
    def __init__(self, hit):
        self.channels = _Channels(hit)


class _StubSim(object):
    """eval_pdf / eval_kernel return fixed arrays and record how they were called."""

    def __init__(self, hitcount, value):
        self.hitcount, self.value = np.array(hitcount, np.uint32), np.array(value, float)
        self.calls = []

    def eval_pdf(self, channels, iterable, min_twidth, trange, min_qwidth, qrange, **kw):
        self.calls.append(dict(kw, sources=list(iterable), min_twidth=min_twidth, trange=trange,
                               min_qwidth=min_qwidth, qrange=qrange, channels=channels))
        return self.hitcount.copy(), self.value.copy(), self.value.copy() * 0.1

    def setup_kernel(self, channels, iterable, trange, qrange, **kw):
        self.calls.append(dict(kw, setup=True, sources=list(iterable)))

    def eval_kernel(self, channels, iterable, trange, qrange, **kw):
        self.calls.append(dict(kw, sources=list(iterable)))
        scale = 1.0 + 0.5 * (len(self.calls) % 2)
        return self.hitcount.copy(), self.value.copy() * scale, np.zeros(len(self.value))


def test_likelihood_arithmetic():
    from chroma.likelihood import Likelihood
    nevals, nreps, ndaq = 2, 2, 5
    ntotal = nevals * nreps * ndaq
    assert ntotal == 20
    observed = [True, True, False, False, True, False]
    sim = _StubSim([20, 0, 0, 20, 5, 3], [0.5, 0.0, np.nan, 0.3, -1.0, 0.2])
    ev = _Event(observed)
    lik = Likelihood(sim, ev, trange=(-0.5, 999.5))
    assert lik.event is ev
    hit_prob, value, uncert = lik.eval_channel_vbin(iter(range(100)), nevals, nreps, ndaq)
    call = sim.calls[-1]
    assert call['sources'] == [0, 1] and call['min_twidth'] == 0.2 and call['min_qwidth'] == 1
    assert call['min_bin_content'] == 320 and call['nreps'] == nreps and call['ndaq'] == ndaq
    assert call['time_only'] is True and call['trange'] == (-0.5, 999.5) and call['channels'] is ev.channels
    assert np.allclose(hit_prob, np.array([20, 0, 0, 20, 5, 3]) / 20.0, rtol=1e-6, atol=0)
    flat = 1.0 / 1000.0
    # non-positive and NaN densities take the flat density over the range, the others stay
    assert np.allclose(value, [0.5, flat, flat, 0.3, flat, 0.2], rtol=1e-12, atol=0)
    assert np.allclose(uncert, [0.05, flat, flat, 0.03, flat, 0.02], rtol=1e-12, atol=0)
    nll = lik.eval(iter(range(100)), nevals, nreps, ndaq)
    assert isinstance(nll, float)
    # flipped where the event has no hit, floored at half a trial
    prob = np.array([1.0, 0.5 / ntotal, 1.0, 0.5 / ntotal, 0.25, 0.85])
    want = -(np.log(prob).sum() + np.log(0.5) + 2 * np.log(flat))
    assert abs(nll - want) < 1e-5 * abs(want)
    # time and charge: the flat density is over both ranges
    both = Likelihood(sim, ev, trange=(0.0, 10.0), qrange=(0.0, 4.0), time_only=False)
    assert both.flat_density() == 1.0 / 40.0
    _, value, _ = both.eval_channel_vbin(iter(range(100)), nevals, nreps, ndaq)
    assert value[1] == value[2] == value[4] == 1.0 / 40.0 and sim.calls[-1]['time_only'] is False
    # set_event replaces the event
    other = _Event([False] * 6)
    lik.set_event(other)
    assert lik.event is other
    nll = lik.eval(iter(range(100)), nevals, nreps, ndaq)
    prob = np.maximum(1.0 - np.array([20, 0, 0, 20, 5, 3]) / 20.0, 0.5 / ntotal)
    assert abs(nll + np.log(prob).sum()) < 1e-5


def test_likelihood_kernel_average():
    from chroma.likelihood import Likelihood
    sim = _StubSim([4, 4, 0], [0.5, 0.25, 0.0])
    lik = Likelihood(sim, _Event([True, True, False]), trange=(0.0, 100.0))
    lik.setup_kernel(iter(range(100)), 3, 2, 2, 4)
    call = sim.calls[-1]
    assert call['setup'] and call['sources'] == list(range(12)) and call['scale_factor'] == 4
    assert call['nreps'] == 2 and call['ndaq'] == 2
    mean, err = lik.eval_kernel(iter(range(100)), 3, nreps=2, ndaq=2, navg=4)
    assert len(sim.calls) == 5 and [c['sources'] for c in sim.calls[1:]] == [[0, 1, 2], [3, 4, 5], [6, 7, 8],
                                                                            [9, 10, 11]]
    # only the densities of the hit channels enter; the stub alternates between two scales
    logs = np.array([np.log(0.5 * s) + np.log(0.25 * s) for s in (1.0, 1.5, 1.0, 1.5)])
    assert abs(mean + logs.mean()) < 1e-12
    assert abs(err - logs.std() / 2.0) < 1e-12


# ------------------------------------------------------------------ not sharded
@pytest.mark.parametrize('method', ['eval_pdf', 'create_pdf', 'setup_kernel', 'eval_kernel'])
def test_sharded_simulation_refuses(method):
    from chroma.sim import ShardedSimulation
    with pytest.raises(NotImplementedError):
        getattr(ShardedSimulation, method)(object(), None, [])
