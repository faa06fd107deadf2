"""The DAQ of all events of a batch in one call (chr_daq_acquire_events,
GPUDaq.acquire_events, Simulation.daq_events), as far as it can be checked
without a GPU: the entry point's refusals (all made before a device is
touched), the grouping arithmetic, and -- on the oracle alone -- that the
events tests/test_gpu_daq_events.py feeds the kernel exercise what it can get
wrong: an RNG slot's state carried from event to event, and a slot's stride
over several photons of one event."""
import ctypes

import numpy as np
import pytest

import oracle

# event sizes 37, 1, 63, 64, 65, 0, 2000, 755: the first event does not start at
# photon 0, the last stops short of the 3000 made records
BOUNDS = np.array([5, 42, 43, 106, 170, 235, 235, 2235, 2990], np.int64)
SIZES = np.diff(BOUNDS)
CHR_OK, CHR_ERR_INVALID = 0, 1


# ------------------------------------------------------------------ entry point
def _call(bounds, nphotons=3000, nevents=None, rng_nslots=64 * 1024, ntpb=64, max_blocks=1024, null=(),
          cdf_len=51):
    """chr_daq_acquire_events with made-up device addresses: every refusal comes
    before the first dereference or launch, so none of them is ever used."""
    from chroma.gpu import _native
    from chroma.gpu.daq import _DetectorDesc
    fake = 0x1000
    arg = lambda name: None if name in null else fake      # noqa: E731
    ph = _native.PhotonsDesc(*[fake] * 9)
    if 'photon_t' in null:
        ph.d_t = None
    det = _DetectorDesc(arg('s2c'), arg('time_cdf_x'), fake, fake, fake, 2, cdf_len, 51, 1.5 / 2 ** 16)
    bounds = np.ascontiguousarray(bounds, np.int64)
    nevents = len(bounds) - 1 if nevents is None else nevents
    return _native.lib().chr_daq_acquire_events(
        None if 'ph' in null else ctypes.byref(ph), nphotons, None if 'bounds' in null else bounds.ctypes.data,
        nevents, arg('rng'), rng_nslots, 0x4, arg('solid_map'), None if 'det' in null else ctypes.byref(det),
        arg('time_int'), arg('q_int'), arg('history'), arg('q'), ctypes.c_float(1.0), ntpb, max_blocks, None)


def test_entry_point_is_exported():
    from chroma.gpu import _native
    assert 'chr_daq_acquire_events' in _native.EXPORTED
    assert hasattr(ctypes.CDLL(_native.library_path()), 'chr_daq_acquire_events')


def test_no_events_is_ok():
    assert _call([0]) == CHR_OK
    assert _call([7]) == CHR_OK


@pytest.mark.parametrize('null', ['ph', 'photon_t', 'bounds', 'rng', 'solid_map', 'det', 's2c', 'time_int', 'q_int',
                                  'history', 'q'])
def test_refuses_null_arguments(null):
    from chroma.gpu import _native
    assert _call(BOUNDS, null=(null,)) == CHR_ERR_INVALID
    assert b'null' in _native.lib().chr_last_error()


def test_refuses_missing_cdfs():
    assert _call(BOUNDS, null=('time_cdf_x',)) == CHR_ERR_INVALID
    assert _call(BOUNDS, cdf_len=1) == CHR_ERR_INVALID


def test_refuses_bad_bounds():
    from chroma.gpu import _native
    assert _call([0, 10, 9, 20]) == CHR_ERR_INVALID                 # decreasing
    assert b'decrease' in _native.lib().chr_last_error()
    assert _call([-1, 10]) == CHR_ERR_INVALID                       # below the first photon
    assert _call([0, 10, 3001]) == CHR_ERR_INVALID                  # beyond the photon count
    assert _call([0, 3001, 3000]) == CHR_ERR_INVALID                # beyond it in the middle
    assert _call(BOUNDS, nevents=-1) == CHR_ERR_INVALID
    assert _call(BOUNDS, ntpb=0) == CHR_ERR_INVALID
    assert _call(BOUNDS, max_blocks=0) == CHR_ERR_INVALID


def test_refuses_too_few_rng_slots():
    from chroma.gpu import _native
    # the largest event has 2000 photons: min(cap, 2000) slots draw
    assert _call(BOUNDS, rng_nslots=1999) == CHR_ERR_INVALID
    assert b'rng states' in _native.lib().chr_last_error()
    assert _call(BOUNDS, rng_nslots=511, ntpb=64, max_blocks=8) == CHR_ERR_INVALID      # cap 512


# ------------------------------------------------------------------ grouping
def test_group_arithmetic():
    from chroma.sim import Simulation, daq_event_groups
    assert Simulation.daq_group_bytes // (16 * 29007) >= 1
    groups = daq_event_groups(np.arange(1001), 29007, 64 << 20)
    assert groups[0] == (0, 144) and all(b - a == 144 for a, b in groups[:-1])
    assert groups[-1] == (864, 1000)
    # a budget below one event's rows still gives groups of one
    assert daq_event_groups(BOUNDS, 29007, 1000) == [(e, e + 1) for e in range(len(SIZES))]
    # every event once, in order
    for budget, per in ((16 * 2 * 3, 3), (16 * 2 * 3 + 31, 3), (64 << 20, len(SIZES))):
        groups = daq_event_groups(BOUNDS, 2, budget)
        assert [e for a, b in groups for e in range(a, b)] == list(range(len(SIZES)))
        assert all(0 < b - a <= per for a, b in groups) and groups[0][1] == min(per, len(SIZES))
    assert daq_event_groups([0], 2, 64 << 20) == []


# ------------------------------------------------------------------ the GPU test's inputs, on the oracle
def oracle_events(detector, host, st, nslots, bounds, ntpb, max_blocks, weight=1.0):
    """oracle.daq(raw=True) per event [bounds[e], bounds[e+1]), in order, on the
    one state array `st`: rows of (time words, charge words, histories), each
    (nevents, nchannels), and the state after every event."""
    from chroma.gpu.detector import cdf_arrays
    nch = int(detector.num_channels())
    unit = np.float32(detector.charge_cdf[0][-1] / 2 ** 16)
    rows, states = [], []
    for start, end in zip(bounds[:-1], bounds[1:]):
        rows.append(oracle.daq(host, detector.solid_id, detector.solid_id_to_channel_index,
                               cdf_arrays(detector.time_cdf), cdf_arrays(detector.charge_cdf), unit, st, nslots,
                               start=int(start), n=int(end - start), ndaq=1, nchannels=nch, global_weight=weight,
                               nthreads_per_block=ntpb, max_blocks=max_blocks, raw=True))
        states.append(st.copy())
    t, q, fl = (np.array([r[k] for r in rows]) for k in range(3))
    return t, q, fl, states


def test_made_events_exercise_carried_state_and_stride(small_detector):
    from test_gpu_daq import _made_records, N_MADE
    saved = small_detector.time_cdf, small_detector.charge_cdf
    small_detector.set_time_dist_gaussian(1.2, -6.0, 6.0)
    small_detector.set_charge_dist_gaussian(1.0, 0.1, 0.5, 1.5)
    try:
        photons, kind = _made_records(small_detector)
        assert BOUNDS[-1] < N_MADE and BOUNDS[0] > 0
        host = oracle.HostPhotons(photons)
        nslots, cap = 64 * 1024, 64 * 8
        st = oracle.rng_init(nslots, seed=5)
        fresh = st.copy()
        t, q, fl, states = oracle_events(small_detector, host, st, nslots, BOUNDS, 64, 8)
        maxbits = np.float32(1e9).view(np.uint32)
        changed = np.zeros(nslots, np.int64)       # events in which a slot's state changed
        before = fresh
        for e, n in enumerate(SIZES):
            moved = (states[e].reshape(6, nslots) != before.reshape(6, nslots)).any(axis=0)
            changed += moved
            assert not moved[min(cap, n):].any()            # only slots below min(cap, n_e) take part
            if n >= 63:
                assert (q[e] > 0).any() and (t[e] < maxbits).any() and (fl[e] != 0).any()
            if n == 0:
                assert not moved.any()
                assert (t[e] == maxbits).all() and (q[e] == 0).all() and (fl[e] == 0).all()
            before = states[e]
        assert (SIZES == 0).any() and (SIZES >= 63).sum() >= 4
        # the state carried across events: a slot that drew in two or more events
        assert (changed >= 2).any()
        # the stride within an event: a slot with two drawing photons (positions s, s + cap, ...) of one event
        strided = False
        for start, end in zip(BOUNDS[:-1], BOUNDS[1:]):
            idx, _ = oracle.hits(host, small_detector.solid_id, small_detector.solid_id_to_channel_index,
                                 start=int(start), n=int(end - start))
            per_slot = np.bincount((idx - start) % cap, minlength=cap)
            strided |= bool(((idx - start) >= cap).any() and (per_slot >= 2).any())
        assert strided
    finally:
        small_detector.time_cdf, small_detector.charge_cdf = saved
