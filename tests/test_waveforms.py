"""Photoelectron trains and digitised waveforms, as far as they can be checked
without a GPU: the numpy model (waveform_model.py) anchored on the oracle's DAQ,
the host twins chr_daq_pe_trains_host / chr_daq_digitise_host against the model
word for word, every refusal of the three new entry points (made before a
pointer is followed), WaveformSpec and the group budget."""
import ctypes

import numpy as np
import pytest

import waveform_model as wm
from library_model import fmaf, sat_u32
from test_daq_events import BOUNDS, SIZES

f32, u32 = np.float32, np.uint32
CHR_OK, CHR_ERR_INVALID = 0, 1
# power-of-two widths: inv = nsamples / width and every edge product are exact in float32.
# The first leaves the pmt1_early (negative), pmt0_late (4e8) and pmt0_never (inf) records
# outside; the second takes the early ones in.
WINDOWS = ((0.0, 64.0), (-128.0, 128.0))
NSAMPLES = (1, 63, 64, 65, 300)
PARAMS = ((64, 8, 1.0), (64, 1024, 0.5))


@pytest.fixture
def daq_detector(small_detector):
    saved = small_detector.time_cdf, small_detector.charge_cdf
    small_detector.set_time_dist_gaussian(1.2, -6.0, 6.0)
    small_detector.set_charge_dist_gaussian(1.0, 0.1, 0.5, 1.5)
    yield small_detector
    small_detector.time_cdf, small_detector.charge_cdf = saved


# ------------------------------------------------------------------ the model is a yardstick
@pytest.mark.parametrize('ntpb,max_blocks,weight', PARAMS)
def test_model_folds_to_the_oracle(daq_detector, ntpb, max_blocks, weight):
    """The model's records, folded per (event, channel), are oracle_events' three
    word arrays, and its draws leave the oracle's RNG states.  (Passes without the
    feature: it is what makes the model a yardstick.)"""
    case = wm.made_case(daq_detector, ntpb, max_blocks, weight)
    pe_c, pe_t, pe_q = case.pe
    assert len(pe_c) == BOUNDS[-1] - BOUNDS[0]
    t, q, fl = wm.fold(pe_c, pe_t, pe_q, case.photons.flags, BOUNDS, case.nchannels)
    assert np.array_equal(t, case.t), 'earliest time words'
    assert np.array_equal(q, case.q), 'charge words'
    assert np.array_equal(fl, case.fl), 'histories'
    assert np.array_equal(case.model_states, case.states), 'RNG states after the draws'
    # what the cases below rely on
    accepted = pe_c >= 0
    assert accepted.sum() > 300 and (~accepted).sum() > 300
    assert (pe_t[~accepted] == wm.NO_HIT_TIME).all() and (pe_q[~accepted] == 0).all()
    assert (pe_t[accepted] < 0).any() and np.isinf(pe_t[accepted]).any() and (pe_t[accepted] > 1e8).any()
    if ntpb * max_blocks < SIZES.max():
        # a slot carried its state across several photons of the 2000-photon event
        big = accepted[BOUNDS[6] - BOUNDS[0]:BOUNDS[7] - BOUNDS[0]]
        per_slot = np.bincount(np.flatnonzero(big) % (ntpb * max_blocks))
        assert per_slot.max() >= 2


# ------------------------------------------------------------------ host twins against the model
def _edited_records(case, trange):
    """The case's records with one NaN time, one exactly at t_lo and one exactly at the upper edge."""
    pe_c, pe_t, pe_q = (a.copy() for a in case.pe)
    # in the 2000-photon event, on channel 0 (hit there whatever the window)
    ev6 = np.arange(BOUNDS[6] - BOUNDS[0], BOUNDS[7] - BOUNDS[0])
    idx = ev6[(pe_c[ev6] == 0) & np.isfinite(pe_t[ev6]) & (pe_t[ev6] < 1e8)]
    assert len(idx) > 20
    special = dict(nan=int(idx[3]), lo=int(idx[5]), hi=int(idx[7]))
    pe_t[special['nan']] = np.nan
    pe_t[special['lo']] = trange[0]
    pe_t[special['hi']] = trange[1]
    return (pe_c, pe_t, pe_q), special


def _row_map(case, rows):
    """(the `rows` argument, the model's row_of_word, nrows) of a row mode"""
    words = case.t.size
    if rows == 'all':
        return 'all', None, words
    if rows == 'hit':
        m, n = wm.hit_map_of(case.t)
        assert 0 < n < words            # the empty event and the one-photon event leave words without a row
        return 'hit', m, n
    # a map of the caller's: every word its own row but word 12 (event 6, channel 0), which has none
    m = np.arange(words, dtype=np.int32)
    m[12] = -1
    m[13:] -= 1
    return m, m, words - 1


def _check_invariant(case, trains, outside, row_of_word, nrows):
    """sum_b trains[row][b] + outside_q[row] == q_int[row] (mod 2^32), on every row"""
    total = (trains.astype(np.uint64).sum(axis=1) + outside).astype(u32)
    q = case.q.reshape(-1)
    if row_of_word is None:
        assert np.array_equal(total, q)
        return
    words = np.flatnonzero(row_of_word >= 0)
    assert len(words) == nrows
    assert np.array_equal(total[row_of_word[words]], q[words])


@pytest.mark.parametrize('rows', ['all', 'hit', 'map'])
@pytest.mark.parametrize('nsamples', NSAMPLES)
def test_host_trains_equal_the_model(daq_detector, nsamples, rows):
    from chroma.gpu import HostWaveforms
    from chroma.gpu.hitmap import bin_scale
    case = wm.made_case(daq_detector, *PARAMS[0])
    arg, row_of_word, nrows = _row_map(case, rows)
    for trange in WINDOWS:
        (pe_c, pe_t, pe_q), special = _edited_records(case, trange)
        t_lo, inv = bin_scale(nsamples, trange)
        want, want_out, want_dropped = wm.trains(pe_c, pe_t, pe_q, BOUNDS, case.nchannels, row_of_word, nrows,
                                                 t_lo, inv, nsamples)
        hw = HostWaveforms(pe_c, pe_t, pe_q, BOUNDS, case.nchannels, trange, nsamples, rows=arg, time_int=case.t)
        assert hw.nrows == nrows and (hw.t_lo, hw.inv) == (t_lo, inv)
        got = hw.trains.reshape(nrows, nsamples)
        assert np.array_equal(got, want), 'train words'
        assert np.array_equal(hw.outside_q, want_out), 'outside words'
        assert hw.dropped == want_dropped
        # the photoelectrons of word 12 have no row in the caller's map; every hit word has one
        assert (hw.dropped > 0) == (rows == 'map')
        _check_invariant(case, got, hw.outside_q, row_of_word, nrows)
        assert want.any() and want_out.any()
        if rows == 'all':
            # the edges, by hand: t_lo is in bin 0 of its row, the upper edge and the NaN are outside
            row = 12
            assert want[row, 0] >= pe_q[special['lo']] > 0
            others = (pe_c == 0) & (wm.event_of(BOUNDS, len(pe_c)) == 6)
            others[[special['nan'], special['hi']]] = False
            alone = wm.trains(np.where(others, pe_c, -1), pe_t, pe_q, BOUNDS, case.nchannels, None, nrows, t_lo, inv,
                              nsamples)
            assert int(want_out[row]) - int(alone[1][row]) == int(pe_q[special['nan']]) + int(pe_q[special['hi']])
            # the records the first window leaves out: negative, 4e8 and infinite times
            if trange == WINDOWS[0]:
                kind = case.kind[BOUNDS[0]:BOUNDS[-1]]
                from test_gpu_daq import KINDS
                for name in ('pmt1_early', 'pmt0_late', 'pmt0_never'):
                    sel = (kind == KINDS.index(name)) & (pe_c >= 0)
                    assert sel.sum() > 10
                    x = (pe_t[sel] - t_lo) * inv
                    assert not ((x >= 0) & (x < nsamples)).any()
        # the event containers
        evs = hw.get()
        assert len(evs) == len(SIZES) and sum(len(w) for w in evs) == nrows
        assert all(w.adc is None and w.trains.shape == (len(w), nsamples) for w in evs)
        assert len(evs[5]) == (case.nchannels if rows != 'hit' else 0)          # the empty event
        assert np.array_equal(np.concatenate([w.trains for w in evs]), want)
        assert evs[0].t_lo == trange[0] and evs[0].dt == (trange[1] - trange[0]) / nsamples


def _template(ntaps, seed=3):
    r = np.random.RandomState(seed)
    return (np.exp(-np.arange(ntaps) / 3.0) * r.uniform(0.5, 1.0, ntaps)).astype(f32)


@pytest.mark.parametrize('ntaps', ['1', '5', 'nsamples+7'])
@pytest.mark.parametrize('nsamples', NSAMPLES)
def test_host_digitiser_equals_the_model(daq_detector, nsamples, ntaps):
    from chroma.gpu import HostWaveforms
    case = wm.made_case(daq_detector, *PARAMS[0])
    ntaps = nsamples + 7 if ntaps == 'nsamples+7' else int(ntaps)
    taps = _template(ntaps)
    hw = HostWaveforms(*case.pe, BOUNDS, case.nchannels, WINDOWS[0], nsamples, rows='all')
    trains = hw.trains.reshape(hw.nrows, nsamples).copy()
    empty = ~trains.any(axis=1)
    assert empty.any() and not empty.all()
    scale = f32(case.unit * f32(200.0))              # a photoelectron of charge 1 is 200 counts at the first tap
    for pedestal, bits in ((100.25, 12), (0.0, 16), (-50.0, 8)):
        adc_max = 2 ** bits - 1
        want, bad = wm.digitise(trains, taps, scale, pedestal, adc_max)
        hw.digitise(taps, scale, pedestal=pedestal, adc_bits=bits)
        got = hw.adc.reshape(hw.nrows, nsamples)
        assert got.dtype == np.uint16 and np.array_equal(got, want), 'ADC words'
        assert hw.bad == bad == 0
        assert got.max() <= adc_max
        # an all-zero row is the pedestal word
        word = min(int(sat_u32(f32(pedestal) + f32(0.5))[0]), adc_max)
        assert (got[empty] == word).all()
        assert (got[~empty] != word).any()
    evs = hw.get()
    assert np.array_equal(np.concatenate([w.adc for w in evs]), got)
    assert np.array_equal(hw.trains.reshape(hw.nrows, nsamples), trains), 'digitise changed the trains'


def _host_digitise(trains, taps, scale, pedestal, adc_max):
    """chr_daq_digitise_host on trains of the test's own making"""
    from chroma.gpu import _native
    trains = np.ascontiguousarray(trains, u32)
    taps = np.ascontiguousarray(taps, f32)
    adc = np.zeros(trains.shape, np.uint16)
    bad = np.full(1, 77, u32)
    _native.call('chr_daq_digitise_host', trains.ctypes.data, trains.shape[0], trains.shape[1], taps.ctypes.data,
                 len(taps), float(scale), float(pedestal), int(adc_max), adc.ctypes.data, bad.ctypes.data)
    return adc, int(bad[0])


def test_single_photoelectron_closed_form():
    """A row with one photoelectron is pedestal + scale * q * template, shifted by its bin."""
    nsamples, b, q = 64, 10, 43690
    taps = _template(5)
    scale, pedestal = f32(0.004), f32(100.25)
    trains = np.zeros((3, nsamples), u32)
    trains[1, b] = q
    trains[2, nsamples - 2] = q                  # the template runs off the end of the row
    adc, bad = _host_digitise(trains, taps, scale, pedestal, 4095)
    assert bad == 0
    flat = int(sat_u32(pedestal + f32(0.5))[0])
    pulse = sat_u32(fmaf(taps * f32(q), scale, pedestal) + f32(0.5)).astype(np.uint16)
    assert (pulse[:3] > flat + 10).all() and pulse.max() < 4095
    want = np.full((3, nsamples), flat, np.uint16)
    want[1, b:b + 5] = pulse
    want[2, nsamples - 2:] = pulse[:2]
    assert np.array_equal(adc, want)
    model, _ = wm.digitise(trains, taps, scale, pedestal, 4095)
    assert np.array_equal(model, want)


def test_saturation_negative_and_nan():
    nsamples = 65
    r = np.random.RandomState(11)
    trains = np.zeros((4, nsamples), u32)
    trains[0, r.randint(0, nsamples, 30)] = 43690
    trains[1, 5] = 0xFFFFFFFF                    # the largest charge word
    trains[3, 64] = 1
    taps = _template(5)
    # saturation at adc_max, and a negative scale clipped at 0
    for scale, pedestal in ((0.5, 10.0), (-0.5, 10.0)):
        adc, bad = _host_digitise(trains, taps, scale, pedestal, 4095)
        want, _ = wm.digitise(trains, taps, scale, pedestal, 4095)
        assert bad == 0 and np.array_equal(adc, want)
        assert (adc[0] == (4095 if scale > 0 else 0)).any() and (adc[2] == 10).all()
    # a NaN tap: every sample it reaches in a row that holds charge counts in `bad` and reads 0;
    # the all-zero row is the pedestal word all the same
    taps[2] = np.nan
    adc, bad = _host_digitise(trains, taps, 0.5, 10.0, 4095)
    want, want_bad = wm.digitise(trains, taps, 0.5, 10.0, 4095)
    assert np.array_equal(adc, want) and bad == want_bad == 3 * (nsamples - 2)
    assert (adc[0, 2:] == 0).all() and (adc[2] == 10).all()
    # a NaN pedestal: every sample of every row
    adc, bad = _host_digitise(trains, _template(5), 0.5, np.nan, 4095)
    assert bad == trains.size and not adc.any()
    # more taps than samples, one sample
    adc, bad = _host_digitise(trains[:, :1] + u32(7), _template(400), 1.0, 0.0, 65535)
    assert np.array_equal(adc, wm.digitise(trains[:, :1] + u32(7), _template(400), 1.0, 0.0, 65535)[0])


# ------------------------------------------------------------------ refusals, before any dereference
FAKE = 0x1000


def _pe_call(bounds=BOUNDS, nphotons=3000, nevents=None, rng_nslots=64 * 1024, ntpb=64, max_blocks=1024, null=(),
             cdf_len=51):
    """chr_daq_acquire_events_pe with made-up device addresses, as test_daq_events._call"""
    from chroma.gpu import _native
    from chroma.gpu.daq import _DetectorDesc
    arg = lambda name: None if name in null else FAKE      # noqa: E731
    ph = _native.PhotonsDesc(*[FAKE] * 9)
    if 'photon_t' in null:
        ph.d_t = None
    det = _DetectorDesc(arg('s2c'), arg('time_cdf_x'), FAKE, FAKE, FAKE, 2, cdf_len, 51, 1.5 / 2 ** 16)
    bounds = np.ascontiguousarray(bounds, np.int64)
    nevents = len(bounds) - 1 if nevents is None else nevents
    return _native.lib().chr_daq_acquire_events_pe(
        None if 'ph' in null else ctypes.byref(ph), nphotons, None if 'bounds' in null else bounds.ctypes.data,
        nevents, arg('rng'), rng_nslots, 0x4, arg('solid_map'), None if 'det' in null else ctypes.byref(det),
        arg('time_int'), arg('q_int'), arg('history'), arg('q'), arg('pe_channel'), arg('pe_time'), arg('pe_q'),
        ctypes.c_float(1.0), ntpb, max_blocks, None)


@pytest.mark.parametrize('null', ['ph', 'photon_t', 'bounds', 'rng', 'solid_map', 'det', 's2c', 'time_int', 'q_int',
                                  'history', 'q', 'pe_channel', 'pe_time', 'pe_q'])
def test_pe_refuses_null_arguments(null):
    from chroma.gpu import _native
    assert _pe_call(null=(null,)) == CHR_ERR_INVALID
    msg = _native.lib().chr_last_error()
    assert b'null' in msg and msg.startswith(b'chr_daq_acquire_events_pe:')


def test_pe_refusals_of_the_plain_call():
    from chroma.gpu import _native
    assert _pe_call([0]) == CHR_OK and _pe_call([7]) == CHR_OK            # no events: nothing touched
    assert _pe_call(null=('time_cdf_x',)) == CHR_ERR_INVALID
    assert _pe_call(cdf_len=1) == CHR_ERR_INVALID
    assert _pe_call([0, 10, 9, 20]) == CHR_ERR_INVALID
    assert b'decrease' in _native.lib().chr_last_error()
    assert _pe_call([-1, 10]) == CHR_ERR_INVALID
    assert _pe_call([0, 10, 3001]) == CHR_ERR_INVALID
    assert _pe_call(nevents=-1) == CHR_ERR_INVALID
    assert _pe_call(ntpb=0) == CHR_ERR_INVALID
    assert _pe_call(max_blocks=0) == CHR_ERR_INVALID
    assert _pe_call(rng_nslots=1999) == CHR_ERR_INVALID
    assert b'rng states' in _native.lib().chr_last_error()
    assert _pe_call(rng_nslots=511, ntpb=64, max_blocks=8) == CHR_ERR_INVALID


def _trains_call(name, null=(), bounds=BOUNDS, nevents=None, nchannels=2, nrows=None, t_lo=0.0, inv=1.0, nsamples=64,
                 use_map=True):
    from chroma.gpu import _native
    arg = lambda a: None if a in null else FAKE      # noqa: E731
    bounds = np.ascontiguousarray(bounds, np.int64)
    nevents = len(bounds) - 1 if nevents is None else nevents
    nrows = max(nevents, 0) * nchannels if nrows is None else nrows
    args = [arg('pe_channel'), arg('pe_time'), arg('pe_q'), None if 'bounds' in null else bounds.ctypes.data, nevents,
            nchannels, FAKE if use_map else None, nrows, ctypes.c_float(t_lo), ctypes.c_float(inv), nsamples,
            arg('trains'), arg('outside_q'), arg('dropped')]
    if not name.endswith('_host'):
        args.append(None)
    return getattr(_native.lib(), name)(*args)


@pytest.mark.parametrize('name', ['chr_daq_pe_trains', 'chr_daq_pe_trains_host'])
def test_trains_refusals(name):
    from chroma.gpu import _native
    err = lambda: _native.lib().chr_last_error()      # noqa: E731
    for null in ('pe_channel', 'pe_time', 'pe_q', 'bounds', 'trains', 'outside_q', 'dropped'):
        assert _trains_call(name, null=(null,)) == CHR_ERR_INVALID
        assert b'null' in err() and err().startswith(name.encode() + b':')
    assert _trains_call(name, nsamples=0) == CHR_ERR_INVALID
    assert b'no samples' in err()
    for t_lo, inv in ((np.inf, 1.0), (-np.inf, 1.0), (np.nan, 1.0), (0.0, np.inf), (0.0, np.nan), (0.0, 0.0),
                      (0.0, -1.0)):
        assert _trains_call(name, t_lo=t_lo, inv=inv) == CHR_ERR_INVALID
        assert b'finite' in err()
    # more than 2^31 train words; exactly 2^31 passes this check (and is refused for its row count below)
    assert _trains_call(name, nrows=2 ** 23 + 1, nsamples=256) == CHR_ERR_INVALID
    assert b'train words' in err()
    assert _trains_call(name, nrows=2 ** 23, nsamples=256, use_map=False) == CHR_ERR_INVALID
    assert b'without a map' in err()
    assert _trains_call(name, nrows=5, use_map=False) == CHR_ERR_INVALID
    assert _trains_call(name, nevents=-1) == CHR_ERR_INVALID
    assert _trains_call(name, nchannels=0) == CHR_ERR_INVALID
    assert _trains_call(name, bounds=[0, 10, 9, 20]) == CHR_ERR_INVALID
    assert b'decrease' in err()
    assert _trains_call(name, bounds=[-1, 10]) == CHR_ERR_INVALID
    assert _trains_call(name, bounds=[0, 2 ** 31]) == CHR_ERR_INVALID
    assert _trains_call(name, bounds=np.arange(3), nchannels=2 ** 30 + 1, nrows=1) == CHR_ERR_INVALID
    assert b'channels exceed' in err()


def _digitise_call(name, null=(), nrows=16, nsamples=64, ntaps=5, adc_max=4095):
    from chroma.gpu import _native
    arg = lambda a: None if a in null else FAKE      # noqa: E731
    args = [arg('trains'), nrows, nsamples, arg('template'), ntaps, ctypes.c_float(1.0), ctypes.c_float(0.0), adc_max,
            arg('adc'), arg('bad')]
    if not name.endswith('_host'):
        args.append(None)
    return getattr(_native.lib(), name)(*args)


@pytest.mark.parametrize('name', ['chr_daq_digitise', 'chr_daq_digitise_host'])
def test_digitise_refusals(name):
    from chroma.gpu import _native
    err = lambda: _native.lib().chr_last_error()      # noqa: E731
    for null in ('trains', 'template', 'adc', 'bad'):
        assert _digitise_call(name, null=(null,)) == CHR_ERR_INVALID
        assert b'null' in err() and err().startswith(name.encode() + b':')
    assert _digitise_call(name, nsamples=0) == CHR_ERR_INVALID
    assert _digitise_call(name, ntaps=0) == CHR_ERR_INVALID
    assert _digitise_call(name, nrows=2 ** 23 + 1, nsamples=256) == CHR_ERR_INVALID
    assert b'train words' in err()
    assert _digitise_call(name, adc_max=65536) == CHR_ERR_INVALID
    assert b'65535' in err()
    # a row and the taps it can reach must fit the LDS words: 8192 + 8192 do, one more sample does not
    assert _digitise_call(name, nrows=1, nsamples=8193, ntaps=2 ** 31) == CHR_ERR_INVALID
    assert b'LDS' in err()
    assert _digitise_call(name, nrows=1, nsamples=16380, ntaps=5) == CHR_ERR_INVALID


def test_entry_points_are_exported():
    from chroma.gpu import _native
    lib = ctypes.CDLL(_native.library_path())
    for name in ('chr_daq_acquire_events_pe', 'chr_daq_pe_trains', 'chr_daq_pe_trains_host', 'chr_daq_digitise',
                 'chr_daq_digitise_host'):
        assert name in _native.EXPORTED and hasattr(lib, name)


# ------------------------------------------------------------------ the Python layer
def test_host_waveforms_arguments(daq_detector):
    from chroma.gpu import HostWaveforms
    case = wm.made_case(daq_detector, *PARAMS[0])
    with pytest.raises(ValueError):
        HostWaveforms(*case.pe, BOUNDS, 2, (0.0, 64.0), 64, rows='hit')              # no time words
    with pytest.raises(ValueError):
        HostWaveforms(*case.pe, BOUNDS, 2, (0.0, 64.0), 64, rows='some')
    with pytest.raises(ValueError):
        HostWaveforms(*case.pe, BOUNDS, 2, (0.0, 64.0), 0)
    with pytest.raises(ValueError):
        HostWaveforms(*case.pe, BOUNDS, 2, (5.0, 5.0), 64)                           # no positive finite scale
    with pytest.raises(ValueError):
        HostWaveforms(case.pe[0][:-1], case.pe[1], case.pe[2], BOUNDS, 2, (0.0, 64.0), 64)
    with pytest.raises(ValueError):
        HostWaveforms(*case.pe, BOUNDS, 2, (0.0, 64.0), 64, rows=np.array([0, 2] + [-1] * 14, np.int32))   # row 1
    hw = HostWaveforms(*case.pe, BOUNDS, 2, (0.0, 64.0), 64)
    for bits in (0, 17):
        with pytest.raises(ValueError):
            hw.digitise([1.0], 1.0, adc_bits=bits)
    with pytest.raises(ValueError):
        hw.digitise([], 1.0)
    # no events at all
    none = HostWaveforms([], [], [], [7], 2, (0.0, 64.0), 64, rows='all')
    assert none.nrows == 0 and none.get() == [] and none.digitise([1.0], 1.0).bad == 0


def test_waveform_spec_and_group_budget():
    from chroma import event
    from chroma.sim import ShardedSimulation, Simulation, WaveformSpec, daq_event_groups, waveform_event_groups
    spec = WaveformSpec((0.0, 64.0), 256)
    assert (spec.rows, spec.template, spec.scale, spec.pedestal, spec.adc_bits, spec.keep_photoelectrons) == \
        ('hit', None, 1.0, 0.0, 12, False)
    assert WaveformSpec((0.0, 64.0), 256, template=[1, 0.5]).template.dtype == np.float32
    for bad in (dict(nsamples=0), dict(trange=(1.0, 1.0)), dict(trange=(2.0, 1.0)), dict(trange=(0.0, np.inf)),
                dict(trange=None), dict(rows='some'), dict(adc_bits=0), dict(adc_bits=17), dict(template=[]),
                dict(template=np.ones((2, 2))), dict(nsamples=16000, template=np.ones(400))):
        kw = dict(trange=(0.0, 64.0), nsamples=256)
        kw.update(bad)
        with pytest.raises(ValueError):
            WaveformSpec(**kw)
    ev = event.Event()
    assert ev.photoelectrons is None and ev.waveforms is None

    # rows='all': every train word counts; uniform events group as daq_event_groups with 16 + 4*nsamples per channel
    nch = 29007
    spec = WaveformSpec((0.0, 64.0), 256, rows='all')
    assert spec.event_bytes(10, nch) == spec.event_bytes(10 ** 6, nch) == (16 + 4 * 256) * nch
    budget = Simulation.daq_group_bytes
    per = budget // ((16 + 4 * 256) * nch)
    assert per == 2
    groups = waveform_event_groups(np.arange(1001), nch, budget, spec)
    assert groups[0] == (0, per) and all(b - a == per for a, b in groups) and groups[-1] == (998, 1000)
    # rows='hit': an upper bound from the photon count -- a row per photon, at most one per channel
    spec = WaveformSpec((0.0, 64.0), 256, rows='hit')
    assert spec.event_bytes(0, nch) == 16 * nch
    assert spec.event_bytes(100, nch) == 16 * nch + 4 * 256 * 100
    assert spec.event_bytes(10 ** 6, nch) == (16 + 4 * 256) * nch
    one_photon = waveform_event_groups(np.arange(1001), nch, budget, spec)
    assert one_photon[0] == (0, budget // (16 * nch + 1024))
    # every event once and in order, groups of at least one, whatever the budget
    for budget in (1, 16 * 2 * 3, 5000, 64 << 20):
        for rows in ('hit', 'all'):
            spec = WaveformSpec((0.0, 64.0), 64, rows=rows)
            groups = waveform_event_groups(BOUNDS, 2, budget, spec)
            assert [e for a, b in groups for e in range(a, b)] == list(range(len(SIZES)))
            for a, b in groups:
                held = sum(spec.event_bytes(n, 2) for n in SIZES[a:b])
                assert b - a == 1 or held <= budget
                if b < len(SIZES):      # the next event did not fit
                    assert held + spec.event_bytes(SIZES[b], 2) > budget
    assert waveform_event_groups([0], 2, 64 << 20, spec) == []
    # without train words (events without photons, rows='hit') the groups are daq_event_groups'
    spec = WaveformSpec((0.0, 64.0), 64, rows='hit')
    assert spec.event_bytes(0, 2) * 3 == 16 * 2 * 3 and daq_event_groups(np.zeros(8), 2, 96) == \
        waveform_event_groups(np.zeros(8), 2, 96, spec)

    with pytest.raises(NotImplementedError, match='waveforms are not sharded: use Simulation'):
        ShardedSimulation._check_waveforms(None)
