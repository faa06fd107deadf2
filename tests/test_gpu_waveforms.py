"""Photoelectron records, charge trains and digitised waveforms on the device
(chr_daq_acquire_events_pe, chr_daq_pe_trains, chr_daq_digitise through
GPUDaq.acquire_photoelectrons, GPUPhotoelectrons.trains, GPUWaveforms.digitise
and Simulation.simulate(waveforms=...)) against acquire_events, the CPU oracle,
the host twins and the numpy model of waveform_model.py: word for word."""
import numpy as np
import pytest

import waveform_model as wm
from test_daq_events import BOUNDS, SIZES
from test_waveforms import WINDOWS, PARAMS, _edited_records, _row_map, _check_invariant, _template

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32


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
    shape = (chans.nevents, chans.nchannels)
    return (chans.time_int.get().reshape(shape), chans.q_int.get().reshape(shape), chans.flags.get().reshape(shape),
            chans.q.get().view(u32).reshape(shape))


def _photon_words(gp):
    got = gp.get()
    return [np.asarray(getattr(got, f)).copy() for f in ('t', 'flags', 'last_hit_triangles', 'weights', 'pos')]


@pytest.mark.parametrize('ntpb,max_blocks,weight', PARAMS)
def test_photoelectrons(cuda, daq_detector, ntpb, max_blocks, weight):
    from chroma import gpu
    case = wm.made_case(daq_detector, ntpb, max_blocks, weight)
    gdet = gpu.GPUDetector(daq_detector)
    gp = gpu.GPUPhotons(case.photons, copy_flags=True, copy_triangles=True, copy_weights=True)
    before = _photon_words(gp)
    kw = dict(nthreads_per_block=ntpb, max_blocks=max_blocks, weight=weight)

    rng = gpu.get_rng_states(case.nslots, seed=case.seed)
    chans, pe = gpu.GPUDaq(gdet).acquire_photoelectrons(gp, rng, BOUNDS, **kw)
    got = _rows(chans)
    assert len(chans) == len(pe) == len(SIZES)

    # against acquire_events from fresh states of the same seed: rows, converted charges, RNG states
    rng2 = gpu.get_rng_states(case.nslots, seed=case.seed)
    plain = _rows(gpu.GPUDaq(gdet).acquire_events(gp, rng2, BOUNDS, **kw))
    for a, b, name in zip(got, plain, ('time words', 'charge words', 'histories', 'converted charges')):
        assert np.array_equal(a, b), name + ' differ from acquire_events'
    assert np.array_equal(rng.get(), rng2.get()), 'RNG slot states differ from acquire_events'

    # against the oracle
    assert np.array_equal(got[0], case.t) and np.array_equal(got[1], case.q) and np.array_equal(got[2], case.fl)
    assert np.array_equal(got[3], (case.q.astype(f32) * f32(gdet.charge_unit)).view(u32))
    assert np.array_equal(rng.get().reshape(-1), case.states), 'RNG slot states differ from the oracle'
    for a, b in zip(before, _photon_words(gp)):
        assert np.array_equal(a.view(u32), b.view(u32)), 'the DAQ changed the photons'

    # the records, on every position of the span
    pe_c, pe_t, pe_q = case.pe
    assert len(pe.channel) == len(pe_c) == BOUNDS[-1] - BOUNDS[0]
    assert np.array_equal(pe.channel.get(), pe_c), 'photoelectron channels'
    assert np.array_equal(pe.t.get().view(u32), pe_t.view(u32)), 'photoelectron times'
    assert np.array_equal(pe.q_int.get(), pe_q), 'photoelectron charge words'
    assert np.array_equal(pe.time_int.get().reshape(case.t.shape), case.t)

    # the containers: the accepted photons of every event, in photon order
    evs = pe.get()
    assert len(evs) == len(SIZES)
    for e, (a, b) in enumerate(zip(BOUNDS[:-1] - BOUNDS[0], BOUNDS[1:] - BOUNDS[0])):
        keep = pe_c[a:b] >= 0
        assert np.array_equal(evs[e].channel, pe_c[a:b][keep]) and np.array_equal(evs[e].q_int, pe_q[a:b][keep])
        assert np.array_equal(evs[e].t.view(u32), pe_t[a:b][keep].view(u32))
        assert np.array_equal(evs[e].q.view(u32), (pe_q[a:b][keep].astype(f32) * f32(gdet.charge_unit)).view(u32))
    assert len(evs[5]) == 0 and sum(len(x) for x in evs) == (pe_c >= 0).sum()


def _device_records(case, records):
    from chroma import gpu
    from chroma.gpu import gpuarray as ga
    return gpu.GPUPhotoelectrons(ga.to_gpu(records[0]), ga.to_gpu(records[1]), ga.to_gpu(records[2]), BOUNDS,
                                 case.nchannels, case.unit, ga.to_gpu(case.t.reshape(-1).copy()))


@pytest.mark.parametrize('rows', ['all', 'hit', 'map'])
@pytest.mark.parametrize('nsamples', [1, 64, 65, 300])
def test_trains_and_adc(cuda, daq_detector, nsamples, rows):
    """The device's trains, outside_q, dropped and adc against the host twin and the
    model, with the NaN, t_lo and upper-edge records of the CPU test."""
    from chroma.gpu import HostWaveforms
    case = wm.made_case(daq_detector, *PARAMS[0])
    arg, row_of_word, nrows = _row_map(case, rows)
    scale = f32(case.unit * f32(200.0))
    for trange in WINDOWS:
        records, _ = _edited_records(case, trange)
        wf = _device_records(case, records).trains(trange, nsamples, rows=arg)
        hw = HostWaveforms(*records, BOUNDS, case.nchannels, trange, nsamples, rows=arg, time_int=case.t)
        want, want_out, want_dropped = wm.trains(*records, BOUNDS, case.nchannels, row_of_word, nrows, wf.t_lo,
                                                 wf.inv, nsamples)
        assert wf.nrows == hw.nrows == nrows and (wf.t_lo, wf.inv) == (hw.t_lo, hw.inv)
        assert np.array_equal(wf.event, hw.event) and np.array_equal(wf.channel, hw.channel)
        got = wf.trains.get().reshape(nrows, nsamples)
        assert np.array_equal(got, want), 'train words differ from the model'
        assert np.array_equal(got, hw.trains.reshape(nrows, nsamples)), 'train words differ from the host twin'
        assert np.array_equal(wf.outside_q.get(), want_out) and np.array_equal(hw.outside_q, want_out)
        assert wf.dropped == hw.dropped == want_dropped and (want_dropped > 0) == (rows == 'map')
        _check_invariant(case, got, wf.outside_q.get(), row_of_word, nrows)
        for ntaps in (1, 5, 400):
            taps = _template(ntaps)
            want_adc, want_bad = wm.digitise(want, taps, scale, 100.25, 4095)
            wf.digitise(taps, scale, pedestal=100.25, adc_bits=12)
            hw.digitise(taps, scale, pedestal=100.25, adc_bits=12)
            adc = wf.adc.get().reshape(nrows, nsamples)
            assert adc.dtype == np.uint16 and np.array_equal(adc, want_adc), 'ADC words differ from the model'
            assert np.array_equal(adc, hw.adc.reshape(nrows, nsamples)), 'ADC words differ from the host twin'
            assert wf.bad == hw.bad == want_bad == 0
        # a NaN tap counts in `bad`, an all-zero row keeps the pedestal word
        taps = _template(5)
        taps[1] = np.nan
        want_adc, want_bad = wm.digitise(want, taps, scale, 100.25, 4095)
        wf.digitise(taps, scale, pedestal=100.25)
        assert np.array_equal(wf.adc.get().reshape(nrows, nsamples), want_adc)
        assert wf.bad == want_bad and (want_bad > 0) == (nsamples > 1)
        assert np.array_equal(wf.trains.get().reshape(nrows, nsamples), want), 'digitise changed the trains'
        evs = wf.get()
        assert len(evs) == len(SIZES) and np.array_equal(np.concatenate([w.adc for w in evs]), want_adc)
        assert np.array_equal(np.concatenate([w.channels for w in evs]), hw.channel)


def _check_event_waveforms(ev, spec, nchannels, unit):
    """ev.waveforms against the direct calls on the event's own photoelectrons
    (the host twins, which the tests above hold to the device word for word)."""
    from chroma.gpu import HostWaveforms
    pe, w = ev.photoelectrons, ev.waveforms
    n = len(pe)
    hw = HostWaveforms(pe.channel, pe.t, pe.q_int, [0, n], nchannels, spec.trange, spec.nsamples, rows=spec.rows,
                       time_int=ev.channels.t.view(u32))
    hw.digitise(spec.template, spec.scale, spec.pedestal, spec.adc_bits)
    direct = hw.get()[0]
    assert np.array_equal(w.channels, direct.channels)
    assert np.array_equal(w.trains, direct.trains) and np.array_equal(w.outside_q, direct.outside_q)
    assert w.adc.dtype == np.uint16 and np.array_equal(w.adc, direct.adc)
    assert (w.t_lo, w.dt) == (direct.t_lo, direct.dt)
    if spec.rows == 'hit':
        assert np.array_equal(w.channels, np.flatnonzero(ev.channels.t.view(u32) != wm.NO_HIT_BITS))
    else:
        assert np.array_equal(w.channels, np.arange(nchannels))
    # the rows' charge is the channels' charge
    total = (w.trains.astype(np.uint64).sum(axis=1) + w.outside_q).astype(u32)
    assert np.array_equal((total.astype(f32) * f32(unit)).view(u32), ev.channels.q[w.channels].view(u32))
    return int(w.trains.any(axis=1).sum())


def test_simulation(cuda, daq_detector):
    """Simulation.simulate(run_daq=True, waveforms=spec): the channels and the
    final rng_states of the run without the spec, and the waveforms of the direct
    calls, also under a budget that forces groups of three events."""
    from chroma.gpu import _native
    from chroma.photon_source import isotropic
    from chroma.sim import Simulation, WaveformSpec
    r = np.random.RandomState(3)
    sizes = r.randint(2, 1500, 14)
    sizes[[3, 8]] = 0
    sizes[5] = 1
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    source = isotropic(int(cuts[-1]), seed=77)
    taps = _template(5)
    hit = WaveformSpec((0.0, 64.0), 65, template=taps, scale=0.004, pedestal=20.5, rows='hit',
                       keep_photoelectrons=True)
    every = WaveformSpec((-8.0, 56.0), 64, template=taps, scale=0.004, pedestal=20.5, adc_bits=10, rows='all',
                         keep_photoelectrons=True)
    runs = []
    for spec, budget in ((None, None), (hit, None), (every, 3 * every.event_bytes(1000, 2) + 5)):
        sim = Simulation(daq_detector, seed=23, nthreads_per_block=64, max_blocks=256)
        if budget is not None:
            sim.daq_group_bytes = budget
        calls = []

        def hook(name, fn):
            if name.startswith('chr_daq'):
                calls.append(name)
            return fn()

        saved, _native.call_hook = _native.call_hook, hook
        try:
            evs = list(sim.simulate((source[a:b] for a, b in zip(cuts[:-1], cuts[1:])), run_daq=True,
                                    photons_per_batch=4000, max_steps=100, waveforms=spec))
        finally:
            _native.call_hook = saved
        assert len(evs) == len(sizes) and sim.last_pipeline[0] >= 2, 'several batches'
        runs.append((evs, sim.rng_states.get(), calls, sim.gpu_daq.charge_unit))
    plain, plain_rng = runs[0][0], runs[0][1]
    assert all(ev.waveforms is None and ev.photoelectrons is None for ev in plain)
    for (evs, rng, calls, unit), spec in zip(runs[1:], (hit, every)):
        assert np.array_equal(rng, plain_rng), 'final rng_states differ from the run without waveforms'
        charged = 0
        for e, (a, b) in enumerate(zip(plain, evs)):
            assert np.array_equal(a.channels.hit, b.channels.hit), e
            assert np.array_equal(a.channels.t.view(u32), b.channels.t.view(u32)), e
            assert np.array_equal(a.channels.q.view(u32), b.channels.q.view(u32)), e
            assert np.array_equal(a.channels.flags, b.channels.flags), e
            charged += _check_event_waveforms(b, spec, 2, unit)
            if sizes[e] == 0:
                assert len(b.photoelectrons) == 0 and not b.waveforms.trains.any()
        assert charged > 8
        assert set(calls) == {'chr_daq_acquire_events_pe', 'chr_daq_pe_trains', 'chr_daq_digitise'}
    # groups of three: more calls than batches
    batches = runs[1][2].count('chr_daq_acquire_events_pe')        # the default budget: a call per batch
    assert runs[2][2].count('chr_daq_acquire_events_pe') > batches
    assert runs[2][2].count('chr_daq_acquire_events_pe') >= -(-len(sizes) // 3)
    with pytest.raises(ValueError):
        Simulation.simulate(sim, [], run_daq=False, waveforms=hit)
    with pytest.raises(TypeError):
        sim.simulate([], run_daq=True, waveforms=dict(nsamples=64))
