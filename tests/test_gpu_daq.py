"""HIP DAQ (csrc/daq.hip through the C ABI) against the CPU oracle, bit for
bit, and the reference's own DAQ test (test/test_detector.py) through
Simulation(run_daq=True)."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from chroma.gpu import create_cuda_context
    return create_cuda_context()


@pytest.mark.parametrize('ndaq,ntpb,max_blocks,charge', [
    (1, 64, 8, (1.0, 0.1, 0.5, 1.5)), (1, 256, 1024, (1.0, 0.1, 0.5, 1.5)), (5, 64, 16, (1.0, 0.1, 0.5, 1.5)),
    # a pedestal-like charge CDF with negative support: negative charges convert
    # to 0 (CUDA's saturating float -> u32; a plain cast is undefined)
    (1, 64, 8, (0.1, 0.5, -2.0, 2.0)), (5, 64, 16, (0.1, 0.5, -2.0, 2.0))])
def test_daq_parity(cuda, small_detector, small_packed, ndaq, ntpb, max_blocks, charge):
    from chroma import gpu
    from chroma.gpu.detector import cdf_arrays
    from chroma.photon_source import isotropic
    from test_gpu_parity import _run_both, _compare
    saved = small_detector.time_cdf, small_detector.charge_cdf
    small_detector.set_time_dist_gaussian(1.2, -6.0, 6.0)
    small_detector.set_charge_dist_gaussian(*charge)
    try:
        photons = isotropic(20000, seed=31)
        nslots = 64 * 1024
        gp, host, rng, st, _ = _run_both(small_detector, small_packed, photons, nslots, 64, 1024, 100, seed=5)
        _compare(host, gp, 'propagate before DAQ')
        gdet = gpu.GPUDetector(small_detector)
        daq = gpu.GPUDaq(gdet, ndaq=ndaq)
        normal = np.zeros(2 * nslots, np.uint32)
        for start, n in ((0, 7000), (7000, 13000)):     # two "events"
            daq.begin_acquire()
            daq.acquire(gp, rng, nthreads_per_block=ntpb, max_blocks=max_blocks, start_photon=start, nphotons=n)
            ch = daq.end_acquire().get()
            t, q, fl = oracle.daq(host, small_detector.solid_id, small_detector.solid_id_to_channel_index,
                                  cdf_arrays(small_detector.time_cdf), cdf_arrays(small_detector.charge_cdf),
                                  gdet.charge_unit, st, nslots, normal_cache=normal, start=start, n=n, ndaq=ndaq,
                                  nchannels=gdet.nchannels, nthreads_per_block=ntpb, max_blocks=max_blocks)
            assert ch.hit.sum() > 0
            assert np.array_equal(ch.t.view(np.uint32), t.view(np.uint32)), 'earliest times differ'
            assert np.array_equal(ch.q.view(np.uint32), q.view(np.uint32)), 'charges differ'
            assert np.array_equal(ch.flags, fl), 'channel histories differ'
            assert np.array_equal(rng.get().reshape(-1), st), 'RNG slot states differ after DAQ'
            if ndaq > 1:
                assert np.array_equal(rng.normal_cache.get(), normal)
    finally:
        small_detector.time_cdf, small_detector.charge_cdf = saved


def _box_sim():
    from chroma.detector import Detector
    from chroma.geometry import Solid, vacuum
    from chroma.loader import create_geometry_from_obj
    from chroma.make import box
    from chroma.demo.optics import r7081hqe_photocathode
    from chroma.sim import Simulation
    cube = Detector(vacuum)
    cube.add_pmt(Solid(box(10.0, 10, 10), vacuum, vacuum, surface=r7081hqe_photocathode))
    cube.set_time_dist_gaussian(1.2, -6.0, 6.0)
    cube.set_charge_dist_gaussian(1.0, 0.1, 0.5, 1.5)
    geo = create_geometry_from_obj(cube, update_bvh_cache=False)
    return Simulation(geo, seed=17)


def _one_photon(t0):
    from chroma.event import Photons
    pos = np.zeros((1, 3), np.float32)
    dir = np.tile([0, 0, 1], (1, 1)).astype(np.float32)
    phi = np.random.uniform(0, 2 * np.pi, 1).astype(np.float32)
    pol = np.zeros_like(pos)
    pol[:, 0], pol[:, 1] = np.cos(phi), np.sin(phi)
    return Photons(pos=pos, dir=dir, pol=pol, t=np.full(1, t0, np.float32), wavelengths=np.full(1, 400.0, np.float32))


def test_detector_time_and_charge(cuda):
    """test/test_detector.py testTime / testCharge, unmodified in substance."""
    sim = _box_sim()
    hit_times = [ev.channels.t[0] for ev in sim.simulate((_one_photon(100.0) for _ in range(1000)), run_daq=True)
                 if ev.channels.hit[0]]
    assert len(hit_times) > 100
    assert abs(np.std(hit_times) - 1.2) < 0.1
    hit_q = [ev.channels.q[0] for ev in sim.simulate((_one_photon(0.0) for _ in range(1000)), run_daq=True)
             if ev.channels.hit[0]]
    assert abs(np.mean(hit_q) - 1.0) < 0.1
    assert abs(np.std(hit_q) - 0.1) < 0.1


# ------------------------------------------------------------------ made records
# The tests above feed the DAQ what propagation on the 2-PMT detector leaves.
# Below the photon records are written by hand (no propagation), so the DAQ
# kernels see last hits of -1 and -2, a solid without a channel, the detect bit
# clear, weights of 0 and in (0, 1), negative and infinite times, and ndaq
# larger than the workgroup.
SURFACE_DETECT, SURFACE_ABSORB, REFLECT_DIFFUSE, RAYLEIGH_SCATTER = 1 << 2, 1 << 3, 1 << 5, 1 << 4
N_MADE = 3000
KINDS = ('pmt0', 'pmt1_light', 'pmt0_weightless', 'pmt1_early', 'no_hit', 'wire', 'no_channel', 'not_detected',
         'pmt0_late', 'pmt1', 'pmt0_never')


def _made_records(detector, n=N_MADE, seed=71):
    """n photon records cycling through KINDS; only t, flags, last hits and
    weights matter to the DAQ.  Returns (Photons, kind index per record)."""
    from chroma.event import Photons
    r = np.random.RandomState(seed)
    solid = np.asarray(detector.solid_id)
    s2c = np.asarray(detector.solid_id_to_channel_index)
    tri = {c: np.flatnonzero(s2c[solid] == c) for c in (-1, 0, 1)}
    assert all(len(v) > 0 for v in tri.values())
    kind = np.arange(n) % len(KINDS)
    k = {name: kind == i for i, name in enumerate(KINDS)}
    last = np.empty(n, np.int32)
    for names, c in ((('pmt0', 'pmt0_weightless', 'pmt0_late', 'pmt0_never', 'not_detected'), 0),
                     (('pmt1_light', 'pmt1_early', 'pmt1'), 1), (('no_channel',), -1)):
        for name in names:
            last[k[name]] = r.choice(tri[c], int(k[name].sum()))
    last[k['no_hit']] = -1
    last[k['wire']] = -2
    assert last.max() < len(solid)
    flags = np.full(n, SURFACE_DETECT, np.uint32)
    flags |= np.where(r.uniform(size=n) < 0.3, REFLECT_DIFFUSE, 0).astype(np.uint32)
    flags |= np.where(r.uniform(size=n) < 0.3, RAYLEIGH_SCATTER, 0).astype(np.uint32)
    flags[k['not_detected']] = SURFACE_ABSORB | REFLECT_DIFFUSE
    t = r.uniform(5.0, 60.0, n).astype(np.float32)
    t[k['pmt1_early']] = r.uniform(-80.0, -1.0, int(k['pmt1_early'].sum())).astype(np.float32)
    t[k['pmt0_late']] = 4e8
    t[k['pmt0_never']] = np.inf
    w = np.ones(n, np.float32)
    w[k['pmt1_light']] = r.uniform(0.05, 0.95, int(k['pmt1_light'].sum())).astype(np.float32)
    w[k['pmt0_weightless']] = 0.0
    pos = np.zeros((n, 3), np.float32)
    dir = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    pol = np.tile(np.array([1, 0, 0], np.float32), (n, 1))
    return Photons(pos, dir, pol, np.full(n, 400.0, np.float32), t=t, last_hit_triangles=last, flags=flags,
                   weights=w), kind


# (start, n): starts that are no multiple of 64; 1, 63, 65 and 0 photons; the whole batch
RANGES = ((0, N_MADE), (37, 1), (101, 63), (165, 65), (300, 0), (231, 2000))


@pytest.mark.parametrize('ndaq,ntpb,max_blocks,weight', [
    (1, 64, 8, 1.0),          # cap = 512 below most ranges: a slot takes several photons
    (1, 64, 1024, 0.5),       # cap above every range, global weight 0.5
    (64, 64, 16, 1.0),        # run_daq_many: exactly one pass of its inner loop
    (65, 64, 16, 1.0),        # one work-item takes a second pass
    (150, 64, 16, 0.5)])      # three passes, the last ragged
def test_daq_made_records(cuda, small_detector, ndaq, ntpb, max_blocks, weight):
    from chroma import gpu
    from chroma.gpu.detector import cdf_arrays
    saved = small_detector.time_cdf, small_detector.charge_cdf
    small_detector.set_time_dist_gaussian(1.2, -6.0, 6.0)
    small_detector.set_charge_dist_gaussian(1.0, 0.1, 0.5, 1.5)
    try:
        photons, kind = _made_records(small_detector)
        host = oracle.HostPhotons(photons)
        nslots = 64 * 1024
        gdet = gpu.GPUDetector(small_detector)
        gp = gpu.GPUPhotons(photons, copy_flags=True, copy_triangles=True, copy_weights=True)
        rng = gpu.get_rng_states(nslots, seed=5)
        st = oracle.rng_init(nslots, seed=5)
        daq = gpu.GPUDaq(gdet, ndaq=ndaq)
        normal = np.zeros(2 * nslots, np.uint32)
        for start, n in RANGES:
            before = st.copy()
            daq.begin_acquire()
            daq.acquire(gp, rng, nthreads_per_block=ntpb, max_blocks=max_blocks, start_photon=start, nphotons=n,
                        weight=weight)
            label = 'range %s' % ((start, n),)
            t, q, fl = oracle.daq(host, small_detector.solid_id, small_detector.solid_id_to_channel_index,
                                  cdf_arrays(small_detector.time_cdf), cdf_arrays(small_detector.charge_cdf),
                                  gdet.charge_unit, st, nslots, normal_cache=normal, start=start, n=n, ndaq=ndaq,
                                  nchannels=gdet.nchannels, global_weight=weight, nthreads_per_block=ntpb,
                                  max_blocks=max_blocks, raw=True)
            # the accumulator words before end_acquire: time bits, quantised charge, history
            assert np.array_equal(daq.earliest_time_int_gpu.get(), t), label + ': earliest time words differ'
            assert np.array_equal(daq.channel_q_int_gpu.get(), q), label + ': charge words differ'
            assert np.array_equal(daq.channel_history_gpu.get(), fl), label + ': channel histories differ'
            assert np.array_equal(rng.get().reshape(-1), st), label + ': RNG slot states differ'
            if ndaq > 1:
                assert np.array_equal(rng.normal_cache.get(), normal), label + ': normal cache differs'
            ch = daq.end_acquire().get()
            assert np.array_equal(ch.t.view(np.uint32), t)
            expect_q = np.zeros(len(q), np.float32)
            expect_q[:gdet.nchannels] = q[:gdet.nchannels].astype(np.float32) * np.float32(gdet.charge_unit)
            assert np.array_equal(ch.q.view(np.uint32), expect_q.view(np.uint32))
            # on the oracle: what this range must show
            kinds = set(kind[start:start + n])
            if n == 0:
                assert np.array_equal(st, before) and (q == 0).all() and (fl == 0).all()
            if n >= 63:
                assert not np.array_equal(st, before)
                assert len(kinds) == len(KINDS)
                # an early (negative) time never wins the unsigned minimum against a positive one
                maxbits = np.float32(1e9).view(np.uint32)
                tt = t.view(np.float32)
                assert ((t < maxbits) & (tt > 0)).any() and (q > 0).any()
                assert not (fl & SURFACE_ABSORB).any()
    finally:
        small_detector.time_cdf, small_detector.charge_cdf = saved


def test_daq_weightless_records_draw_but_add_nothing(cuda, small_detector):
    """weight = 0: the acceptance draw is taken (the RNG advances as the oracle
    says) and nothing is recorded; acquire(weight=0) does the same to all."""
    from chroma import gpu
    from chroma.gpu.detector import cdf_arrays
    saved = small_detector.time_cdf, small_detector.charge_cdf
    small_detector.set_time_dist_gaussian(1.2, -6.0, 6.0)
    small_detector.set_charge_dist_gaussian(1.0, 0.1, 0.5, 1.5)
    try:
        photons, kind = _made_records(small_detector)
        photons.weights[:] = 0.0
        host = oracle.HostPhotons(photons)
        nslots = 64 * 64
        gdet = gpu.GPUDetector(small_detector)
        gp = gpu.GPUPhotons(photons, copy_flags=True, copy_triangles=True, copy_weights=True)
        for ndaq in (1, 65):
            rng = gpu.get_rng_states(nslots, seed=6)
            st = oracle.rng_init(nslots, seed=6)
            fresh = st.copy()
            daq = gpu.GPUDaq(gdet, ndaq=ndaq)
            normal = np.zeros(2 * nslots, np.uint32)
            daq.begin_acquire()
            daq.acquire(gp, rng, nthreads_per_block=64, max_blocks=64)
            t, q, fl = oracle.daq(host, small_detector.solid_id, small_detector.solid_id_to_channel_index,
                                  cdf_arrays(small_detector.time_cdf), cdf_arrays(small_detector.charge_cdf),
                                  gdet.charge_unit, st, nslots, normal_cache=normal, ndaq=ndaq,
                                  nchannels=gdet.nchannels, nthreads_per_block=64, max_blocks=64, raw=True)
            assert (q == 0).all() and (fl == 0).all() and (t == np.float32(1e9).view(np.uint32)).all()
            assert not np.array_equal(st, fresh), 'the oracle drew nothing'
            assert np.array_equal(daq.channel_q_int_gpu.get(), q)
            assert np.array_equal(daq.channel_history_gpu.get(), fl)
            assert np.array_equal(daq.earliest_time_int_gpu.get(), t)
            assert np.array_equal(rng.get().reshape(-1), st)
    finally:
        small_detector.time_cdf, small_detector.charge_cdf = saved


def test_channel_hit_counts(cuda, small_detector):
    """chr_channel_hit_counts (the per-rank array a sharded run sums) against
    a bincount of the oracle's hit selection over the same records."""
    import ctypes
    from chroma import gpu
    from chroma.gpu import _native, gpuarray as ga
    from chroma.gpu.tools import current_stream
    photons, kind = _made_records(small_detector)
    host = oracle.HostPhotons(photons)
    gdet = gpu.GPUDetector(small_detector)
    gp = gpu.GPUPhotons(photons, copy_flags=True, copy_triangles=True, copy_weights=True)
    nch = int(gdet.nchannels)
    assert nch == 2

    def counts(start, n, nchannels, fill=0):
        out = ga.to_gpu(np.full(nch, fill, np.uint32))
        _native.call('chr_channel_hit_counts', ctypes.byref(gp._desc()), start, n, SURFACE_DETECT,
                     gdet.solid_id_map.gpudata, gdet.solid_id_to_channel_index_gpu.gpudata, out.gpudata, nchannels,
                     current_stream())
        return out.get()      # the call is asynchronous: the download synchronises

    def expected(start, n):
        idx, ch = oracle.hits(host, small_detector.solid_id, small_detector.solid_id_to_channel_index, start=start,
                              n=n)
        return np.bincount(ch, minlength=nch).astype(np.uint32)

    for start, n in RANGES:
        want = expected(start, n)
        assert np.array_equal(counts(start, n, nch), want), (start, n)
        if n >= 63:
            assert (want > 0).all() and want.sum() < n
    whole = expected(0, N_MADE)
    assert np.array_equal(counts(0, N_MADE, nch, fill=7), whole + 7)          # counts accumulate
    assert np.array_equal(counts(300, 0, nch, fill=7), np.full(nch, 7, np.uint32))   # nphotons = 0: untouched
    assert np.array_equal(counts(0, N_MADE, 1), np.array([whole[0], 0], np.uint32))  # c < nchannels guard
