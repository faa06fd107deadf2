"""chr_generate_photons on the device against its host twin (bit for bit), the
generated photons through propagate against the oracle, and through
Simulation.simulate.  tests/test_gensteps.py checks the host twin's physics."""
import numpy as np
import pytest

import oracle

import genstep_scene
from chroma import gensteps as gs

pytestmark = pytest.mark.gpu

FIELDS = ('pos', 'dir', 'pol', 'wavelengths', 't', 'weights', 'flags', 'last_hit_triangles', 'evidx')


@pytest.fixture(scope='module')
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from chroma.gpu import create_cuda_context
    return create_cuda_context()


@pytest.fixture(scope='module')
def scene(cuda):
    from chroma import gpu
    geo, packed, m = genstep_scene.build()
    return gpu.GPUGeometry(geo), packed, m


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _fill(gp, value):
    """Every word of the nine arrays set to `value` (to see what a call leaves alone)."""
    import torch
    for f in FIELDS:
        getattr(gp, f).tensor.view(torch.int32).fill_(value)


def test_rng_init_host_matches_device(cuda):
    from chroma import gpu
    for nslots, seed, offset, first in ((1000, 1, 0, 0), (257, 2 ** 40 + 12345, 17, 0), (64, 3, 0, 4096)):
        dev = gpu.get_rng_states(nslots, seed=seed, offset=offset, first_subsequence=first)
        assert np.array_equal(dev.get().reshape(-1), gs.rng_init_host(nslots, seed, offset, first))


def test_host_twin_parity(scene):
    """128 slots, steps of 0 / 1 / 63 / 64 / 65 / 1000 / 0 / 777 / 300 photons: every slot
    draws ~18 photons and waves straddle step boundaries; written from photon 5 of a
    larger buffer."""
    from chroma import gpu
    from chroma.gpu.photon import _alloc
    gg, packed, m = scene
    steps = genstep_scene.mixed_steps(m)
    n, first, cap, nslots = len(steps), 5, len(steps) + 5 + 11, 128
    host_st = gs.rng_init_host(nslots, seed=5)
    host, host_exhausted = gs.generate_photons_host(steps, packed, host_st, first_photon=first, capacity=cap)

    rng = gpu.get_rng_states(nslots, seed=5)
    buf = type('H', (), _alloc(cap))()
    _fill(buf, 0x5a5a5a5a)
    made = gpu.generate_photons(steps, gg, rng, out=buf, first_photon=first)
    assert len(made) == n and made.exhausted == host_exhausted == 0
    got = gpu.GPUPhotonsSlice(*[getattr(buf, f) for f in ('pos', 'dir', 'pol', 'wavelengths', 't',
                                                          'last_hit_triangles', 'flags', 'weights', 'evidx')]).get()
    w = slice(first, first + n)
    for f in FIELDS:
        a, b = _bits(getattr(got, f)), _bits(getattr(host, f))
        assert np.array_equal(a[w], b[w]), '%s differs from the host twin at %s' % (
            f, np.flatnonzero((a[w] != b[w]).reshape(n, -1).any(axis=1))[:5])
        assert np.all(a[:first] == 0x5a5a5a5a) and np.all(a[first + n:] == 0x5a5a5a5a), f + ': wrote outside its range'
    assert np.array_equal(rng.get().reshape(-1), host_st), 'RNG slot states differ after generation'
    assert np.array_equal(_bits(made.get().dir), _bits(host.dir[w]))


def test_exhaustion_parity(scene):
    """The rejection loop's bounded exit, on the device as on the host."""
    from chroma import gpu
    gg, packed, m = scene
    steps = gs.cherenkov_step(m['disp'], 2000, x0=(0, 0, 0), dx=(1, 2, 3), beta=1.0 / 1.3599,
                              wavelength_range=(300.0, 600.0))
    host_st = gs.rng_init_host(256, seed=19)
    host, host_exhausted = gs.generate_photons_host(steps, packed, host_st)
    rng = gpu.get_rng_states(256, seed=19)
    made = gpu.generate_photons(steps, gg, rng)
    assert made.exhausted == host_exhausted > 0
    got = made.get()
    for f in ('dir', 'pol', 'wavelengths'):
        assert np.array_equal(_bits(getattr(got, f)), _bits(getattr(host, f))), f
    assert np.array_equal(rng.get().reshape(-1), host_st)


def test_device_validation(scene):
    from chroma import gpu
    from chroma.gpu._native import NativeError
    gg, packed, m = scene
    rng = gpu.get_rng_states(64, seed=1)
    before = rng.get().copy()
    for bad in (gs.cherenkov_step(m['disp'], 10, x0=(0, 0, 0), dx=(0, 0, 1), beta=0.7),
                gs.isotropic_flash(99, 10), gs.scintillation_step(m['water'], 10, x0=(0, 0, 0))):
        with pytest.raises(NativeError):
            gpu.generate_photons(bad, gg, rng)
    small = gpu.GPUPhotons(gpu.generate_photons(gs.isotropic_flash(m['water'], 4), gg, gpu.get_rng_states(64, seed=2)))
    with pytest.raises(NativeError):
        gpu.generate_photons(gs.isotropic_flash(m['water'], 4), gg, rng, out=small, first_photon=1)
    assert np.array_equal(rng.get(), before)


@pytest.fixture(scope='module')
def physics(cuda):
    import scenes
    from chroma import gpu, loader
    from chroma.gpu.packing import PackedGeometry
    geo = loader.create_geometry_from_obj(scenes.physics_scene())
    packed = PackedGeometry(geo)
    by_name = {x.name: x for x in packed.material_objects}
    steps = gs.Gensteps.join([
        gs.cherenkov_step(by_name['water'], 4000, x0=(0, 0, 0), dx=(30, 10, -20), beta=0.95, dt=0.1,
                          wavelength_range=(300.0, 600.0)),
        gs.scintillation_step(by_name['scint'], 3000, x0=(100, -50, -900), dx=(5, 5, 20), component=0),
        gs.scintillation_step(by_name['scint'], 1001, x0=(-200, 100, -850), dx=(0, 0, 0), component=1, t0=3.0),
        gs.isotropic_flash(by_name['water'], 4000, x0=(500, 300, -200), wavelength_range=(300.0, 600.0))])
    return geo, packed, steps


def test_generate_then_propagate_matches_oracle(physics):
    """GPU generate + propagate == the oracle's propagate of the host twin's photons,
    started from the host twin's final RNG states, photon for photon."""
    from chroma import gpu
    from test_gpu_parity import _compare
    geo, packed, steps = physics
    ntpb, blocks, max_steps = 64, 64, 60
    nslots = ntpb * blocks
    rng = gpu.get_rng_states(nslots, seed=3)
    gg = gpu.GPUGeometry(geo)
    made = gpu.generate_photons(steps, gg, rng)
    assert made.exhausted == 0
    made.propagate(gg, rng, nthreads_per_block=ntpb, max_blocks=blocks, max_steps=max_steps)

    st = gs.rng_init_host(nslots, seed=3)
    twin, _ = gs.generate_photons_host(steps, packed, st)
    host = oracle.HostPhotons(twin)
    oracle.propagate(packed, host, st, nslots, ntpb, blocks, max_steps)
    _compare(host, made, 'gensteps')
    assert np.array_equal(rng.get().reshape(-1), st)
    fl = host.flags
    assert ((fl & (1 << 10)) != 0).sum() == 4000 and ((fl & (1 << 11)) != 0).sum() == 4001   # the origin bits survive
    assert ((fl & (1 << 2)) != 0).any() and ((fl & (1 << 9)) != 0).any()


def test_through_simulation(physics):
    """Simulation.simulate([gensteps]) == generate_photons on fresh same-seed states,
    propagate, get_flat_hits; keep_photons_beg returns the generated photons."""
    from chroma import gpu
    from chroma.sim import Simulation
    geo, packed, steps = physics
    sim = Simulation(geo, seed=7, nthreads_per_block=64, max_blocks=256)
    out = list(sim.simulate([steps], keep_photons_beg=True, max_steps=100))
    assert len(out) == 1 and out[0].nphotons == len(steps) and sim.last_exhausted == 0

    rng = gpu.get_rng_states(64 * 256, seed=7)
    made = gpu.generate_photons(steps, sim.gpu_geometry, rng)
    beg = made.get()
    made.propagate(sim.gpu_geometry, rng, nthreads_per_block=64, max_blocks=256, max_steps=100)
    want = made.get_flat_hits(sim.gpu_geometry)
    got = out[0].flat_hits
    assert len(want) > 0 and len(got) == len(want)
    for f in FIELDS + ('channel',):
        assert np.array_equal(_bits(getattr(got, f)), _bits(getattr(want, f))), f
    kept = out[0].photons_beg.get()
    for f in FIELDS:
        assert np.array_equal(_bits(getattr(kept, f)), _bits(getattr(beg, f))), f
    # a Gensteps alone, and two events of them, are accepted too
    two = list(sim.simulate([steps, steps], max_steps=10))
    assert [ev.nphotons for ev in two] == [len(steps)] * 2
    one = list(sim.simulate(steps, max_steps=10))
    assert len(one) == 1
