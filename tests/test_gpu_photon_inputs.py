"""Photons that are not fresh, and photons outside the tables' domain, on the
HIP path against the CPU oracle.

The other parity tests start from flags = 0, last_hit = -1, t = 0, weight = 1
and wavelengths in 300-600 nm.  Here the inputs are what a caller that resumes
photons after a max_steps cut feeds back: terminated photons that must draw
nothing, be written nowhere and never be queued (while still holding their
slot in the first step's chunks), live photons whose self-hit exclusion is
their incoming last_hit (the wire plane's -2 included), times and weights that
are no longer 0 and 1; then origins outside the world, wavelengths on and
beyond both ends of the property tables (60..995 nm), and photons that really
take the NaN-abort branch.  Every non-vacuity condition is asserted on the
oracle's arrays.  The contract is test_gpu_parity's: flags, last hits and RNG
slot states bit-exact, floats within 1e-5 relative, NaN equal to NaN.

Every test computes its oracle half first; gpu_side=False (not a fixture: a
plain default) runs that half alone, which is how the conditions were checked
on a machine without a GPU.
"""
import numpy as np
import pytest

import oracle
import scenes
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

NO_HIT, BULK_ABSORB, SURFACE_DETECT, SURFACE_ABSORB = 1 << 0, 1 << 1, 1 << 2, 1 << 3
RAYLEIGH_SCATTER, REFLECT_DIFFUSE, SURFACE_REEMIT, BULK_REEMIT = 1 << 4, 1 << 5, 1 << 7, 1 << 9
NAN_ABORT = 1 << 15      # the device's 16-bit history (chroma.event.NAN_ABORT_DEVICE)
DEAD_BITS = (NO_HIT, BULK_ABSORB, SURFACE_DETECT, SURFACE_ABSORB, NAN_ABORT)
DEAD = sum(DEAD_BITS)

SHAPES = [(64, 64), (256, 64)]     # per-step chunk launches at N >= 8192; one multi-step launch below 32768


@pytest.fixture(scope='module')
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from chroma.gpu import create_cuda_context
    return create_cuda_context()


_cache = {}


def _geometry(name):
    """(geometry, packed, GPUGeometry or None) of scenes.physics_scene() or
    chroma.demo.scint.tiny(), built once per module; the GPUGeometry is added
    by the first GPU test that asks."""
    if name not in _cache:
        from chroma import loader
        from chroma.demo import scint
        from chroma.gpu.packing import PackedGeometry
        geo = loader.create_geometry_from_obj(scenes.physics_scene() if name == 'scene' else scint.tiny())
        _cache[name] = [geo, PackedGeometry(geo), None]
    return _cache[name]


def _gpu_geometry(name):
    from chroma import gpu
    entry = _geometry(name)
    if entry[2] is None:
        entry[2] = gpu.GPUGeometry(entry[0])
    return entry[2]


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _snapshot(host):
    return {f: getattr(host, f).copy() for f in host.FIELDS}


def _unchanged(before, after, mask):
    """The photons of `mask` are the same words in all nine fields."""
    for f in oracle.HostPhotons.FIELDS:
        a, b = _bits(np.ascontiguousarray(before[f]))[mask], _bits(np.ascontiguousarray(getattr(after, f)))[mask]
        if not np.array_equal(a, b):
            return False
    return True


class _Both(object):
    """One batch on both sides: GPUPhotons uploaded with flags, last hits and
    weights (copy_* = True) and the same arrays on the host, one RNG each."""

    def __init__(self, name, photons, ntpb, max_blocks, seed, gpu_side=True):
        self.name, self.ntpb, self.max_blocks = name, ntpb, max_blocks
        self.nslots = ntpb * max_blocks
        self.packed = _geometry(name)[1]
        self.host = oracle.HostPhotons(photons)
        self.st = oracle.rng_init(self.nslots, seed=seed)
        self.gpu_side = gpu_side
        if gpu_side:
            from chroma import gpu
            self.gg = _gpu_geometry(name)
            self.gp = gpu.GPUPhotons(photons, copy_flags=True, copy_triangles=True, copy_weights=True)
            self.rng = gpu.get_rng_states(self.nslots, seed=seed)

    def leg_oracle(self, max_steps, use_weights=False):
        return oracle.propagate(self.packed, self.host, self.st, self.nslots, self.ntpb, self.max_blocks, max_steps,
                                use_weights=use_weights)

    def leg_gpu(self, max_steps, use_weights=False):
        if self.gpu_side:
            self.gp.propagate(self.gg, self.rng, nthreads_per_block=self.ntpb, max_blocks=self.max_blocks,
                              max_steps=max_steps, use_weights=use_weights)

    def compare(self, label):
        if self.gpu_side:
            _compare(self.host, self.gp, label)
            assert np.array_equal(self.rng.get().reshape(-1), self.st), label + ': RNG slot states differ'
            return self.gp.get()


def _gpu_unchanged(before, after, mask, label):
    if before is None:
        return
    for f in oracle.HostPhotons.FIELDS:
        assert np.array_equal(_bits(getattr(before, f))[mask], _bits(getattr(after, f))[mask]), \
            '%s: %s of a photon dead on entry was written' % (label, f)


# ------------------------------------------------------------------ resume
def _resume_leg1(ntpb, max_blocks, gpu_side=True):
    """photon_sources(12000, seed=61) run to max_steps = 3 on both sides and
    compared; the conditions of the second leg asserted on the oracle."""
    both = _Both('scene', scenes.photon_sources(12000, seed=61), ntpb, max_blocks, 61, gpu_side)
    both.leg_oracle(3)
    both.leg_gpu(3)
    got = both.compare('resume leg 1 %s' % ((ntpb, max_blocks),))
    h = both.host
    dead = (h.flags & DEAD) != 0
    assert dead.sum() >= 1000 and (~dead).sum() >= 1000, (int(dead.sum()), int((~dead).sum()))
    assert (h.last_hit_triangles[~dead] >= 0).any()
    assert (h.last_hit_triangles == -2).any()
    assert (h.t[~dead] != 0).all()
    return both, dead, got


def _after_leg2(both, dead, before_host, before_gpu, label):
    got = both.compare(label)
    assert _unchanged(before_host, both.host, dead), label + ': the oracle moved a photon dead on entry'
    assert not _unchanged(before_host, both.host, ~dead)
    _gpu_unchanged(before_gpu, got, dead, label)


@pytest.mark.parametrize('ntpb,max_blocks', SHAPES)
def test_resume_two_legs(cuda, ntpb, max_blocks, gpu_side=True):
    """The same GPUPhotons and RNG run on after a max_steps = 3 cut.  (64, 64):
    12000 >= 64*128 queued, so the second leg's first step is per-step chunk
    launches over a queue that is mostly dead photons; (256, 64): one
    multi-step launch per leg."""
    both, dead, got1 = _resume_leg1(ntpb, max_blocks, gpu_side)
    before = _snapshot(both.host)
    stats = both.leg_oracle(40)
    assert (stats['host_steps'] > 1) == (12000 >= ntpb * 128)
    both.leg_gpu(40)
    _after_leg2(both, dead, before, got1, 'resume leg 2 %s' % ((ntpb, max_blocks),))


@pytest.mark.parametrize('leg2_steps', [40, 1])
@pytest.mark.parametrize('ntpb,max_blocks', SHAPES)
def test_resume_batches_shared_photons(cuda, ntpb, max_blocks, leg2_steps, gpu_side=True):
    """The second leg through propagate_batches([gp, gp]): the same photons
    twice in one pipelined call, against two oracle calls.  After 40 steps the
    oracle leaves (next to) nobody alive, so the second pass is a queue of dead
    photons; leg2_steps = 1 keeps it busy as well."""
    both, dead, got1 = _resume_leg1(ntpb, max_blocks, gpu_side)
    before = _snapshot(both.host)
    both.leg_oracle(leg2_steps)
    alive_between = int(((both.host.flags & DEAD) == 0).sum())
    if leg2_steps == 1:
        assert alive_between >= 1000, alive_between
    both.leg_oracle(leg2_steps)
    if gpu_side:
        from chroma import gpu
        gpu.propagate_batches([both.gp, both.gp], both.gg, both.rng, nthreads_per_block=ntpb, max_blocks=max_blocks,
                              max_steps=leg2_steps)
    _after_leg2(both, dead, before, got1, 'resume batches %s' % ((ntpb, max_blocks, leg2_steps),))


@pytest.mark.parametrize('first_weighted', [True, False])
def test_resume_with_weights(cuda, first_weighted, gpu_side=True):
    """One leg with use_weights (absorption and detection folded into the
    weight), one without, in both orders: the second leg starts from weights
    below 1, or from a weighted leg's survivors."""
    both = _Both('scene', scenes.photon_sources(12000, seed=61), 64, 64, 61, gpu_side)
    both.leg_oracle(3, use_weights=first_weighted)
    both.leg_gpu(3, use_weights=first_weighted)
    got1 = both.compare('weights leg 1')
    h = both.host
    if first_weighted:
        assert (h.weights != 1).all(), int((h.weights == 1).sum())
    else:
        assert (h.weights == 1).all()
    dead = (h.flags & DEAD) != 0
    assert (~dead).sum() >= 1000 and dead.sum() >= 100, (int(dead.sum()), int((~dead).sum()))
    before = _snapshot(h)
    both.leg_oracle(40, use_weights=not first_weighted)
    both.leg_gpu(40, use_weights=not first_weighted)
    _after_leg2(both, dead, before, got1, 'weights leg 2 (first weighted: %s)' % first_weighted)
    w = both.host.weights[~dead]
    assert ((w > 0) & (w < 1)).any()


# --------------------------------------------------------- terminal inputs
def _terminal_photons():
    """9000 photons, two in three of them terminated on entry: every DEAD_MASK
    bit alone, all together, and each with non-terminal bits; dead and live
    ones share waves.  The dead ones carry times, weights and last hits that a
    write-back would disturb."""
    photons = scenes.photon_sources(9000, seed=65)
    extra = RAYLEIGH_SCATTER | REFLECT_DIFFUSE
    patterns = list(DEAD_BITS) + [DEAD] + [b | extra for b in DEAD_BITS] + [DEAD | extra]
    i = np.arange(9000)
    dead = i % 3 != 1
    flags = np.zeros(9000, np.uint32)
    flags[dead] = np.array(patterns, np.uint32)[np.arange(dead.sum()) % len(patterns)]
    flags[(i % 3 == 1) & (i % 2 == 0)] = extra      # live with a history
    photons.flags[:] = flags
    photons.t[dead] = -3.5 - (i[dead] % 7)
    photons.weights[dead] = 0.25
    photons.last_hit_triangles[dead] = np.where(i[dead] % 2 == 0, 5, -2)
    return photons, dead, patterns


@pytest.mark.parametrize('ntpb,max_blocks', SHAPES)
def test_terminal_inputs_are_left_alone(cuda, ntpb, max_blocks, gpu_side=True):
    photons, dead, patterns = _terminal_photons()
    assert set(np.unique(photons.flags[dead])) == set(patterns)
    both = _Both('scene', photons, ntpb, max_blocks, 65, gpu_side)
    before = _snapshot(both.host)
    stats = both.leg_oracle(30)
    assert (stats['host_steps'] > 1) == (9000 >= ntpb * 128)
    both.leg_gpu(30)
    got = both.compare('terminal inputs %s' % ((ntpb, max_blocks),))
    assert _unchanged(before, both.host, dead)
    live_done = ((both.host.flags[~dead] & DEAD) != 0).mean()
    assert live_done > 0.9, live_done
    if gpu_side:
        _gpu_unchanged(photons, got, dead, 'terminal inputs')
    if 9000 < ntpb * 128:      # one launch, slot = photon: the oracle spends no draw on a dead photon's slot
        cap = ntpb * max_blocks
        fresh = oracle.rng_init(cap, seed=65).reshape(6, cap)
        assert np.array_equal(both.st.reshape(6, cap)[:, :9000][:, dead], fresh[:, :9000][:, dead])


# ----------------------------------------------------------- volume source
def _volume_photons(n=12000, seed=63):
    from chroma.event import Photons
    r = np.random.RandomState(seed)
    pos = r.uniform(-2600.0, 2600.0, (n, 3)).astype(np.float32)
    d = r.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    p = np.cross(d, r.normal(size=(n, 3)))
    p /= np.linalg.norm(p, axis=1)[:, None]
    return Photons(pos, d.astype(np.float32), p.astype(np.float32), r.uniform(300.0, 600.0, n).astype(np.float32),
                   t=r.uniform(-50.0, 50.0, n).astype(np.float32))


@pytest.mark.parametrize('ntpb,max_blocks', SHAPES)
def test_volume_source(cuda, ntpb, max_blocks, gpu_side=True):
    """Origins uniform in a +-2600 mm cube around the +-2000 mm world, times
    uniform in +-50 ns: photons born outside (many miss everything, some enter
    through the black box from behind) and inside any solid."""
    photons = _volume_photons()
    both = _Both('scene', photons, ntpb, max_blocks, 63, gpu_side)
    both.leg_oracle(40)
    outside = (np.abs(photons.pos) > 2000.0).any(axis=1)
    hit = both.host.last_hit_triangles != -1
    assert outside.sum() >= 1000 and (outside & hit).sum() >= 100, (int(outside.sum()), int((outside & hit).sum()))
    assert ((both.host.flags & NO_HIT) != 0).sum() >= 1000
    assert (both.host.t < 0).any()
    both.leg_gpu(40)
    both.compare('volume source %s' % ((ntpb, max_blocks),))


# --------------------------------------------------- wavelength table edges
EDGE_WAVELENGTHS = (59.9, 60.0, 60.0001, 62.5, 65.0, 200.0, 300.0, 400.0, 402.5, 600.0, 990.0, 994.999, 995.0,
                    995.1, 2000.0)


def _edge_photons(name, n=12000):
    from chroma.photon_source import isotropic
    photons = scenes.photon_sources(n, seed=66) if name == 'scene' else isotropic(n, seed=66)
    photons.wavelengths[:] = np.array(EDGE_WAVELENGTHS, np.float32)[np.arange(n) % len(EDGE_WAVELENGTHS)]
    return photons


@pytest.mark.parametrize('name', ['scene', 'scint'])
def test_wavelength_table_edges(cuda, name, gpu_side=True):
    """Below, on, just inside and beyond both ends of standard_wavelengths
    (60..995 nm in 5-nm steps), and exact grid points.  At exactly 995 nm
    interp_property reads fp[n]: the packing's pad element."""
    photons = _edge_photons(name)
    start = photons.wavelengths.copy()
    both = _Both(name, photons, 128, 256, 66, gpu_side)
    both.leg_oracle(100)
    h = both.host
    for f in ('pos', 'dir', 'pol', 'wavelengths', 't', 'weights'):
        assert np.isfinite(getattr(h, f)).all(), f
    assert ((h.flags & NAN_ABORT) == 0).all()
    reemit = (h.flags & (SURFACE_REEMIT | BULK_REEMIT)) != 0
    for wl in (995.0, 60.0):
        assert reemit[start == np.float32(wl)].any(), 'no re-emission from %g nm' % wl
    for wl in EDGE_WAVELENGTHS:      # every listed wavelength is propagated, not just terminated at once
        assert (h.flags[start == np.float32(wl)] & ~np.uint32(DEAD)).any(), wl
    both.leg_gpu(100)
    both.compare('wavelength edges ' + name)


# ----------------------------------------------------------------- NaN abort
def _abort_photons():
    photons = scenes.photon_sources(6000, seed=64)
    photons.wavelengths[np.arange(6000) % 4 != 0] = 1e-3      # the thin-film surface then yields NaN state
    return photons


def test_photons_that_abort(cuda, gpu_side=True):
    """Three quarters of the wavelengths at 1e-3 nm: for the few of them that
    reach the thin-film surface at the right angle it yields a NaN direction,
    and the next step's NaN check sets NO_HIT | NAN_ABORT.
    test_abort_at_normal_incidence asserts that none aborts; here some do."""
    both = _Both('scene', _abort_photons(), 64, 64, 64, gpu_side)
    both.leg_oracle(40)
    aborted = (both.host.flags & NAN_ABORT) != 0
    assert aborted.sum() >= 1, 'no photon takes the NaN-abort branch'
    assert np.isnan(both.host.pos[aborted]).any() or np.isnan(both.host.dir[aborted]).any()
    both.leg_gpu(40)
    both.compare('NaN abort')
