"""Photons from gensteps, through the host twin (chr_generate_photons_host: the
device kernel's per-photon source, csrc/genstep.h, built by the host compiler;
tests/test_gpu_gensteps.py pins the device to it bit for bit).  No GPU.

Bounds.  Unit vectors and orthogonality, 1e-5: about a dozen separately rounded
float32 operations (6e-8 each, chr_sincosf within 2 ulp) with a tenfold margin;
a wrong formula misses by 1e-3 or more.  The Cherenkov angle, 1e-5: n(wl) and
1/(beta n) are three float32 operations on the device, compared with float64.
Distributions: the reference's own threshold, KS p > 1e-3 (test/test_rayleigh.py),
at fixed seeds, 200k photons each.
"""
import numpy as np
import pytest
from scipy import stats

import oracle

import genstep_scene
from chroma import gensteps as gs
from chroma.gpu._native import NativeError

NSLOTS = 128
KS_N = 200000
KS_P = 1e-3


@pytest.fixture(scope='module')
def scene():
    geo, packed, m = genstep_scene.build()
    return packed, m


def _generate(packed, steps, seed=1, nslots=NSLOTS, **kw):
    st = gs.rng_init_host(nslots, seed=seed)
    photons, exhausted = gs.generate_photons_host(steps, packed, st, **kw)
    return photons, exhausted, st


@pytest.fixture(scope='module')
def mixed(scene):
    packed, m = scene
    steps = genstep_scene.mixed_steps(m)
    photons, exhausted, st = _generate(packed, steps, seed=5)
    return steps, photons, exhausted


def _table(packed, material, name):
    """The material's float32 table on the packed wavelength grid (without the pad)."""
    i = [k for k, x in enumerate(packed.material_objects) if x is material][0]
    return np.asarray(packed.materials[i][name])


def _n_of(packed, material, wl):
    return np.interp(np.asarray(wl, np.float64), packed.wavelengths.astype(np.float64),
                     _table(packed, material, 'refractive_index')[:-1].astype(np.float64))


def test_record_is_64_bytes():
    assert gs.GENSTEP_DTYPE.itemsize == 64
    assert [gs.GENSTEP_DTYPE.fields[f][1] for f in ('kind', 'x0', 'dx', 'wl_lo', 'component')] == [0, 16, 32, 48, 60]


def test_count_order_and_fields(scene, mixed):
    packed, m = scene
    steps, p, exhausted = mixed
    counts = np.array(genstep_scene.MIXED_COUNTS)
    assert len(steps) == counts.sum() == len(p) == gs.count(steps)
    assert exhausted == 0
    owner = np.repeat(np.arange(len(counts)), counts)          # step-major
    assert np.array_equal(p.evidx, owner.astype(np.uint32))
    kind = steps.steps['kind'][owner]
    assert np.array_equal(p.flags, np.where(kind == gs.CHERENKOV, 1 << 10, np.where(kind == gs.SCINTILLATION, 1 << 11, 0)))
    assert np.all(p.weights == 1.0) and np.all(p.last_hit_triangles == -1)
    for f in ('pos', 'dir', 'pol', 'wavelengths', 't'):
        assert np.isfinite(getattr(p, f)).all(), f
    # pos on the segment, pos and t from the same f
    x0, dx = np.array(genstep_scene.X0), np.array(genstep_scene.DX)
    f3 = (p.pos.astype(np.float64) - x0) / dx
    f = f3[:, 0]
    assert np.all((f > 0) & (f <= 1.0 + 1e-6))
    assert np.abs(f3 - f[:, None]).max() < 1e-5
    prompt = kind != gs.SCINTILLATION
    ft = (p.t.astype(np.float64) - genstep_scene.T0) / genstep_scene.DT
    assert np.abs(ft[prompt] - f[prompt]).max() < 1e-5
    # scintillation adds a delay >= 0 drawn from the time CDF (mean 5 ns here)
    delay = (ft[~prompt] - f[~prompt]) * genstep_scene.DT
    assert delay.min() > -1e-5 and 3.0 < delay.mean() < 7.0
    # wavelengths inside each step's range
    for i, s in enumerate(steps.steps):
        if s['kind'] != gs.SCINTILLATION and s['nphotons']:
            wl = p.wavelengths[owner == i]
            assert wl.min() >= s['wl_lo'] * (1 - 1e-6) and wl.max() <= s['wl_hi'] * (1 + 1e-6)


def test_depends_on_seed_and_slots_only(scene, mixed):
    packed, m = scene
    steps, p, _ = mixed
    again, _, st1 = _generate(packed, steps, seed=5)
    for f in ('pos', 'dir', 'pol', 'wavelengths', 't'):
        assert np.array_equal(getattr(again, f), getattr(p, f))
    other, _, _ = _generate(packed, steps, seed=6)
    assert not np.array_equal(other.dir, p.dir)
    # photon k is drawn by slot k mod nslots in ascending k: a slot's first photon uses the
    # first uniform of its fresh state as f
    st = gs.rng_init_host(NSLOTS, seed=5)
    x0, dx = np.float32(genstep_scene.X0[0]), np.float32(genstep_scene.DX[0])
    for slot in (0, 1, 77, 127):
        u = oracle.uniforms(st, NSLOTS, slot, 1)[0]
        assert p.pos[slot, 0] == np.float32(np.float64(u) * np.float64(dx) + np.float64(x0))


def test_first_photon_offset(scene, mixed):
    packed, m = scene
    steps, p, _ = mixed
    st = gs.rng_init_host(NSLOTS, seed=5)
    q, _ = gs.generate_photons_host(steps, packed, st, first_photon=5, capacity=len(p) + 9)
    assert np.array_equal(q.dir[5:5 + len(p)], p.dir) and np.array_equal(q.t[5:5 + len(p)], p.t)
    assert not q.dir[:5].any() and not q.dir[5 + len(p):].any() and not q.weights[:5].any()


def test_unit_vectors(mixed):
    _, p, _ = mixed
    d, e = p.dir.astype(np.float64), p.pol.astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-5
    assert np.abs(np.linalg.norm(e, axis=1) - 1).max() < 1e-5
    assert np.abs((d * e).sum(axis=1)).max() < 1e-5


@pytest.mark.parametrize('direction', [(100.0, -50.0, 25.0), (0.0, 0.0, 1.0), (0.0, -2.0, 0.0), (3.0, 3.0, 3.0),
                                       (-1e-3, 5.0, 1e-3)])
def test_cherenkov_angle(scene, direction):
    packed, m = scene
    beta = 0.9
    steps = gs.cherenkov_step(m['disp'], 5000, x0=(0, 0, 0), dx=direction, beta=beta,
                              wavelength_range=(300.0, 600.0))
    p, exhausted, _ = _generate(packed, steps, seed=3)
    assert exhausted == 0
    u = np.asarray(direction, np.float64)
    u /= np.linalg.norm(u)
    d, e = p.dir.astype(np.float64), p.pol.astype(np.float64)
    cos = 1.0 / (beta * _n_of(packed, m['disp'], p.wavelengths))
    assert np.abs(d @ u - cos).max() < 1e-5
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-5
    assert np.abs(np.linalg.norm(e, axis=1) - 1).max() < 1e-5
    assert np.abs((d * e).sum(axis=1)).max() < 1e-5
    assert np.abs((np.cross(d, e) @ u)).max() < 1e-5              # pol coplanar with u and dir
    want = cos[:, None] * d - u                                       # pol = normalise(cos dir - u)
    want /= np.linalg.norm(want, axis=1)[:, None]
    assert np.abs(e - want).max() < 1e-5
    # the azimuth about u is uniform
    a = np.array([1.0, 0, 0]) if abs(u[0]) < 0.9 else np.array([0, 1.0, 0])
    e1 = np.cross(u, a); e1 /= np.linalg.norm(e1)
    phi = np.arctan2(d @ np.cross(u, e1), d @ e1)
    assert stats.kstest(phi, stats.uniform(-np.pi, 2 * np.pi).cdf).pvalue > KS_P


def test_cherenkov_wavelength_constant_n(scene):
    """dN/dwl ~ 1/wl^2 where n does not depend on the wavelength."""
    packed, m = scene
    lo, hi = 300.0, 600.0
    steps = gs.cherenkov_step(m['water'], KS_N, x0=(0, 0, 0), dx=(0, 0, 1), beta=0.95, wavelength_range=(lo, hi))
    p, exhausted, _ = _generate(packed, steps, seed=11, nslots=1024)
    assert exhausted == 0
    cdf = lambda w: (1 / lo - 1 / np.asarray(w, np.float64)) / (1 / lo - 1 / hi)   # noqa: E731
    res = stats.kstest(p.wavelengths.astype(np.float64), cdf)
    print('constant n: KS p = %.4g' % res.pvalue)
    assert res.pvalue > KS_P


def test_cherenkov_wavelength_dispersive(scene):
    """dN/dwl ~ (1 - 1/(beta n(wl))^2) / wl^2 (Frank-Tamm), integrated numerically."""
    packed, m = scene
    lo, hi, beta = 300.0, 600.0, 0.78          # sin^2 varies by a factor 1.6 over the range
    steps = gs.cherenkov_step(m['disp'], KS_N, x0=(0, 0, 0), dx=(0, 0, 1), beta=beta, wavelength_range=(lo, hi))
    p, exhausted, _ = _generate(packed, steps, seed=12, nslots=1024)
    assert exhausted == 0
    w = np.linspace(lo, hi, 300001)
    pdf = (1 - 1 / (beta * _n_of(packed, m['disp'], w)) ** 2) / w ** 2
    assert pdf.min() > 0
    c = np.concatenate([[0], np.cumsum(0.5 * (pdf[1:] + pdf[:-1]) * np.diff(w))])
    c /= c[-1]
    res = stats.kstest(p.wavelengths.astype(np.float64), lambda x: np.interp(x, w, c))
    print('dispersive: KS p = %.4g' % res.pvalue)
    assert res.pvalue > KS_P
    # and it is not the constant-n spectrum
    flat = stats.kstest(p.wavelengths.astype(np.float64), lambda x: (1 / lo - 1 / x) / (1 / lo - 1 / hi))
    assert flat.pvalue < 1e-6


@pytest.mark.parametrize('component', [0, 1])
def test_scintillation_spectrum_and_delay(scene, component):
    packed, m = scene
    steps = gs.scintillation_step(m['scint'], KS_N, x0=(1, 2, 3), component=component)
    p, exhausted, _ = _generate(packed, steps, seed=13 + component, nslots=1024)
    assert exhausted == 0
    wcdf = _table(packed, m['scint'], 'comp_reemission_wvl_cdf')[component][:-1].astype(np.float64)
    tcdf = _table(packed, m['scint'], 'comp_reemission_time_cdf')[component][:-1].astype(np.float64)
    rw = stats.kstest(p.wavelengths.astype(np.float64),
                      lambda x: np.interp(x, packed.wavelengths.astype(np.float64), wcdf))
    rt = stats.kstest(p.t.astype(np.float64), lambda x: np.interp(x, packed.times.astype(np.float64), tcdf))
    print('scintillation %d: KS p = %.4g (wavelength), %.4g (delay)' % (component, rw.pvalue, rt.pvalue))
    assert rw.pvalue > KS_P and rt.pvalue > KS_P
    assert np.all(p.pos == np.float32([1, 2, 3]))


def test_isotropic_direction_and_wavelength(scene):
    packed, m = scene
    steps = gs.isotropic_flash(m['water'], KS_N, wavelength_range=(380.0, 500.0))
    p, exhausted, _ = _generate(packed, steps, seed=17, nslots=1024)
    assert exhausted == 0
    rz = stats.kstest(p.dir[:, 2].astype(np.float64), stats.uniform(-1, 2).cdf)
    rw = stats.kstest(p.wavelengths.astype(np.float64), stats.uniform(380, 120).cdf)
    rphi = stats.kstest(np.arctan2(p.dir[:, 1], p.dir[:, 0]).astype(np.float64), stats.uniform(-np.pi, 2 * np.pi).cdf)
    print('isotropic: KS p = %.4g (dir_z), %.4g (wavelength), %.4g (azimuth)' % (rz.pvalue, rw.pvalue, rphi.pvalue))
    assert rz.pvalue > KS_P and rw.pvalue > KS_P and rphi.pvalue > KS_P


def test_rejection_loop_exhaustion(scene):
    """beta a hair above threshold for the last nanometre of the dispersive table
    (n > 1/beta only above 599 nm; n_max = 1.36 at 600 nm): a try is accepted with
    probability ~8e-4, so about 4 photons in 10 use up CHR_GEN_MAX_TRIES = 1024
    tries and are emitted at the wavelength of n_max.  The run terminates."""
    packed, m = scene
    beta = 1.0 / 1.3599
    n = _n_of(packed, m['disp'], np.linspace(300, 600, 3001))
    assert (beta * n > 1).any() and (beta * n < 1).mean() > 0.99
    steps = gs.cherenkov_step(m['disp'], 2000, x0=(0, 0, 0), dx=(1, 2, 3), beta=beta, wavelength_range=(300.0, 600.0))
    p, exhausted, _ = _generate(packed, steps, seed=19)
    print('exhausted %d of 2000' % exhausted)
    assert 0 < exhausted < 2000
    for f in ('pos', 'dir', 'pol', 'wavelengths', 't'):
        assert np.isfinite(getattr(p, f)).all(), f
    assert (p.wavelengths == np.float32(600.0)).sum() >= exhausted
    assert p.wavelengths.min() > 598.9
    assert np.abs(np.linalg.norm(p.dir.astype(np.float64), axis=1) - 1).max() < 1e-5


def _bad_records(m):
    good = dict(x0=(0, 0, 0), dx=(0, 0, 1))
    ch = lambda **kw: gs.cherenkov_step(m['disp'], 10, **dict(dict(good, beta=0.9, wavelength_range=(300.0, 600.0)), **kw))  # noqa: E731
    iso = lambda **kw: gs.isotropic_flash(m['water'], 10, **kw)   # noqa: E731

    def raw(g, **fields):
        for k, v in fields.items():
            g.steps[k] = v
        return g
    return {
        'unknown kind': raw(iso(), kind=3),
        'material out of range': gs.isotropic_flash(99, 10),
        'component out of range': gs.scintillation_step(m['scint'], 10, x0=(0, 0, 0), component=2),
        'component of a material without any': gs.scintillation_step(m['water'], 10, x0=(0, 0, 0)),
        'nan position': iso(x0=(np.nan, 0, 0)),
        'infinite extent': iso(dx=(0, np.inf, 0)),
        'nan time': iso(t0=np.nan),
        'infinite duration': iso(dt=-np.inf),
        'nan beta': ch(beta=np.nan),
        'wl_lo > wl_hi': iso(wavelength_range=(500.0, 400.0)),
        'zero wavelength limit': iso(wavelength_range=(0.0, 400.0)),
        'negative wavelength limit': ch(wavelength_range=(-300.0, 600.0)),
        'nan wavelength limit': iso(wavelength_range=(300.0, np.nan)),
        'cherenkov without direction': ch(dx=(0, 0, 0)),
        'beta zero': ch(beta=0.0),
        'beta negative': ch(beta=-0.5),
        'beta above one': ch(beta=1.0001),
        'below threshold': ch(beta=0.7),                       # 0.7 * 1.36 < 1
        'below threshold, constant n': gs.cherenkov_step(m['water'], 10, beta=0.75, **good),   # 0.75 * 1.33 < 1
    }


def test_validation(scene):
    packed, m = scene
    for label, steps in _bad_records(m).items():
        with pytest.raises(NativeError):
            _generate(packed, steps)
            pytest.fail('accepted: ' + label)
    good = gs.isotropic_flash(m['water'], 10)
    p, _, _ = _generate(packed, good)
    assert len(p) == 10
    with pytest.raises(NativeError):                                   # more photons than the capacity
        _generate(packed, good, capacity=9)
    with pytest.raises(NativeError):
        _generate(packed, good, first_photon=3, capacity=12)
    with pytest.raises(NativeError):                                   # more than 2^31 - 1 in all
        _generate(packed, gs.isotropic_flash(m['water'], 2 ** 31 - 1) + gs.isotropic_flash(m['water'], 1))
    assert gs.count(gs.isotropic_flash(0, 2 ** 32 - 1) + gs.isotropic_flash(0, 2 ** 32 - 1)) == 2 ** 33 - 2
    with pytest.raises(NativeError):                                   # no rng states
        gs.generate_photons_host(good, packed, np.zeros(0, np.uint32))
    with pytest.raises(NativeError):
        gs.rng_init_host(0)
    # a refused call leaves the states as they were
    st = gs.rng_init_host(NSLOTS, seed=1)
    before = st.copy()
    with pytest.raises(NativeError):
        gs.generate_photons_host(good + _bad_records(m)['beta zero'], packed, st)
    assert np.array_equal(st, before)


def test_material_objects_resolve_to_indices(scene):
    packed, m = scene
    i = [k for k, x in enumerate(packed.material_objects) if x is m['disp']][0]
    by_object = gs.cherenkov_step(m['disp'], 100, x0=(0, 0, 0), dx=(0, 1, 0), beta=0.9)
    by_index = gs.cherenkov_step(i, 100, x0=(0, 0, 0), dx=(0, 1, 0), beta=0.9)
    assert by_object.records(packed.material_objects)['material'][0] == i
    a, _, _ = _generate(packed, by_object)
    b, _, _ = _generate(packed, by_index)
    assert np.array_equal(a.dir, b.dir) and np.array_equal(a.wavelengths, b.wavelengths)
    with pytest.raises(ValueError):
        gs.isotropic_flash(scenes_glass(), 1).records(packed.material_objects)


def scenes_glass():
    import scenes
    return scenes.materials()['glass']        # a Material object that is not part of the geometry


@pytest.mark.parametrize('nslots,seed,offset,first', [(1, 1, 0, 0), (5, 1, 0, 0), (64, 2 ** 40 + 12345, 0, 0),
                                                      (7, 9, 3, 0), (33, 7, 1000003, 128), (3, 0, 0, 2 ** 32 - 3)])
def test_rng_init_host_matches_oracle(nslots, seed, offset, first):
    got = gs.rng_init_host(nslots, seed=seed, offset=offset, first_subsequence=first)
    assert np.array_equal(got, oracle.rng_init(nslots, seed=seed, offset=offset, first_subsequence=first))
