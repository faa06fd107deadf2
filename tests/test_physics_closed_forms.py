"""The rest of the per-step photon physics pinned to closed forms outside the
oracle: the sibling of test_physics_analytic.py (same helpers, same style: one
isolated scene, one propagate with max_steps = 1, the outcome compared with a
float64 / closed-form answer computed here in numpy).

  * the Rayleigh scattering law (rayleigh_scatter, photon.h:400-453): the new
    direction makes an angle with the old polarisation whose cosine c has the
    pdf 3/4 (1 - c^2), its azimuth about the old polarisation is uniform
    (measured in the z-axis frame the kernel draws it in, too), the new
    polarisation is normalize(p0 - c d1);
  * multi-component bulk re-emission (photon.h:496-540): the component is
    chosen with probability absorption_length / comp_absorption_length, then
    re-emits with its own probability, wavelength CDF and time CDF, into an
    isotropic direction;
  * the DICHROIC surface (photon.h:877-907): R and T bilinear in (angle,
    wavelength);
  * the ANGULAR surface (photon.h:909-951): transmit / specular / diffuse
    linear in angle, and its use_weights form (no absorption, weight 1 - absorb);
  * the default surface model (photon.h:967-1035) with wavelength-dependent
    tables, its PASS remainder, and its use_weights forms (forced detection
    with weight detect; detect = 0: weight 1 - absorb);
  * use_weights and scatter_first in the bulk (photon.h:459-494, 541-568): the
    survival weight exp(-x / absorption_length), the forced / forbidden first
    scatter with weight 1 - exp(-D/L) / exp(-D/L), and WEIGHT_LOWER_THRESHOLD;
  * the analytic FP64 wire planes (photon.h:108-277) against a float64
    ray-cylinder solver written here.

Every test runs on the HIP path (-m gpu) and on the CPU oracle.  Statistical
checks ask p > P_MIN at fixed seeds (the first seed tried, everywhere);
geometric ones state their tolerance at the assert: derived from float32
where it can be, else four times the largest deviation measured on the oracle,
with the measured figure beside it.
"""
import numpy as np
import pytest
import scipy.stats

import scenes
from test_physics_analytic import (BACKENDS, C_MM_NS, NOWHERE, P_MIN, cuda,  # noqa: F401 (cuda: the fixture)
                                   _incidence, _material, _photons, _propagate, _slab_geometry, _surface,
                                   _truncated_exp_cdf)

BULK_ABSORB, DETECT, SURFACE_ABSORB, RAYLEIGH, DIFFUSE, SPECULAR, TRANSMIT, BULK_REEMIT = (
    1 << 1, 1 << 2, 1 << 3, 1 << 4, 1 << 5, 1 << 6, 1 << 8, 1 << 9)
NO_HIT, NAN_ABORT = 1 << 0, 1 << 15
ULP = 2.0 ** -23                 # float32 spacing at 1
UNIFORM_AZIMUTH = scipy.stats.uniform(-np.pi, 2 * np.pi).cdf


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def _isotropic(n, rng):
    """n isotropic unit directions and random unit polarisations orthogonal to them."""
    cz = rng.uniform(-1.0, 1.0, n)
    phi = rng.uniform(0.0, 2 * np.pi, n)
    s = np.sqrt(1.0 - cz * cz)
    d = np.column_stack((s * np.cos(phi), s * np.sin(phi), cz))
    r = rng.normal(size=(n, 3))
    pol = _unit(r - (r * d).sum(1)[:, None] * d)
    return d, pol


def _box_geometry(medium, size, surface=None, extra=()):
    """A cube of `medium` (side `size`, centred at the origin) in the same
    medium, with `surface` on its walls; `extra`: (solid, displacement) pairs."""
    from chroma import make
    from chroma.geometry import Geometry, Solid
    from chroma.loader import create_geometry_from_obj
    g = Geometry(medium)
    g.add_solid(Solid(make.box(size, size, size), medium, medium, surface=surface))
    for solid, displacement in extra:
        g.add_solid(solid, displacement=displacement)
    return create_geometry_from_obj(g, update_bvh_cache=False)


def _assert_unit_orthogonal(pol, d, what):
    """pol: unit vectors normal to d (float32 normalisation and products: 1e-5,
    the bound test_physics_analytic uses for the same property)."""
    assert np.abs(np.linalg.norm(pol, axis=1) - 1).max() < 1e-5, what
    assert np.abs((pol * d).sum(1)).max() < 1e-5, what


# ---------------------------------------------------------------- 1. Rayleigh
@pytest.mark.parametrize('backend', BACKENDS)
def test_rayleigh_scattering_law(backend, request):
    """A Rayleigh-scattered photon leaves with the dipole pattern about its old
    polarisation p0: c = d1.p0 has the pdf 3/4 (1 - c^2), i.e. the CDF
    1/2 + (3c - c^3)/4; the azimuth of d1 about p0 is uniform, both from the
    old direction and in the fixed frame the kernel draws it in, and is
    uncorrelated with c; the new polarisation is p0 with its component along
    d1 taken out, normalised.

    The reference's own arithmetic sets the precision of the last property:
    pick_new_direction (photon.h:400-427) takes the azimuth of its axis p0 as
    (p0x, p0y) / sqrt(1 - p0z^2), and a float32 unit vector has
    p0x^2 + p0y^2 = 1 - p0z^2 only to 1e-7, so that pair is a unit vector only
    to 1e-7 / (1 - p0z^2): the new direction it builds (and the polarisation
    taken from it) is off by that much where p0 lies along z.  That is the
    reference's behaviour and is pinned as such: the deviations are bounded
    after scaling with 1 - p0z^2, and unscaled at what the worst photon of
    this sample shows."""
    n = 200000
    geo = _box_geometry(_material('medium', 1.33, scat=1000.0), 6000.0)
    d, pol = _isotropic(n, np.random.default_rng(9))
    ph = _photons((1.0, 2.0, 3.0), d, pol)
    end = _propagate(backend, geo, ph, request=request)
    assert not (end.flags & (NAN_ABORT | NO_HIT)).any()
    sc = (end.flags & RAYLEIGH) != 0
    assert sc.sum() > 0.9 * n                                  # 1 - exp(-D/1000), D >= 3000 - 3
    d0, p0 = _unit(_f64(ph.dir[sc])), _unit(_f64(ph.pol[sc]))  # the kernel normalises both on load
    d1, p1 = _f64(end.dir[sc]), _f64(end.pol[sc])
    c = (d1 * p0).sum(1)
    pv = scipy.stats.kstest(c, lambda x: 0.5 + (3 * x - x ** 3) / 4).pvalue
    print('rayleigh: scattered %d, cos KS p %.3g' % (sc.sum(), pv))
    assert pv > P_MIN
    # the azimuth of d1 about p0, (a) from the old direction: uniform, and independent of how the old
    # direction lay about p0 (the input makes that orientation random, so this alone cannot tell a wrong
    # law for the drawn angle: (b) does)
    az = np.arctan2((d1 * np.cross(p0, d0)).sum(1), (d1 * d0).sum(1))
    pv = scipy.stats.kstest(az, UNIFORM_AZIMUTH).pvalue
    print('rayleigh: azimuth from the old direction KS p %.3g' % pv)
    assert pv > P_MIN
    # (b) in the frame the drawn angle phi is defined in (pick_new_direction: the polar and azimuthal unit
    # vectors of p0 about the z axis, d1 = cos(theta) p0 + sin(theta) (cos(phi) e_theta + sin(phi) e_phi)):
    # phi is uniform over the whole circle
    z = np.array([0.0, 0.0, 1.0])
    e_theta = -_unit(z - p0[:, 2:3] * p0)
    e_phi = np.cross(p0, e_theta)
    phi = np.arctan2((d1 * e_phi).sum(1), (d1 * e_theta).sum(1))
    pv = scipy.stats.kstest(phi, UNIFORM_AZIMUTH).pvalue
    print('rayleigh: azimuth in the frame of the z axis KS p %.3g' % pv)
    assert pv > P_MIN
    # and independent of the polar angle: the correlation of two independent samples of this size is
    # normal with sigma 1 / sqrt(n); 4 sigma
    for name, a, b in (('cos phi', np.cos(phi), c), ('sin phi', np.sin(phi), c),
                       ('cos 2 phi', np.cos(2 * phi), c * c)):
        r = np.corrcoef(a, b)[0, 1]
        print('rayleigh: correlation of %s with the polar cosine %.3g (sigma %.3g)' % (name, r, sc.sum() ** -0.5))
        assert abs(r) < 4 * sc.sum() ** -0.5, (name, r)
    assert np.abs(np.linalg.norm(d1, axis=1) - 1).max() < 1e-5
    assert np.abs(np.linalg.norm(p1, axis=1) - 1).max() < 1e-5
    # p0 - c d1 cancels as |c| -> 1 (its length is sqrt(1 - c^2), so float32 leaves the result off the
    # normal plane of d1 by 1e-7 / sqrt(1 - c^2)): compared where 1 - |c| >= 0.01
    keep = 1.0 - np.abs(c) >= 0.01
    excluded = 1.0 - keep.mean()
    print('rayleigh: excluded share %.3g' % excluded)
    assert excluded <= 1e-3                                    # the law puts 1.5e-4 there
    s2 = 1.0 - p0[keep, 2] ** 2
    orth = np.abs((p1[keep] * d1[keep]).sum(1))
    err = np.abs(p1[keep] - _unit(p0[keep] - c[keep, None] * d1[keep])).max(1)
    print('rayleigh: polarisation error %.3g, times 1 - p0z^2 %.3g; p1.d1 times 1 - p0z^2 %.3g' % (
        err.max(), (err * s2).max(), (orth * s2).max()))
    # measured on the oracle: 2.41e-3 (at 1 - p0z^2 = 5.2e-6), asserted with a margin of 4
    assert err.max() < 4 * 2.41e-3
    # measured on the oracle: 8.15e-7 and 7.58e-7, asserted with a margin of 4 (3.3e-6 / (1 - p0z^2): below
    # 3.3e-5 for the 95% of the photons with 1 - p0z^2 > 0.1)
    assert (err * s2).max() < 4 * 8.15e-7
    assert (orth * s2).max() < 4 * 7.58e-7
    # unscaled, away from the z axis (95% of an isotropic p0): the flat float32 bound of the other tests
    away = s2 > 0.1
    print('rayleigh: share with 1 - p0z^2 > 0.1: %.3f, p1.d1 there %.3g' % (away.mean(), orth[away].max()))
    assert away.mean() > 0.94
    assert orth[away].max() < 1e-5


# ---------------------------------------------------------------- 2. bulk re-emission
def _ramp_cdf(wl, lo, hi):
    """CDF on the grid `wl` of a pdf rising linearly from 0 at lo to its peak at hi, 0 outside."""
    return np.clip((np.asarray(wl, np.float64) - lo) / (hi - lo), 0.0, 1.0) ** 2


@pytest.mark.parametrize('backend', BACKENDS)
def test_two_component_bulk_reemission(backend, request):
    """A medium of absorption length 800 whose two components absorb with
    lengths 1200 and 2400 (800/1200 + 800/2400 = 1) and re-emit with
    probabilities 0.8 and 0.3: an absorbed photon belongs to component 0 with
    probability 2/3, and is then re-emitted with that component's probability,
    wavelength CDF (disjoint supports 310-390 / 510-590 nm tell the components
    apart) and delay CDF (exponentials of 5 / 20 ns), isotropically."""
    from chroma.geometry import standard_wavelengths as wl
    n, nref, absl, lam0 = 200000, 1.45, 800.0, 420.0
    comp_absl, comp_prob, comp_band, comp_tau = (1200.0, 2400.0), (0.8, 0.3), ((310.0, 390.0), (510.0, 590.0)), \
        (5.0, 20.0)
    times = np.arange(0, 1000, 0.05)
    medium = _material('scint', nref, absl=absl)
    wcdfs, tcdfs = [], []
    for k in range(2):
        wcdf = _ramp_cdf(wl, *comp_band[k])
        tcdf = 1.0 - np.exp(-times / comp_tau[k])
        tcdf /= tcdf[-1]
        wcdfs.append(wcdf)
        tcdfs.append(tcdf)
        medium.comp_reemission_prob.append(np.column_stack((wl, np.full(len(wl), comp_prob[k]))))
        medium.comp_reemission_wvl_cdf.append(np.column_stack((wl, wcdf)))
        medium.comp_reemission_time_cdf.append(np.column_stack((times, tcdf)))
        medium.comp_absorption_length.append(np.column_stack((wl, np.full(len(wl), comp_absl[k]))))
    geo = _box_geometry(medium, 1e5)
    d, pol = _isotropic(n, np.random.default_rng(10))
    end = _propagate(backend, geo, _photons((0.0, 0.0, 0.0), d, pol, wl=lam0), request=request)
    assert not (end.flags & (NAN_ABORT | NO_HIT)).any()
    reemit = (end.flags & BULK_REEMIT) != 0
    absorbed = (end.flags & BULK_ABSORB) != 0
    assert not (reemit & absorbed).any()
    lam = end.wavelengths.astype(np.float64)
    comp = [reemit & (lam < 450.0), reemit & (lam >= 450.0)]
    counts = np.array([comp[0].sum(), comp[1].sum(), absorbed.sum()])
    assert counts.sum() == n                                   # exp(-5e4/800): nobody reaches the wall
    p0 = absl / comp_absl[0]
    expected = np.array([p0 * comp_prob[0], (1 - p0) * comp_prob[1], 0.0])
    expected[2] = 1.0 - expected[:2].sum()
    pv = scipy.stats.chisquare(counts, expected * n).pvalue
    print('reemission: counts %s expected %s p %.3g' % (counts / n, expected, pv))
    assert pv > P_MIN
    # the absorption distance of every photon (re-emitted or not) is Exp(800)
    dist = np.linalg.norm(end.pos.astype(np.float64), axis=1)
    pv = scipy.stats.kstest(dist, scipy.stats.expon(scale=absl).cdf).pvalue
    print('reemission: distance KS p %.3g' % pv)
    assert pv > P_MIN
    grid = np.asarray(wl, np.float64)
    delay = end.t.astype(np.float64) - dist * nref / C_MM_NS
    dd, pp = end.dir.astype(np.float64), end.pol.astype(np.float64)
    for k in range(2):
        m = comp[k]
        lo, hi = comp_band[k]
        assert (lam[m] >= lo).all() and (lam[m] <= hi).all(), k
        wcdf32 = _f64(wcdfs[k])
        pvs = [scipy.stats.kstest(lam[m], lambda x: np.interp(x, grid, wcdf32)).pvalue]
        tcdf32 = _f64(tcdfs[k])
        pvs.append(scipy.stats.kstest(delay[m], lambda x: np.interp(x, times, tcdf32)).pvalue)
        pvs.append(scipy.stats.kstest(dd[m][:, 2], scipy.stats.uniform(-1, 2).cdf).pvalue)
        pvs.append(scipy.stats.kstest(np.arctan2(dd[m][:, 1], dd[m][:, 0]), UNIFORM_AZIMUTH).pvalue)
        print('reemission: component %d wavelength / delay / dir_z / azimuth KS p %s' % (k, pvs))
        assert min(pvs) > P_MIN, (k, pvs)
        _assert_unit_orthogonal(pp[m], dd[m], k)
    # the others keep their wavelength
    assert (end.wavelengths[absorbed] == np.float32(lam0)).all()


# ---------------------------------------------------------------- 3. DICHROIC
def _beams(cases, n, pol='s'):
    """n photons per (theta, ...) case onto the slab's top face: the photons and
    per case (float32-rounded incidence angle, float32 direction, normal)."""
    starts, dirs, pols, meta = [], [], [], []
    for case in cases:
        start, d, s, p, nrm = _incidence(case[0], n)
        starts.append(np.tile(start, (n, 1)))
        dirs.append(np.tile(d, (n, 1)))
        pols.append(np.tile(s if pol == 's' else p, (n, 1)))
        d32 = _unit(_f64(d))
        meta.append((float(np.arccos(np.clip(-d32 @ nrm, -1, 1))), d32, nrm))
    return np.concatenate(starts), np.concatenate(dirs), np.concatenate(pols), meta


def _table(wl, prop, lam):
    """A float32 (wavelength, value) table read at lam: linear between grid points."""
    return float(np.interp(lam, np.asarray(wl, np.float64), _f64(np.asarray(prop)[:, 1])))


def _between_rows(angles, theta):
    """(lower row, upper row, weight of the upper row) of theta in the float32 angle grid."""
    a = _f64(angles)
    i = int(np.clip(np.searchsorted(a, theta, side='right') - 1, 0, len(a) - 2))
    return i, i + 1, float(np.clip((theta - a[i]) / (a[i + 1] - a[i]), 0.0, 1.0))


DICHROIC_CASES = [(0.25, 412.5), (0.5, 500.0), (0.8, 633.0), (1.3, 377.0)]      # (theta, wavelength)
DICHROIC_ANGLES = [0.0, 0.5, 1.0, np.pi / 2]
DICHROIC_EDGES = [420.0, 500.0, 640.0, 370.0]          # one filter edge per angle row, next to a beam's wavelength


def _dichroic_surface():
    """A filter edge per angle row: reflect rises across it over a width of 15 nm
    (up to 0.013 / nm, so a wavelength read 2.5 nm off shifts R by 0.02-0.03,
    tens of sigma at n = 100,000), transmit falls with its own centre (10 nm
    further) and width (25 nm), so that it is no function of reflect and
    neither is linear in wavelength or in the row angle.  Each beam of
    DICHROIC_CASES lies on the slope of at least one of its two rows."""
    from chroma.geometry import DichroicProps, standard_wavelengths as wl
    lam = np.asarray(wl, np.float64)
    refl = [np.column_stack((lam, 0.05 + 0.8 / (1.0 + np.exp(-(lam - e) / 15.0)))) for e in DICHROIC_EDGES]
    trans = [np.column_stack((lam, 0.03 + 0.7 / (1.0 + np.exp((lam - e - 10.0) / 25.0)))) for e in DICHROIC_EDGES]
    dich = _surface('dichroic', model=3)
    dich.dichroic_props = DichroicProps(np.array(DICHROIC_ANGLES), refl, trans)
    return dich


@pytest.mark.parametrize('backend', BACKENDS)
def test_dichroic_surface_bilinear(backend, request):
    """DICHROIC: reflect / transmit probabilities linear in wavelength within
    each angle row, then linear in the incidence angle between rows; the rest
    absorbs (tables: _dichroic_surface).  A transmitted photon goes on to the
    Fresnel boundary in the same step and may be reflected there
    (TRANSMIT | SPECULAR): transmission is counted by its own bit first."""
    from chroma.geometry import standard_wavelengths as wl
    n = 100000
    dich = _dichroic_surface()
    props = dich.dichroic_props
    geo = _slab_geometry(_material('glass', 1.5), _material('water', 1.33), surface=dich)
    start, d, pol, meta = _beams(DICHROIC_CASES, n)
    ph = _photons(start, d, pol)
    ph.wavelengths[:] = np.repeat(np.array([c[1] for c in DICHROIC_CASES], np.float32), n)
    end = _propagate(backend, geo, ph, request=request)
    assert not (end.flags & (NAN_ABORT | NO_HIT)).any()
    for k, ((theta, lam), (ti, d32, nrm)) in enumerate(zip(DICHROIC_CASES, meta)):
        sl = slice(k * n, (k + 1) * n)
        f = end.flags[sl]
        lo, hi, w = _between_rows(props.angles, ti)
        R = (1 - w) * _table(wl, props.dichroic_reflect[lo], lam) + w * _table(wl, props.dichroic_reflect[hi], lam)
        T = (1 - w) * _table(wl, props.dichroic_transmit[lo], lam) + w * _table(wl, props.dichroic_transmit[hi], lam)
        assert 0.05 < R < 0.9 and 0.05 < T < 0.9 and R + T < 0.95, (theta, lam, R, T)
        trans = (f & TRANSMIT) != 0
        refl = ((f & SPECULAR) != 0) & ~trans
        absorb = (f & SURFACE_ABSORB) != 0
        counts = np.array([refl.sum(), trans.sum(), absorb.sum()])
        assert counts.sum() == n and not (absorb & (trans | refl)).any(), (theta, lam)
        pv = scipy.stats.chisquare(counts, np.array([R, T, 1 - R - T]) * n).pvalue
        print('dichroic: theta %.2f lambda %.1f counts %s expected %s p %.3g' % (theta, lam, counts / n,
                                                                               (R, T, 1 - R - T), pv))
        assert pv > P_MIN, (theta, lam, counts / n, (R, T), pv)
        mirror = d32 - 2 * (d32 @ nrm) * nrm
        assert np.abs(end.dir[sl][refl].astype(np.float64) - mirror).max() < 2e-5, (theta, lam)


# ---------------------------------------------------------------- 4. ANGULAR
ANGULAR_THETAS = [(0.2,), (0.6,), (1.0,), (1.4,)]


def _angular_probabilities(props, ti):
    lo, hi, w = _between_rows(props.angles, ti)
    t, rs, rd = ((1 - w) * float(np.float32(a[lo])) + w * float(np.float32(a[hi]))
                 for a in (props.transmit, props.reflect_specular, props.reflect_diffuse))
    return 1.0 - t - rs - rd, t, rs, rd


def _angular_counts(f):
    trans = (f & TRANSMIT) != 0
    return np.array([((f & SURFACE_ABSORB) != 0).sum(), trans.sum(), (((f & SPECULAR) != 0) & ~trans).sum(),
                     ((f & DIFFUSE) != 0).sum()])


@pytest.mark.parametrize('backend', BACKENDS)
def test_angular_surface(backend, request):
    """ANGULAR: transmit / specular / diffuse probabilities linear in the
    incidence angle between the table's angles, absorption the remainder."""
    n = 100000
    ang = scenes.surfaces()['ang']
    geo = _slab_geometry(_material('glass', 1.5), _material('water', 1.33), surface=ang)
    start, d, pol, meta = _beams(ANGULAR_THETAS, n)
    end = _propagate(backend, geo, _photons(start, d, pol), request=request)
    assert not (end.flags & (NAN_ABORT | NO_HIT)).any()
    for k, ((theta,), (ti, d32, nrm)) in enumerate(zip(ANGULAR_THETAS, meta)):
        probs = np.array(_angular_probabilities(ang.angular_props, ti))
        assert (probs > 0.05).all()
        counts = _angular_counts(end.flags[k * n:(k + 1) * n])
        assert counts.sum() == n, theta
        pv = scipy.stats.chisquare(counts, probs * n).pvalue
        print('angular: theta %.1f counts %s expected %s p %.3g' % (theta, counts / n, probs, pv))
        assert pv > P_MIN, (theta, counts / n, probs, pv)


@pytest.mark.parametrize('backend', BACKENDS)
def test_angular_surface_weighted(backend, request):
    """ANGULAR with use_weights: nobody is absorbed, every photon's weight is
    the survival probability 1 - absorb(theta), and the three other outcomes
    follow their probabilities divided by it."""
    n = 100000
    ang = scenes.surfaces()['ang']
    geo = _slab_geometry(_material('glass', 1.5), _material('water', 1.33), surface=ang)
    start, d, pol, meta = _beams(ANGULAR_THETAS, n)
    end = _propagate(backend, geo, _photons(start, d, pol), request=request, use_weights=True)
    assert not (end.flags & (NAN_ABORT | NO_HIT | SURFACE_ABSORB)).any()
    for k, ((theta,), (ti, d32, nrm)) in enumerate(zip(ANGULAR_THETAS, meta)):
        sl = slice(k * n, (k + 1) * n)
        probs = np.array(_angular_probabilities(ang.angular_props, ti))
        survive = 1.0 - probs[0]
        w = end.weights[sl].astype(np.float64)
        print('angular weighted: theta %.1f weight %.9g expected %.9g' % (theta, w[0], survive))
        assert (w == w[0]).all()
        # float32 throughout: the angle (acos of a dot product, |slope| of the tables <= 0.75 / rad), the
        # fractional index and three roundings of the sum: well inside 4 ulp of 1
        assert abs(w[0] - survive) <= 4 * ULP, (theta, w[0], survive)
        counts = _angular_counts(end.flags[sl])
        assert counts[0] == 0 and counts.sum() == n, theta
        pv = scipy.stats.chisquare(counts[1:], probs[1:] / survive * n).pvalue
        print('angular weighted: theta %.1f counts %s expected %s p %.3g' % (theta, counts[1:] / n,
                                                                           probs[1:] / survive, pv))
        assert pv > P_MIN, (theta, counts / n, probs, pv)


# ---------------------------------------------------------------- 5. default surface model
DEFAULT_LAMBDAS = [402.5, 611.0]


def _linear_tables(detect=True):
    """detect / absorb / reflect_diffuse / reflect_specular linear in wavelength
    over the whole grid, summing to 0.95 at every wavelength (the rest is the
    reference's PASS); detect=False: detect = 0 and absorb takes its share."""
    from chroma.geometry import standard_wavelengths as wl
    x = (np.asarray(wl, np.float64) - wl[0]) / (wl[-1] - wl[0])
    tables = dict(detect=0.10 + 0.30 * x, absorb=0.30 - 0.10 * x, reflect_diffuse=0.25 - 0.15 * x,
                  reflect_specular=0.30 - 0.05 * x)
    if not detect:
        tables['absorb'] = tables['absorb'] + tables['detect']
        tables['detect'] = np.zeros_like(x)
    return tables


def _default_scene(tables):
    # index-matched media: a PASS photon goes on to a Fresnel boundary that reflects nobody
    # (n1 = n2, off normal incidence), so SPECULAR is the surface's alone
    surface = _surface('tables', **tables)
    geo = _slab_geometry(_material('inside', 1.33), _material('outside', 1.33), surface=surface)
    return surface, geo


def _default_beams(n):
    start, d, pol, meta = _beams([(0.4,)] * len(DEFAULT_LAMBDAS), n)
    ph = _photons(start, d, pol)
    ph.wavelengths[:] = np.repeat(np.array(DEFAULT_LAMBDAS, np.float32), n)
    return ph


def _default_probabilities(surface, lam):
    from chroma.geometry import standard_wavelengths as wl
    return [_table(wl, getattr(surface, name), lam)
            for name in ('detect', 'absorb', 'reflect_diffuse', 'reflect_specular')]


def _default_counts(f):
    cats = [(f & bit) != 0 for bit in (DETECT, SURFACE_ABSORB, DIFFUSE, SPECULAR)]
    none = ~(cats[0] | cats[1] | cats[2] | cats[3])
    return np.array([c.sum() for c in cats + [none]])


@pytest.mark.parametrize('backend', BACKENDS)
def test_default_surface_wavelength_tables(backend, request):
    """The default surface model: detect / absorb / diffuse / specular with the
    tables' probabilities at the photon's wavelength (linear between grid
    points), and the reference's PASS for the remaining 5%."""
    n = 100000
    surface, geo = _default_scene(_linear_tables())
    end = _propagate(backend, geo, _default_beams(n), request=request)
    assert not (end.flags & (NAN_ABORT | NO_HIT)).any()
    for k, lam in enumerate(DEFAULT_LAMBDAS):
        probs = _default_probabilities(surface, lam)
        probs.append(1.0 - sum(probs))
        assert abs(probs[4] - 0.05) < 1e-6
        counts = _default_counts(end.flags[k * n:(k + 1) * n])
        assert counts.sum() == n, lam
        pv = scipy.stats.chisquare(counts, np.array(probs) * n).pvalue
        print('default: lambda %.1f counts %s expected %s p %.3g' % (lam, counts / n, probs, pv))
        assert pv > P_MIN, (lam, counts / n, probs, pv)


@pytest.mark.parametrize('backend', BACKENDS)
def test_default_surface_weighted_detection(backend, request):
    """use_weights with detect > 0: every photon is detected and carries the
    weight detect(lambda) ((1 - absorb) * (detect / (1 - absorb)) in float32)."""
    n = 20000
    surface, geo = _default_scene(_linear_tables())
    end = _propagate(backend, geo, _default_beams(n), request=request, use_weights=True)
    for k, lam in enumerate(DEFAULT_LAMBDAS):
        sl = slice(k * n, (k + 1) * n)
        assert (end.flags[sl] == DETECT).all(), lam
        detect = _default_probabilities(surface, lam)[0]
        w = end.weights[sl].astype(np.float64)
        print('default weighted: lambda %.1f weight %.9g expected %.9g' % (lam, w[0], detect))
        assert (w == w[0]).all()
        # two table reads, a division and two products in float32, all of values below 1: 4 ulp of 1
        assert abs(w[0] - detect) <= 4 * ULP, (lam, w[0], detect)


@pytest.mark.parametrize('backend', BACKENDS)
def test_default_surface_weighted_no_detection(backend, request):
    """use_weights with detect = 0: nobody is absorbed, the weight is
    1 - absorb(lambda), and diffuse : specular : PASS follow their
    probabilities divided by it."""
    n = 100000
    surface, geo = _default_scene(_linear_tables(detect=False))
    end = _propagate(backend, geo, _default_beams(n), request=request, use_weights=True)
    assert not (end.flags & (NAN_ABORT | NO_HIT | SURFACE_ABSORB | DETECT)).any()
    for k, lam in enumerate(DEFAULT_LAMBDAS):
        sl = slice(k * n, (k + 1) * n)
        detect, absorb, diffuse, specular = _default_probabilities(surface, lam)
        assert detect == 0.0
        survive = 1.0 - absorb
        w = end.weights[sl].astype(np.float64)
        print('default weighted, no detect: lambda %.1f weight %.9g expected %.9g' % (lam, w[0], survive))
        assert (w == w[0]).all()
        assert abs(w[0] - survive) <= 4 * ULP, (lam, w[0], survive)      # one table read and a subtraction
        counts = _default_counts(end.flags[sl])[2:]
        assert counts.sum() == n, lam
        expected = np.array([diffuse, specular, survive - diffuse - specular]) / survive
        pv = scipy.stats.chisquare(counts, expected * n).pvalue
        print('default weighted, no detect: lambda %.1f counts %s expected %s p %.3g' % (lam, counts / n,
                                                                                       expected, pv))
        assert pv > P_MIN, (lam, counts / n, expected, pv)


# ---------------------------------------------------------------- 6. weights in the bulk
def _bulk_scene(scat, absl):
    """The medium of test_beer_lambert_distances: its boundary D ~ 3000 mm along
    a beam with no zero direction component.  Returns (geometry, direction,
    polarisation, D)."""
    from chroma import make
    from chroma.geometry import Geometry, Solid
    from chroma.loader import create_geometry_from_obj
    medium = _material('medium', 1.33, absl=absl, scat=scat)
    g = Geometry(medium)
    g.add_solid(Solid(make.box(1e5, 1e5, 6000.0), medium, medium))          # top face at z = 3000
    geo = create_geometry_from_obj(g, update_bvh_cache=False)
    d = np.array([1e-3, 2e-3, 1.0])
    d /= np.linalg.norm(d)
    D = 3000.0 / float(_unit(_f64(d))[2])
    pol = np.cross(d, [1.0, 0.0, 0.0])
    pol /= np.linalg.norm(pol)
    return geo, d, pol, D


def _bulk_run(backend, request, n, scat, absl, **kw):
    geo, d, pol, D = _bulk_scene(scat, absl)
    end = _propagate(backend, geo, _photons((0, 0, 0), np.tile(d, (n, 1)), np.tile(pol, (n, 1))), request=request,
                     **kw)
    assert not (end.flags & (NAN_ABORT | NO_HIT)).any()
    scattered = (end.flags & RAYLEIGH) != 0
    dist = np.linalg.norm(end.pos.astype(np.float64), axis=1)
    assert np.abs(end.pos[~scattered & ((end.flags & BULK_ABSORB) == 0)][:, 2] - 3000.0).max(initial=0) < 1e-2
    return end, scattered, dist, D


@pytest.mark.parametrize('backend', BACKENDS)
def test_bulk_survival_weights(backend, request):
    """use_weights in the bulk: absorption never ends a photon; it scatters
    within D with probability 1 - exp(-D/1000) and carries the survival
    probability of its path, exp(-x/2500), as its weight (x the scattering
    distance, or D at the boundary)."""
    n, scat, absl = 100000, 1000.0, 2500.0
    end, scattered, dist, D = _bulk_run(backend, request, n, scat, absl, use_weights=True)
    assert not (end.flags & BULK_ABSORB).any()
    pv = scipy.stats.binomtest(int(scattered.sum()), n, 1.0 - np.exp(-D / scat)).pvalue
    assert pv > P_MIN, (scattered.mean(), 1.0 - np.exp(-D / scat))
    assert scipy.stats.kstest(dist[scattered], _truncated_exp_cdf(scat, D)).pvalue > P_MIN
    w = end.weights.astype(np.float64)
    # x is read back from the float32 end position (|pos| <= 3000: 2e-4 mm, 1e-7 of 2500), expf is good to
    # an ulp or two, the weight is below 1: 4 ulp of 1.  The oracle's largest error is 6.6e-8.
    err = np.abs(w[scattered] - np.exp(-dist[scattered] / absl)).max()
    print('bulk weights: scattered %.4f, weight error %.3g (scattered) %.3g (boundary)' % (
        scattered.mean(), err, np.abs(w[~scattered] - np.exp(-D / absl)).max()))
    assert err <= 4 * ULP
    assert np.abs(w[~scattered] - np.exp(-D / absl)).max() <= 4 * ULP


@pytest.mark.parametrize('backend', BACKENDS)
def test_scatter_first_forced(backend, request):
    """scatter_first = 1: every photon scatters before the boundary, at a
    distance from the exponential truncated to [0, D], with weight 1 - exp(-D/L)."""
    n, L = 100000, 1000.0
    end, scattered, dist, D = _bulk_run(backend, request, n, L, NOWHERE, scatter_first=1)
    assert scattered.all()
    pv = scipy.stats.kstest(dist, _truncated_exp_cdf(L, D)).pvalue
    print('scatter_first=1: distance KS p %.3g, weight %.9g expected %.9g' % (pv, end.weights[0],
                                                                           1.0 - np.exp(-D / L)))
    assert pv > P_MIN
    assert (dist <= D * (1 + 1e-6)).all()
    assert (end.weights == end.weights[0]).all()
    # D is the float32 walk distance (1e-7 relative, exp(-3) * 3e-7 in the weight), expf and a subtraction
    assert abs(float(end.weights[0]) - (1.0 - np.exp(-D / L))) <= 4 * ULP


@pytest.mark.parametrize('backend', BACKENDS)
def test_scatter_first_forbidden(backend, request):
    """scatter_first = -1: nobody scatters, every photon reaches the boundary with weight exp(-D/L)."""
    n, L = 100000, 1000.0
    end, scattered, dist, D = _bulk_run(backend, request, n, L, NOWHERE, scatter_first=-1)
    assert not scattered.any()
    assert (end.flags == 0).all()                              # at the boundary of a medium with itself
    print('scatter_first=-1: weight %.9g expected %.9g' % (end.weights[0], np.exp(-D / L)))
    assert (end.weights == end.weights[0]).all()
    assert abs(float(end.weights[0]) - np.exp(-D / L)) <= 4 * ULP


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('scatter_first,L', [(1, 1e8), (-1, 300.0)])
def test_scatter_first_below_weight_threshold(backend, scatter_first, L, request):
    """Where the forced outcome's probability is below WEIGHT_LOWER_THRESHOLD
    (1e-4) nothing is forced: weights stay exactly 1 and the photons scatter
    as they would without scatter_first.  L = 1e8: 1 - exp(-D/L) = 3e-5;
    L = 300: exp(-D/L) = 4.5e-5."""
    n = 100000
    end, scattered, dist, D = _bulk_run(backend, request, n, L, NOWHERE, scatter_first=scatter_first)
    forced = 1.0 - np.exp(-D / L) if scatter_first == 1 else np.exp(-D / L)
    assert forced < 1e-4
    assert (end.weights == np.float32(1.0)).all()
    k = int(scattered.sum())
    pv = scipy.stats.binomtest(k, n, 1.0 - np.exp(-D / L)).pvalue
    print('threshold: scatter_first %d scattered %d of %d, p %.3g' % (scatter_first, k, n, pv))
    assert pv > P_MIN, (k, n * (1.0 - np.exp(-D / L)))
    assert k < n if scatter_first == 1 else k > 0              # the outcome is not forced


# ---------------------------------------------------------------- 7. analytic wire planes
WIRE_Z, WIRE_PITCH, WIRE_RADIUS, WIRE_WINDOW = 600.0, 40.0, 3.0, 700.0


def _wire_geometry(plate=False):
    """A 4 m black-walled water box with one wire plane at z = 600: wires along
    x (u = x), stepping in y (v = y) with pitch 40, radius 3, mirror surface,
    u and v windows +-700.  plate: a black plate at z = 395..405 under it."""
    from chroma import make
    from chroma.geometry import Solid
    water, metal = _material('water', 1.33), _material('metal', 1.2)
    black = _surface('black', absorb=1.0)
    extra = [(Solid(make.box(3000.0, 3000.0, 10.0), metal, water, surface=black), (0, 0, 400))] if plate else []
    geo = _box_geometry(water, 4000.0, surface=black, extra=extra)
    geo.wireplanes = [dict(origin=(0.0, 0.0, WIRE_Z), u=(1.0, 0.0, 0.0), v=(0.0, 1.0, 0.0), pitch=WIRE_PITCH,
                           radius=WIRE_RADIUS, umin=-WIRE_WINDOW, umax=WIRE_WINDOW, vmin=-WIRE_WINDOW,
                           vmax=WIRE_WINDOW, v0=0.0, surface=_surface('wire', reflect_specular=1.0),
                           material_inner=metal, material_outer=water)]
    return geo


def _ray_cylinders(o, d):
    """Float64 ray-cylinder solver, independent of the kernel's slab and
    k-range pruning: per ray the smallest root t > 1e-4 of
    |(o + t d - axis_k)_yz|^2 = r^2 over the wires k = -17..17 (axes along x
    at y = 40 k, z = 600), kept only if the hit's x lies inside the u window.
    Returns (t or inf, the hit's unit normal, the smallest | |closest approach|
    - r | over the wires)."""
    ks = np.arange(-17, 18)
    assert ks[0] == np.ceil(-WIRE_WINDOW / WIRE_PITCH) and ks[-1] == np.floor(WIRE_WINDOW / WIRE_PITCH)
    wv = o[:, 1, None] - ks[None, :] * WIRE_PITCH
    wn = (o[:, 2] - WIRE_Z)[:, None] + 0 * wv
    dv, dn = d[:, 1, None], d[:, 2, None]
    A = dv * dv + dn * dn
    B = wv * dv + wn * dn
    C = wv * wv + wn * wn - WIRE_RADIUS ** 2
    disc = B * B - A * C
    with np.errstate(invalid='ignore'):
        sq = np.sqrt(disc)
        t = np.where(disc >= 0, (-B - sq) / A, np.inf)
        t = np.where(t > 1e-4, t, np.where(disc >= 0, (-B + sq) / A, np.inf))
    t = np.where(t > 1e-4, t, np.inf)
    k = np.argmin(t, axis=1)
    rows = np.arange(len(o))
    tmin = t[rows, k]
    hit = np.isfinite(tmin)
    tt = np.where(hit, tmin, 0.0)
    tmin = np.where(hit & (np.abs(o[:, 0] + tt * d[:, 0]) <= WIRE_WINDOW), tmin, np.inf)
    nv, nn = wv[rows, k] + tt * d[:, 1], wn[rows, k] + tt * d[:, 2]
    normal = np.column_stack((np.zeros(len(o)), nv, nn)) / WIRE_RADIUS
    tangency = np.abs(np.abs(wv * dn - wn * dv) / np.sqrt(A) - WIRE_RADIUS).min(axis=1)
    return tmin, normal, tangency


@pytest.mark.parametrize('backend', BACKENDS)
def test_wire_plane_oblique_beam(backend, request):
    """An oblique beam through the wire plane: exactly the photons the float64
    solver sends onto a wire hit one (last_hit_triangles == -2), where it says,
    and leave mirrored about the cylinder's normal there; the others end on the
    black wall at z = 2000."""
    n = 100000
    geo = _wire_geometry()
    rng = np.random.default_rng(12)
    pos = np.column_stack((rng.uniform(-500, 500, n), rng.uniform(-500, 500, n), np.full(n, 100.0)))
    d = np.array([0.05, np.sin(np.radians(25.0)), np.cos(np.radians(25.0))])
    d /= np.linalg.norm(d)
    pol = _unit(np.cross(d, [1.0, 0.0, 0.0]))
    ph = _photons(pos, np.tile(d, (n, 1)), np.tile(pol, (n, 1)))
    end = _propagate(backend, geo, ph, request=request)
    assert not (end.flags & (NAN_ABORT | NO_HIT)).any()
    o, dd = _f64(ph.pos), _unit(_f64(ph.dir))
    t, normal, tangency = _ray_cylinders(o, dd)
    clear = tangency >= 1e-3                                   # a grazing ray's hit / miss is rounding's
    print('wire oblique: excluded share %.3g' % (1.0 - clear.mean()))
    assert 1.0 - clear.mean() <= 1e-3
    wire = end.last_hit_triangles == -2
    expect = np.isfinite(t)
    print('wire oblique: %d wire hits, %d expected, %d mismatches' % (wire.sum(), expect.sum(),
                                                                      (wire != expect)[clear].sum()))
    assert 0.1 * n < expect.sum() < 0.3 * n                    # 2 r / pitch = 0.15 of the plane is wire
    assert (wire == expect)[clear].all()
    m = wire & expect & clear
    assert ((end.flags[m] & SPECULAR) != 0).all()
    perr = np.abs(end.pos[m].astype(np.float64) - (o[m] + t[m, None] * dd[m])).max()
    mirror = dd[m] - 2 * (dd[m] * normal[m]).sum(1)[:, None] * normal[m]
    derr = np.abs(end.dir[m].astype(np.float64) - mirror).max()
    print('wire oblique: position error %.3g mm, direction error %.3g' % (perr, derr))
    assert perr < 4 * 7.57e-5                                  # measured on the oracle: 7.57e-5 mm, margin 4
    assert derr < 4 * 2.31e-5                                  # measured on the oracle: 2.31e-5, margin 4
    rest = ~wire & clear
    assert ((end.flags[rest] & SURFACE_ABSORB) != 0).all() and (end.last_hit_triangles[rest] >= 0).all()
    assert np.abs(end.pos[rest][:, 2] - 2000.0).max() < 1e-2


@pytest.mark.parametrize('backend', BACKENDS)
def test_wire_plane_in_plane_beam(backend, request):
    """A beam inside the wire layer, parallel to the plane (no component along
    its normal: the kernel's |dn| <= 1e-12 branch): every photon hits the first
    wire ahead, at the solver's distance.  (The zero direction component makes
    a 'flat' walk: n is small.)"""
    n = 2000
    geo = _wire_geometry()
    rng = np.random.default_rng(13)
    pos = np.column_stack((rng.uniform(-500, 500, n), rng.uniform(-500, 500, n),
                           WIRE_Z + rng.uniform(-2.9, 2.9, n)))
    axis_y = np.round(pos[:, 1] / WIRE_PITCH) * WIRE_PITCH
    pos = pos[np.hypot(pos[:, 1] - axis_y, pos[:, 2] - WIRE_Z) >= 3.2]        # not inside or on a wire
    n = len(pos)
    assert n > 1500
    d = np.array([0.05, 1.0, 0.0])
    d /= np.linalg.norm(d)
    ph = _photons(pos, np.tile(d, (n, 1)), np.tile([0.0, 0.0, 1.0], (n, 1)))
    end = _propagate(backend, geo, ph, request=request)
    o, dd = _f64(ph.pos), _unit(_f64(ph.dir))
    assert (dd[:, 2] == 0).all()
    t, normal, tangency = _ray_cylinders(o, dd)
    assert np.isfinite(t).all() and (t < (WIRE_PITCH + WIRE_RADIUS) * 1.01).all() and tangency.min() > 1e-3
    assert (end.last_hit_triangles == -2).all()
    assert ((end.flags & SPECULAR) != 0).all()
    perr = np.abs(end.pos.astype(np.float64) - (o + t[:, None] * dd)).max()
    print('wire in-plane: %d photons, position error %.3g mm' % (n, perr))
    assert perr < 4 * 3.01e-5                                  # measured on the oracle: 3.01e-5 mm, margin 4


@pytest.mark.parametrize('backend', BACKENDS)
def test_wire_plane_misses(backend, request):
    """No wire hit for a photon outside the u window, for one heading away
    from the plane, or where a mesh face (a plate at z = 395) is nearer than
    the wires: the mesh wins."""
    n = 3000
    rng = np.random.default_rng(14)
    d = _unit(np.array([1e-3, 2e-3, 1.0]))
    pol = _unit(np.cross(d, [1.0, 0.0, 0.0]))
    y = rng.uniform(-500, 500, 3 * n)
    x = np.concatenate((rng.uniform(WIRE_WINDOW + 10, 1500, n), rng.uniform(-500, 500, 2 * n)))
    z = np.concatenate((np.full(n, 100.0), np.full(n, WIRE_Z + 50.0), np.full(n, 100.0)))
    dirs = np.concatenate((np.tile(d, (n, 1)), np.tile(d, (n, 1)), np.tile(d * [1, 1, -1], (n, 1))))
    ph = _photons(np.column_stack((x, y, z)), dirs, np.tile(pol, (3 * n, 1)))
    end = _propagate(backend, _wire_geometry(), ph, request=request)
    assert (end.last_hit_triangles >= 0).all()
    assert (end.flags == SURFACE_ABSORB).all()
    assert np.abs(np.abs(end.pos[:, 2]) - 2000.0).max() < 1e-2
    # under the plate the same upward beam that crosses the wire layer never reaches it
    up = slice(0, n)
    pos = np.column_stack((rng.uniform(-500, 500, n), y[up], z[up]))
    ph = _photons(pos, dirs[up], np.tile(pol, (n, 1)))
    t, _, _ = _ray_cylinders(_f64(ph.pos), _unit(_f64(ph.dir)))
    assert np.isfinite(t).sum() > 0.1 * n                      # without the plate these would hit wires
    end = _propagate(backend, _wire_geometry(plate=True), ph, request=request)
    assert (end.last_hit_triangles >= 0).all()
    assert (end.flags == SURFACE_ABSORB).all()
    assert np.abs(end.pos[:, 2] - 395.0).max() < 1e-2
