"""The wide nodes' padded one-FMA slab test (csrc/slab_plane.h, expand_node)
against the CPU oracle, on rays chosen to sit on the decisions it takes.

The padded planes may only enter MORE children than the exact two-FMA planes
did; what a photon hits is decided at the leaves and must not move.  One batch
per geometry holds four sets of rays:

  (a) grazing: from fixed points, at the 8 corners, 12 edge midpoints and 6
      face centres of the reference leaf boxes of sampled triangles, each
      direction also with every component moved by +-1 ulp;
  (b) axis-parallel and near-parallel directions: one component ~1, the other
      two from the CPU test's sweep (0, denormal, smallest normal, 1e-33 ..
      1e-3, both signs) -- flat axes, wild axes (pad +inf: never culls, the
      NaN-skipping max/min chains) and ordinary tiny ones;
  (c) origins outside the world box, 2x..10x its size away, looking in;
  (d) 20,000 plain isotropic photons.

Each case is one propagate (max_steps 1 and 10) on the 2-PMT detector (90,912
triangles) and on demo.tiny(), through the step launches (trace_kernel, with
64 x 64 slots and > 8192 photons) and, with CHR_STEP_LAUNCH=0, through the
one-launch walkers that share expand_node.  The contract is test_gpu_parity's:
flags, last-hit triangles and evidx bit-exact, floats within 1e-5 relative, RNG
slot states equal; no stack overflow.  The oracle half is computed once per
(geometry, max_steps); on it, at least half of each of (a)-(c) must hit
geometry on the first step (checked on the CPU when the sets were chosen:
a set of NO_HITs would test nothing).
"""
import numpy as np
import pytest

import oracle
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

NTPB, MAX_BLOCKS = 64, 64
SWEEP = (0.0, 1e-45, 1e-40, 1.17549435e-38, 1e-33, 1e-30, 1e-20, 1e-10, 1e-3)


@pytest.fixture(scope='module')
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from chroma.gpu import create_cuda_context
    return create_cuda_context()


def _leaf_boxes(packed, tris):
    """(lo, hi) float64 (n, 3) of the reference leaf boxes of triangles `tris`."""
    nodes = packed.nodes
    leaf = (nodes[:, 3] >> 28) == 0
    of_tri = np.full(len(packed.triangles), -1, np.int64)
    of_tri[(nodes[leaf, 3] & 0x0FFFFFFF).astype(np.int64)] = np.flatnonzero(leaf)
    w = nodes[of_tri[tris], :3]
    assert (of_tri[tris] >= 0).all()
    wo, ws = packed.world_origin.astype(np.float64), float(packed.world_scale)
    return wo + (w & 0xFFFF) * ws, wo + (w >> 16) * ws


def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def _grazing(packed, r, ntri, origins):
    tris = r.choice(len(packed.triangles), ntri, replace=False)
    lo, hi = _leaf_boxes(packed, tris)
    # the 26 boundary points of a box with coordinates in {lo, mid, hi}, centre excluded
    sel = np.array([(i, j, k) for i in range(3) for j in range(3) for k in range(3) if (i, j, k) != (1, 1, 1)])
    grid = np.stack([lo, 0.5 * (lo + hi), hi], axis=1)            # (ntri, 3 levels, 3 axes)
    targets = np.stack([grid[:, sel[:, a], a] for a in range(3)], axis=2).reshape(-1, 3)
    o = origins[np.arange(len(targets)) % len(origins)]
    d = _unit(targets - o).astype(np.float32)
    out_o, out_d = [o], [d]
    for axis in range(3):
        for to in (np.float32(np.inf), np.float32(-np.inf)):
            n = d.copy()
            n[:, axis] = np.nextafter(d[:, axis], to)
            out_o.append(o)
            out_d.append(n)
    return np.concatenate(out_o), np.concatenate(out_d)


def _near_parallel(r, radius):
    vals = np.array(sorted(set(SWEEP) | set(-v for v in SWEEP)), np.float64)
    a, b = np.meshgrid(vals, vals, indexing='ij')
    a, b = a.ravel(), b.ravel()
    # a pair with a flat component (1/d not finite) goes with one of the six main
    # directions, the others with all six: the reference's walk of a flat ray enters
    # every box its projection crosses, milliseconds each on the oracle
    flat = (np.abs(a) < 1.17549435e-38) | (np.abs(b) < 1.17549435e-38)
    ds = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            keep = ~flat | (np.arange(len(a)) % 6 == len(ds))
            d = np.zeros((int(keep.sum()), 3))
            d[:, axis] = sign
            d[:, (axis + 1) % 3] = a[keep]
            d[:, (axis + 2) % 3] = b[keep]
            ds.append(_unit(d))
    d = np.concatenate(ds).astype(np.float32)
    o = _unit(r.normal(size=(len(d), 3))) * (radius * r.uniform(0.0, 1.0, (len(d), 1)) ** (1.0 / 3.0))
    return o, d


def _outside(packed, r, n, radius):
    wo = packed.world_origin.astype(np.float64)
    ext = 65535.0 * float(packed.world_scale)
    centre = wo + 0.5 * ext
    o = centre + _unit(r.normal(size=(n, 3))) * ext * r.uniform(2.0, 10.0, (n, 1))
    target = _unit(r.normal(size=(n, 3))) * (radius * r.uniform(0.0, 1.0, (n, 1)))
    return o, _unit(target - o).astype(np.float32)


def _photons(packed, radius, seed):
    """The batch and the index ranges of its sets.  radius: of the PMT sphere (rays
    start or aim inside it)."""
    from chroma.event import Photons
    from chroma.photon_source import isotropic
    r = np.random.RandomState(seed)
    origins = np.array([[0.0, 0.0, 0.0], [0.31 * radius, -0.17 * radius, 0.23 * radius],
                        [-0.45 * radius, 0.4 * radius, -0.1 * radius]])
    sets = [_grazing(packed, r, 40, origins), _near_parallel(r, 0.8 * radius), _outside(packed, r, 2000, 0.9 * radius)]
    iso = isotropic(20000, seed=seed)
    pos = np.concatenate([s[0] for s in sets] + [iso.pos]).astype(np.float32)
    d = np.concatenate([s[1] for s in sets] + [iso.dir]).astype(np.float32)
    pol = np.cross(d.astype(np.float64), r.normal(size=d.shape))
    pol = _unit(pol).astype(np.float32)
    pol[-len(iso):] = iso.pol
    bounds = np.cumsum([0] + [len(s[0]) for s in sets] + [len(iso)])
    ranges = {k: (int(bounds[i]), int(bounds[i + 1])) for i, k in enumerate('abcd')}
    wl = r.uniform(300.0, 600.0, len(pos)).astype(np.float32)
    return Photons(pos, d, pol, wl), ranges


_cache = {}


def _geometry(name):
    if name not in _cache:
        from chroma import demo, loader
        from chroma.gpu.packing import PackedGeometry
        geo = loader.create_geometry_from_obj(demo.detector(600.0, 900.0, 1500.0) if name == 'small' else demo.tiny())
        packed = PackedGeometry(geo)
        photons, ranges = _photons(packed, 600.0 if name == 'small' else 2000.0, 71 if name == 'small' else 72)
        _cache[name] = dict(geo=geo, packed=packed, photons=photons, ranges=ranges, gg=None, oracle={})
    return _cache[name]


def _oracle_side(name, max_steps):
    """The oracle's photons, RNG states and first-step hit fractions per set, once
    per (geometry, max_steps), never modified afterwards."""
    g = _geometry(name)
    photons = g['photons']
    if 'hit' not in g:
        _, tri = oracle.intersect_rays(g['packed'], photons.pos, photons.dir, np.full(len(photons), -1, np.int32))
        g['hit'] = {k: float((tri[a:b] >= 0).mean()) for k, (a, b) in g['ranges'].items()}
    hit = g['hit']
    if max_steps not in g['oracle']:
        host = oracle.HostPhotons(photons)
        st = oracle.rng_init(NTPB * MAX_BLOCKS, seed=7)
        stats = oracle.propagate(g['packed'], host, st, NTPB * MAX_BLOCKS, NTPB, MAX_BLOCKS, max_steps)
        g['oracle'][max_steps] = (host, st, stats, hit)
    return g['oracle'][max_steps]


@pytest.mark.parametrize('step_launch', ['1', '0'])
@pytest.mark.parametrize('max_steps', [1, 10])
@pytest.mark.parametrize('name', ['small', 'tiny'])
def test_padded_slab_parity(cuda, monkeypatch, name, max_steps, step_launch):
    from chroma import gpu
    g = _geometry(name)
    host, st, stats, hit = _oracle_side(name, max_steps)
    print('first-step hit fractions on the oracle:', hit)
    for k in 'abc':
        assert hit[k] >= 0.5, (k, hit)
    assert stats['overflows'] == 0
    assert len(g['photons']) >= NTPB * 128          # one launch per step: the split step, trace_kernel
    monkeypatch.setenv('CHR_STEP_LAUNCH', step_launch)
    if g['gg'] is None:
        g['gg'] = gpu.GPUGeometry(g['geo'])
    rng = gpu.get_rng_states(NTPB * MAX_BLOCKS, seed=7)
    gp = gpu.GPUPhotons(g['photons'])
    gp.propagate(g['gg'], rng, nthreads_per_block=NTPB, max_blocks=MAX_BLOCKS, max_steps=max_steps)
    _compare(host, gp, 'padded slab %s' % ((name, max_steps, step_launch),))
    assert np.array_equal(rng.get().reshape(-1), st), 'RNG slot states differ'
    assert gp.last_stats.stack_overflows == 0
    if step_launch == '1':
        assert gp.last_stats.trace_launches >= 1
    else:
        assert gp.last_stats.trace_launches == 0
