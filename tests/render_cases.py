"""Scenes, ray sets and a host model of render_kernel's stack for the renderer
cases the camera views of test_gpu_render.py never reach: entries of equal
distance (coincident faces), rays with a zero direction component, ray counts
that are no multiple of the workgroup, and a walk whose stack goes past the
LDS half (csrc/render.hip RENDER_LDS).

tests/test_render_cases.py proves on the oracle and the model that each case
meets its condition; tests/test_gpu_render.py runs them on the device."""
import functools
import os
import re

import numpy as np

from conftest import ROOT
from scenes import camera_rays, materials

RENDER_LDS = 16     # csrc/render.hip (render_lds_in_source reads the source's value)
WIDE_STACK = 128    # csrc/wide_bvh.h
FLAT_MULT = 2.0 ** 100   # csrc/slab_plane.h SLAB_FLAT_MULT
FLT_MAX = 3.4028235e38


def render_lds_in_source():
    text = open(os.path.join(ROOT, 'chroma-lite_amd', 'csrc', 'render.hip')).read()
    m = re.search(r'constexpr\s+int\s+RENDER_LDS\s*=\s*(\d+)\s*;', text)
    assert m, 'RENDER_LDS not found in csrc/render.hip'
    return int(m.group(1))


# ---------------------------------------------------------------- scenes
def _detector(parts):
    from chroma import loader
    from chroma.detector import Detector
    from chroma.geometry import Solid
    m = materials()
    det = Detector(m['water'])
    for mesh, rotation, displacement in parts:
        det.add_solid(Solid(mesh, m['glass'], m['water']), rotation=rotation, displacement=displacement)
    return loader.create_geometry_from_obj(det)


@functools.lru_cache(maxsize=None)
def scene_T():
    """Coincident faces: the same cube twice, and a box whose -x face lies in
    the cubes' x = 500 plane.  48 triangles."""
    from chroma import make
    return _detector([(make.cube(1000.0), None, None), (make.cube(1000.0), None, None),
                      (make.box(400.0, 400.0, 400.0), None, (700.0, 0.0, 0.0))])


@functools.lru_cache(maxsize=None)
def scene_S():
    """A sheaf of 160 thin sticks through the origin: every stick's box overlaps
    every other's near the centre, so an unpruned walk towards the centre holds
    many pending nodes at once.  2560 triangles."""
    from chroma import make
    from chroma.transform import make_rotation_matrix
    rng = np.random.default_rng(5)
    parts = []
    for _ in range(160):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        parts.append((make.box(2000.0, 20.0, 20.0), make_rotation_matrix(rng.uniform(0.0, np.pi), axis), None))
    return _detector(parts)


@functools.lru_cache(maxsize=None)
def packed(scene):
    from chroma.gpu.packing import PackedGeometry
    return PackedGeometry({'T': scene_T, 'S': scene_S}[scene]())


# ---------------------------------------------------------------- ray sets
def _grid():
    y, z = np.meshgrid(np.linspace(-600.0, 600.0, 25), np.linspace(-600.0, 600.0, 13))
    return y.reshape(-1), z.reshape(-1)


def _r2_origins():
    y, z = _grid()
    return np.column_stack((np.full(len(y), 2000.0), y, z)).astype(np.float32)


def _const_dir(n, d):
    return np.tile(np.asarray(d, np.float32), (n, 1))


def _r1():
    return camera_rays(50, 30, (2500.0, -3000.0, 1200.0), (0.0, 0.0, 0.0))


def _r2():
    pos = _r2_origins()
    return pos, _const_dir(len(pos), (-1.0, 0.0, 0.0))


def _r2_negzero():
    pos = _r2_origins()
    d = _const_dir(len(pos), (-1.0, -0.0, 0.0))
    assert np.signbit(d[:, 1]).all()
    return pos, d


def _r3():
    u, v = _grid()
    pos = (np.array([1500.0, -2000.0, 0.0]) + u[:, None] * np.array([0.8, 0.6, 0.0])
           + v[:, None] * np.array([0.0, 0.0, 1.0]))
    return pos.astype(np.float32), _const_dir(len(pos), (-0.6, 0.8, 0.0))


def _r4():
    return camera_rays(50, 30, (100.0, 50.0, 20.0), (900.0, 0.0, 0.0), fov_deg=90.0)


def _r5():
    pos = _r2_origins()
    return pos, _const_dir(len(pos), (0.0, 0.0, 0.0))


def _r6():
    return camera_rays(20, 15, (1500.0, -1800.0, 700.0), (0.0, 0.0, 0.0), fov_deg=10.0)


# name: (scene, rays, alpha depths)
CASES = {
    'R1': ('T', _r1, (3, 10)),          # oblique camera; 1500 rays = 5 workgroups + 220
    'R2': ('T', _r2, (10,)),            # along -x: two flat axes, origins with y or z exactly 0
    'R2z': ('T', _r2_negzero, (10,)),   # the same with dir.y = -0.0
    'R3': ('T', _r3, (10,)),            # one flat axis, the other two oblique
    'R4': ('T', _r4, (10,)),            # origin inside both cubes
    'R5': ('T', _r5, (4,)),             # direction (0, 0, 0): no hit anywhere
    'R6': ('S', _r6, (1, 10)),          # stack past RENDER_LDS
}
CASE_DEPTHS = [(name, depth) for name, (_, _, depths) in CASES.items() for depth in depths]
TIE_CASES = ('R1', 'R2', 'R2z', 'R3', 'R4')


def rays(name):
    pos, d = CASES[name][1]()
    return pos, d


def tie_rays(dx, dxlen, color, depth):
    """Rays whose list holds two adjacent entries of equal distance and
    different colour quadruples: their order shows in the colour column."""
    n = len(dxlen)
    dx = dx.reshape(n, depth)
    col = color.reshape(n, depth, 4).view(np.uint32)
    k = np.arange(depth - 1)[None, :]
    pair = (dx[:, :-1] == dx[:, 1:]) & (k + 1 < dxlen[:, None]) & (col[:, :-1] != col[:, 1:]).any(axis=2)
    return np.flatnonzero(pair.any(axis=1))


# ---------------------------------------------------------------- host model of the stack
def _fma32(q, s, o):
    """float32 fmaf(q, s, o) for small-integer q (exact in long double, one rounding)."""
    return (np.asarray(q, np.longdouble) * np.asarray(s, np.longdouble) + np.asarray(o, np.longdouble)).astype(np.float32)


def stack_high_water(nodes, pos, d):
    """Largest number of stack entries render_kernel's walk holds, per ray.

    A restatement of its loop over the wide nodes (chroma.bvh.wide
    build_wide_bvh(packed).nodes): child boxes decoded as the kernel decodes
    them, fmaf(q, 2^(e-127), origin) in float32; the slab constants of
    make_slab (1/d and -o/d in float32; multiplier 2^100 and offset -o 2^100
    on an axis whose 1/d is not finite); the near and far planes picked by the
    sign of 1/d; tmin = max(near.., 0) > tmax = min(far..) culls; a node's
    inner children that pass are pushed in child order and one entry is popped
    per node.  The plane distances are in float64 where the kernel's are one
    float32 fmaf: enough for a count, which test_render_cases takes with two
    entries of margin.  Leaves push nothing and are left out."""
    from chroma.bvh.wide import WIDE_INNER
    scale = (nodes['exp'].astype(np.uint32) << 23).view(np.float32)          # (N, 3)
    lo = _fma32(nodes['qlo'], scale[:, :, None], nodes['origin'][:, :, None]).astype(np.float64)   # (N, 3, 8)
    hi = _fma32(nodes['qhi'], scale[:, :, None], nodes['origin'][:, :, None]).astype(np.float64)
    inner = nodes['kind'] == WIDE_INNER                                       # (N, 8)
    child = nodes['child_base'][:, None].astype(np.int64) + nodes['off']     # (N, 8)
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    with np.errstate(divide='ignore', invalid='ignore'):
        inv = np.float32(1.0) / d
        noid = -pos / d
    finite = np.abs(inv) <= np.float32(FLT_MAX)                               # false for NaN
    mult = np.where(finite, inv.astype(np.float64), FLAT_MULT)[:, :, None]   # (R, 3, 1)
    off = np.where(finite, noid.astype(np.float64), -(pos.astype(np.float64) * FLAT_MULT))[:, :, None]
    neg = (finite & (inv < 0))[:, :, None]
    nrays = len(pos)
    stack = np.zeros((nrays, WIDE_STACK), np.int64)
    sp = np.zeros(nrays, np.int64)
    high = np.zeros(nrays, np.int64)
    node = np.zeros(nrays, np.int64)
    live = np.arange(nrays) if len(nodes) else np.zeros(0, np.int64)
    while len(live):
        nd = node[live]
        near = np.where(neg[live], hi[nd], lo[nd]) * mult[live] + off[live]  # (L, 3, 8)
        far = np.where(neg[live], lo[nd], hi[nd]) * mult[live] + off[live]
        tmin = np.fmax(np.fmax(np.fmax(near[:, 0], near[:, 1]), near[:, 2]), 0.0)
        tmax = np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2])
        push = inner[nd] & ~(tmin > tmax)                                     # (L, 8)
        for k in range(8):
            w = live[push[:, k] & (sp[live] < WIDE_STACK)]
            stack[w, sp[w]] = child[node[w], k]
            sp[w] += 1
        high[live] = np.maximum(high[live], sp[live])
        live = live[sp[live] > 0]
        sp[live] -= 1
        node[live] = stack[live, sp[live]]
    return high
