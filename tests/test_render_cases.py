"""The renderer cases of render_cases.py meet their conditions -- on the CPU
oracle (orc_render) and the host model of render_kernel's stack alone, so the
device tests of test_gpu_render.py that use them test what they are there for:

  * R1-R4 hold, in at least 100 rays each, two adjacent entries of equal
    distance with different colour quadruples (the order under equal distance
    -- the rank column of render_kernel -- shows in the result);
  * R1 at depth 3 and R6 at depth 10 fill at least 100 lists (entries fall off);
  * R5 (direction 0) hits nothing;
  * a second pass over R1 with the lists kept doubles every distance and drops
    entries of the longest lists;
  * every ray of R6 holds at least RENDER_LDS + 2 stack entries at some point
    of the model's walk (two entries of margin for the model's float64 plane
    distances against the kernel's float32 ones), and under the same model no
    ray of the views test_gpu_render.py had before holds more than RENDER_LDS:
    R6 is what runs the private half of the kernel's stack."""
import numpy as np
import pytest

import oracle
import render_cases as rc
from scenes import camera_rays
from test_gpu_render import _colors

BG = 0x80FFFFFF


def _geometry(scene):
    return {'T': rc.scene_T, 'S': rc.scene_S}[scene]()


def _render(name, depth, **kept):
    scene = rc.CASES[name][0]
    pos, d = rc.rays(name)
    return oracle.render(rc.packed(scene), pos, d, _colors(_geometry(scene), True), depth, bg_color=BG, **kept)


def test_scenes():
    from chroma.bvh.wide import build_wide_bvh
    assert len(rc.packed('T').triangles) == 48
    assert len(rc.packed('S').triangles) == 2560
    wb = build_wide_bvh(rc.packed('S'))
    assert wb.usable and wb.max_depth >= 3


def test_ray_counts_are_ragged():
    """No ray set of the new cases fills its last workgroup (BLOCK = 256)."""
    for name in rc.CASES:
        pos, d = rc.rays(name)
        assert pos.shape == d.shape and pos.dtype == d.dtype == np.float32
        assert len(pos) % 256 != 0
    assert len(rc.rays('R1')[0]) == 5 * 256 + 220


def test_flat_axes():
    """R2 and R3 have zero direction components (1/d infinite), R2 also origin
    coordinates exactly 0 on such an axis (-o/d NaN) and rays lying in the
    planes y, z = +-500 of the cubes' faces."""
    pos, d = rc.rays('R2')
    assert (d[:, 1:] == 0).all() and ((pos[:, 1] == 0) | (pos[:, 2] == 0)).sum() > 30
    assert ((np.abs(pos[:, 1]) == 500) | (np.abs(pos[:, 2]) == 500)).sum() > 30
    with np.errstate(divide='ignore', invalid='ignore'):
        assert np.isnan(-pos / d).any()
    _, dz = rc.rays('R2z')
    assert np.array_equal(d, dz) and np.signbit(dz[:, 1]).all() and not np.signbit(d[:, 1]).any()
    _, d3 = rc.rays('R3')
    assert (d3[:, 2] == 0).all() and (d3[:, :2] != 0).all()
    assert (rc.rays('R5')[1] == 0).all()


@pytest.mark.parametrize('name', rc.TIE_CASES)
def test_equal_distance_pairs(name):
    for depth in rc.CASES[name][2]:
        _, dx, dxlen, col = _render(name, depth)
        assert len(rc.tie_rays(dx, dxlen, col, depth)) >= 100, depth


def test_full_lists():
    for name, depth in (('R1', 3), ('R6', 10)):
        dxlen = _render(name, depth)[2]
        assert (dxlen == depth).sum() >= 100, name


def test_zero_direction_hits_nothing():
    pix, _, dxlen, _ = _render('R5', 4)
    assert not dxlen.any() and (pix == BG).all()


def test_second_pass_doubles_and_drops():
    depth = 10
    _, dx, dxlen, col = _render('R1', depth)
    first, n1 = dx.reshape(-1, depth).copy(), dxlen.copy()
    assert n1.max() == 6
    _, dx, dxlen, col = _render('R1', depth, dx=dx, dxlen=dxlen, color=col)
    dx = dx.reshape(-1, depth)
    for i in np.flatnonzero(n1):
        assert dxlen[i] == min(depth, 2 * n1[i])
        assert np.array_equal(dx[i, :dxlen[i]], np.repeat(first[i, :n1[i]], 2)[:dxlen[i]])
    assert (2 * n1 > depth).any()


def test_render_lds_copy_is_current():
    assert rc.RENDER_LDS == rc.render_lds_in_source(), 'render_cases.RENDER_LDS is stale'


def test_stack_passes_lds_half_only_in_R6(cube_geometry, small_packed):
    from chroma.bvh.wide import build_wide_bvh
    from chroma.gpu.packing import PackedGeometry
    high = rc.stack_high_water(build_wide_bvh(rc.packed('S')).nodes, *rc.rays('R6'))
    assert high.min() >= rc.RENDER_LDS + 2
    assert high.max() <= rc.WIDE_STACK
    # the views test_render_parity and test_snapshot_and_transforms render, first pass and rotated
    axis = np.array([0.0, 0.0, 1.0], np.float32)
    # (every ray; the 2-PMT detector reaches 13 entries, 15 with the rays rotated)
    for p, eye in ((PackedGeometry(cube_geometry), (2500.0, -3000.0, 1200.0)),
                   (small_packed, (1800.0, -2400.0, 700.0))):
        nodes = build_wide_bvh(p).nodes
        pos, d = camera_rays(96, 64, eye, (0.0, 0.0, 0.0))
        assert rc.stack_high_water(nodes, pos, d).max() <= rc.RENDER_LDS
        pos2 = oracle.transform(pos, 2, phi=0.05, axis=axis, v=(0.0, 0.0, 0.0))
        d2 = oracle.transform(d, 1, phi=0.05, axis=axis)
        assert rc.stack_high_water(nodes, pos2, d2).max() <= rc.RENDER_LDS
    # and the tie cases: their scene is a root and seven leaves' worth of nodes
    nodes = build_wide_bvh(rc.packed('T')).nodes
    for name in rc.TIE_CASES + ('R5',):
        assert rc.stack_high_water(nodes, *rc.rays(name)).max() <= rc.RENDER_LDS
