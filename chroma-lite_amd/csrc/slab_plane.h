// slab_plane.h -- the plane arithmetic of the slab test on 8-wide nodes, as plain
// inline functions that compile for host and device, so the kernels
// (propagate.hip: make_slab, expand_node) and the CPU test of the bound
// (tests/test_slab_pad.py, tests/slab_pad_check.cpp) run the same text.
//
// A wide node stores its children's planes as bytes q against a per-node origin
// `org` and a power-of-two quantum s = 2^e per axis (wide_bvh.h).  For a ray with
// per-axis multiplier m and offset c (m = 1/d and c = -o/d, or m = 2^100 and
// c = -o * 2^100 on a flat axis, make_slab) the distance to a plane is
//
//   two steps:  T  = fl(fl(q s + org) m + c)      slab_t2: the decode the builder
//                                                 checked, then the reference's fmaf
//   one step:   T' = fl(q S + O'),  S = fl(s m),  O' = fl(org m + c')   slab_t1
//
// with c' the offset moved outward by a pad eps: c' = fl(c - eps) for a near plane,
// fl(c + eps) for a far plane.  S and O' are the same for the 16 planes of a node
// and axis, so the one-step form costs one FMA per plane where the two-step form
// costs two.  It is used ONLY to decide which children of a wide node to enter:
// the claim proved here is
//
//   T'_near <= T_near   and   T'_far >= T_far                               (*)
//
// for every plane, hence max(T'_near.., 0) <= max(T_near.., 0) and
// min(T'_far..) >= min(T_far..): a child the two-step test enters, the one-step
// test enters too (both at the same cut, since its entry distance is not larger).
// A superset of boxes changes no result: what a photon hits is decided at the
// leaves, by the reference's own box test on the reference leaf box
// (intersect_box_slab, unpadded) and its decision rule.
//
// Proof of (*).  u = 2^-24.  fl() rounds to nearest, so |fl(y) - y| <= u |fl(y)|
// and <= u |y| while fl(y) is normal, and <= 2^-150 when it is subnormal.  W is a
// bound on |org| and on every decoded plane |q s + org| of the geometry
// (slab_world_bound; wide_validate refuses a tree with a plane beyond it).  Let
// x = q s + org (real), t = x m + c (real), M = |m| W + |c|.  slab_pad returns
// eps = max(fl(|m| W + |c|) * 2^-21, 2^-120) >= 8u (1 - u) M when that sum is
// <= 2^124, and +inf otherwise (the "wild" case, below).
//  - Nothing overflows: |x m| <= |m| W <= M, |c| <= M, s <= W (a quantum is not
//    larger than the world, same check), so |S| <= M and every intermediate is
//    below 2 (M + eps) < 2^126.  S = s m is exact (s is a power of two) unless it
//    is subnormal; then it is off by at most 2^-150 and q S by at most 2^-142.
//  - Two steps: p = fl(x) = x (1 + d1), T = fl(p m + c) = (p m + c)(1 + d2), so
//    |T - t| <= u |m| |x| + u |T|.
//  - One step, near plane: c' <= c - eps + u |c'|;  O' <= org m + c' + u |O'|;
//    T' <= q S + O' + u |T'|;  and q S + org m = x m.  Summed:
//    T' <= t - eps + u (|c'| + |O'| + |T'|).
//  - So T - T' >= eps - u (|m||x| + |T| + |c'| + |O'| + |T'|) - 2^-140 (the last
//    term covers every subnormal rounding above).  Each of the five magnitudes is
//    at most (M + eps)(1 + 5u): |m||x| <= M; |T| <= |t|(1 + 3u) <= M (1 + 3u);
//    |c'| <= (|c| + eps)(1 + u); |O'| <= (|m| W + |c'|)(1 + u);
//    |T'| <= (|t| + eps)(1 + 5u) (second order: the rounding errors of c' and O'
//    are themselves <= u (M + eps), which the factor 1 + 5u absorbs).  With
//    eps <= 8u (1 + u) M (or eps = 2^-120 > 8u M) this gives
//       u * 5 (M + eps)(1 + 5u) + 2^-140 <= 5u M (1 + 15u) + 2^-140  <  eps:
//    the gap 3u M (1 - 30u) exceeds 2^-140 once M >= 2^-99, and below that
//    eps = 2^-120 >= 5/8 * 2^-120 (1 + 15u) + 2^-140.  The far plane is the mirror image.
//    The pad is 8u M where 5u M is needed: 1.6x slack.  Without the pad the two
//    forms differ by at most u (|m||x| + |T| + |O| + |T'|) <= 4u M (1 + 5u) -- half
//    of eps, the figure the CPU test measures (limit 0.5).
//  - The clamp at 0 and the cut are monotone: max(.., 0) and min keep (*), and a
//    child is entered when !(tmin > tmax) & !(tmin > cut).
//  - Flat axis: m = 2^100, c = -o 2^100, both exact; the same formulas hold (only
//    the sign of T matters there, and (*) keeps a zero or negative near distance
//    <= 0 and a far one >= 0).
//  - Wild axis (the sum above 2^124, infinite or NaN: |d| under about 1e-32 on a
//    100 m world, or an origin astronomically far away): eps = +inf, so the near
//    offset c - inf is -inf (NaN when c = +inf) and the far offset +inf (NaN when
//    c = -inf).  Then O'_near and T'_near are -inf or NaN (S may be infinite;
//    0 * inf and inf - inf give NaN) and T'_far is +inf or NaN.  The max/min chains are
//    fmaxf/fminf (IEEE-754 maxNum/minNum: a NaN operand is ignored, the other
//    returned -- what v_max3_f32/v_min3_f32 do too), so such an axis never culls:
//    -inf loses every max, +inf every min, NaN is skipped, and with all three
//    axes NaN tmax is NaN and !(tmin > tmax) holds.  That NaN rule is the only
//    one relied on, and only for wild axes; elsewhere every value is finite.
//    The two-step test with the same inputs culls no less, so (*) holds in the
//    sense that matters (entered before => entered now).
#pragma once

#if defined(__HIPCC__)
#define CHR_SLAB_HD __host__ __device__ inline
#else
#define CHR_SLAB_HD inline
#endif

namespace chr {

// Largest absolute coordinate a decoded plane of a wide node may take: the world box
// of the reference's 16-bit quantisation ([origin, origin + 65535 scale], leaf margin
// of one quantum included since it is clamped to that range) widened by one world
// extent on each axis for the 8-bit planes, whose quantum can overshoot a child's
// bound.  wide_validate checks every node against it (slab_planes_within).
CHR_SLAB_HD float slab_world_bound(float ox, float oy, float oz, float scale) {
    const float ext = 65536.0f * scale;
    const float wx = __builtin_fmaxf(__builtin_fabsf(ox), __builtin_fabsf(ox + ext));
    const float wy = __builtin_fmaxf(__builtin_fabsf(oy), __builtin_fabsf(oy + ext));
    const float wz = __builtin_fmaxf(__builtin_fabsf(oz), __builtin_fabsf(oz + ext));
    return __builtin_fmaxf(__builtin_fmaxf(wx, wy), wz) + ext;
}
// one axis of one node inside the bound: origin, last plane and quantum
CHR_SLAB_HD bool slab_planes_within(float org, float s, float W) {
    return __builtin_fabsf(org) <= W && __builtin_fabsf(__builtin_fmaf(255.0f, s, org)) <= W && s <= W;
}

CHR_SLAB_HD bool slab_finite(float x) { return __builtin_fabsf(x) <= 3.4028235e38f; }   // false for NaN
constexpr float SLAB_FLAT_MULT = 1.2676506e30f;   // 2^100

// multiplier and exact offset of one axis (inv = 1/d, noid = -o/d): the reference's,
// or the flat axis's test of the constant coordinate o (propagate.hip, RaySlab)
CHR_SLAB_HD float slab_mult(float inv) { return slab_finite(inv) ? inv : SLAB_FLAT_MULT; }
CHR_SLAB_HD float slab_off(float o, float noid, float inv) { return slab_finite(inv) ? noid : -(o * SLAB_FLAT_MULT); }

// the pad eps of one axis (+inf: wild, the axis never culls)
CHR_SLAB_HD float slab_pad(float mult, float off, float W) {
    const float M = __builtin_fmaf(__builtin_fabsf(mult), W, __builtin_fabsf(off));
    return M <= 0x1p124f ? __builtin_fmaxf(M * 0x1p-21f, 0x1p-120f) : __builtin_inff();   // NaN: +inf
}
CHR_SLAB_HD float slab_near_off(float off, float eps) { return off - eps; }
CHR_SLAB_HD float slab_far_off(float off, float eps) { return off + eps; }

// per node and axis
CHR_SLAB_HD float slab_scale(float s, float mult) { return s * mult; }                                       // S
CHR_SLAB_HD float slab_origin(float org, float mult, float poff) { return __builtin_fmaf(org, mult, poff); }   // O'
// per plane
CHR_SLAB_HD float slab_t1(float q, float S, float O) { return __builtin_fmaf(q, S, O); }
CHR_SLAB_HD float slab_t2(float q, float s, float org, float mult, float off) {
    return __builtin_fmaf(__builtin_fmaf(q, s, org), mult, off);
}

}  // namespace chr
