// photon_state.h -- what every device function of the propagate translation unit shares: the
// constants, Photon / State, the reference walk's LDS stack, global loads (gld), the
// top-of-tree LDS copy, the property tables and the box / triangle / record tests.
// It knows no walker, no physics and no kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/chroma_amd.h"
#include "../../include/chroma_fmath.h"
#include "common.h"
#include "device_geometry.h"
#include "device_math.h"
#include "wide_bvh.h"

namespace chr {

constexpr int BLOCK = 256;
constexpr int STACK_SIZE = 1000;   // mesh.h:10
constexpr int STACK_LDS = 24;      // entries kept in LDS per work-item
constexpr uint32_t DEAD_MASK = CHR_NO_HIT | CHR_BULK_ABSORB | CHR_SURFACE_DETECT | CHR_SURFACE_ABSORB | CHR_NAN_ABORT;
constexpr float WEIGHT_LOWER_THRESHOLD = 0.0001f;
constexpr float SPEED_OF_LIGHT = 299.792458f;
// float thresholds equivalent to the reference's float-vs-double compares
// (intersect.h:259-267): (double)u < -1e-6, (double)u > 1+1e-6, (double)t > 1e-6
constexpr float T_NEG_EPS = -9.99999997e-07f;
constexpr float T_ONE_EPS = 1.00000095367431640625f;
constexpr float T_POS_EPS = 9.99999997e-07f;

enum { BREAK = 0, CONTINUE = 1, PASS = 2 };

struct Photon {
    V3 pos, dir, pol;
    float wavelength, time, weight;
    uint32_t history;   // holds a 16-bit value (photon.h:29)
    int last_hit;
};

struct State {
    V3 normal;
    float n1, n2, absorption_length, scattering_length, distance;
    int material1, surface_index;
    bool inside_to_outside;   // photon.h:38 (the hybrid renderer reads it)
};

#define CHR_LDS __attribute__((address_space(3)))
#define CHR_COLD __forceinline__
// The LDS column pointer travels as a plain value (never inside an object that
// also holds the scratch spill array: such an object lives in scratch and its
// LDS pointer degrades to flat loads/stores).
struct Stack {
    CHR_LDS uint32_t *lds;   // this work-item's column: entry i at lds[i * BLOCK]
};

__device__ __forceinline__ void stack_put(const Stack &s, uint32_t *spill, int i, uint32_t v) {
    if (i < STACK_LDS) s.lds[i * BLOCK] = v;
    else spill[i - STACK_LDS] = v;
}
__device__ __forceinline__ uint32_t stack_get(const Stack &s, const uint32_t *spill, int i) {
    return (i < STACK_LDS) ? s.lds[i * BLOCK] : spill[i - STACK_LDS];
}

// Loads through pointers fetched from the device-resident DevGeom are flat
// (generic) loads unless the address space is stated; flat loads also count in
// lgkmcnt and so serialise against the LDS stack.  gld() = global_load.
#define CHR_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ T gld(const T *p) { return *(const CHR_GLOBAL T *)p; }
typedef uint32_t chr_u32x4 __attribute__((ext_vector_type(4)));
typedef float chr_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 gld(const uint4 *p) {
    const chr_u32x4 v = *(const CHR_GLOBAL chr_u32x4 *)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float4 gld(const float4 *p) {
    const chr_f32x4 v = *(const CHR_GLOBAL chr_f32x4 *)p;
    return make_float4(v.x, v.y, v.z, v.w);
}
typedef uint32_t chr_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 gld_lo2(const void *p) {   // the first 8 bytes at p (global_load_dwordx2)
    const chr_u32x2 v = *(const CHR_GLOBAL chr_u32x2 *)p;
    return make_uint2(v.x, v.y);
}

// ---------------------------------------------------------------- geometry.h
// The top of the wide BVH in LDS (north_star: "BVH nodes ... staged through
// LDS").  The builder numbers nodes level by level (wide_bvh.cpp), so nodes
// [0, TOP_NODES) are the root and the two levels below it of the 8-wide tree:
// every walk starts there and re-enters them from its stack.  A workgroup copies
// them once (96 B each: the node without its slot pad); a walk reads node i < n
// from LDS, every other node from global memory.  Same bytes, same results.
constexpr uint32_t TOP_NODES = 73;   // 1 + 8 + 64: 7,008 B
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // (HIP's uint4 has no LDS assignment)
struct TopNodes {
    const CHR_LDS u32x4 *p;          // 6 x 16 B per node
    uint32_t n;                      // nodes held (0: none)
};
template <int TB>
__device__ __forceinline__ TopNodes stage_top(const DevGeom &g, CHR_LDS u32x4 *lds, uint32_t want) {
    const uint32_t n = want < g.nwnodes ? want : g.nwnodes;   // workgroup-uniform
    for (uint32_t i = threadIdx.x; i < 6u * n; i += TB) {
        const uint4 v = gld(g.wnodes + (size_t)g.wstride * (i / 6u) + i % 6u);
        u32x4 w;
        w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
        lds[i] = w;
    }
    __syncthreads();
    return TopNodes{lds, n};
}
__device__ __forceinline__ uint4 u4(u32x4 v) { return make_uint4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void load_node(const DevGeom &g, const TopNodes &top, uint32_t node, uint4 &h, uint4 &a1,
                                          uint4 &a2, uint4 &a3, uint4 &a4, uint4 &a5) {
    if (node < top.n) {
        const CHR_LDS u32x4 *tp = top.p + 6u * node;
        h = u4(tp[0]); a1 = u4(tp[1]); a2 = u4(tp[2]); a3 = u4(tp[3]); a4 = u4(tp[4]); a5 = u4(tp[5]);
    } else {
        const uint4 *np = g.wnodes + (size_t)g.wstride * node;
        h = gld(np); a1 = gld(np + 1); a2 = gld(np + 2); a3 = gld(np + 3); a4 = gld(np + 4); a5 = gld(np + 5);
    }
}

__device__ __forceinline__ void node_bounds(const DevGeom &g, uint4 n, V3 &lo, V3 &hi) {
    lo = v3(__builtin_fmaf((float)(n.x & 0xFFFFu), g.scale, g.ox), __builtin_fmaf((float)(n.y & 0xFFFFu), g.scale, g.oy),
            __builtin_fmaf((float)(n.z & 0xFFFFu), g.scale, g.oz));
    hi = v3(__builtin_fmaf((float)(n.x >> 16), g.scale, g.ox), __builtin_fmaf((float)(n.y >> 16), g.scale, g.oy),
            __builtin_fmaf((float)(n.z >> 16), g.scale, g.oz));
}

// a table word: from LDS when the tables were copied there (phys_cache), else a global load
__device__ __forceinline__ float tab(const float *p) {
    return __builtin_amdgcn_is_shared((const __attribute__((address_space(0))) void *)p) ? *(const CHR_LDS float *)p
                                                                                         : gld(p);
}
__device__ __forceinline__ float interp_property(const DevGeom &g, float x, const float *fp) {
    const float start = g.wl_start, step = g.wl_step;
    const int n = (int)g.wl_n;
    if (x < start) return tab(fp);
    if (x > __builtin_fmaf((float)(n - 1), step, start)) return tab(fp + n - 1);
    const int jl = (int)((x - start) / step);
    const float base = __builtin_fmaf((float)jl, step, start);
    const float f0 = tab(fp + jl), f1 = tab(fp + jl + 1);
    return f0 + ((x - base) * (f1 - f0)) / step;
}

// ---------------------------------------------------------------- intersect.h / mesh.h
__device__ __forceinline__ bool intersect_box(V3 noid, V3 inv, V3 lo, V3 hi, float &dist) {
    float tmin = 0.0f, tmax = __builtin_inff();
    if (chr_isfinite(inv.x)) {
        const float t0 = __builtin_fmaf(lo.x, inv.x, noid.x), t1 = __builtin_fmaf(hi.x, inv.x, noid.x);
        tmin = fmax_(tmin, fmin_(t0, t1)); tmax = fmin_(tmax, fmax_(t0, t1));
    }
    if (chr_isfinite(inv.y)) {
        const float t0 = __builtin_fmaf(lo.y, inv.y, noid.y), t1 = __builtin_fmaf(hi.y, inv.y, noid.y);
        tmin = fmax_(tmin, fmin_(t0, t1)); tmax = fmin_(tmax, fmax_(t0, t1));
    }
    if (chr_isfinite(inv.z)) {
        const float t0 = __builtin_fmaf(lo.z, inv.z, noid.z), t1 = __builtin_fmaf(hi.z, inv.z, noid.z);
        tmin = fmax_(tmin, fmin_(t0, t1)); tmax = fmin_(tmax, fmax_(t0, t1));
    }
    if (tmin > tmax) return false;
    dist = tmin;
    return true;
}

// Moller-Trumbore on a de-indexed record (v0, e1, e2)
__device__ __forceinline__ bool intersect_triangle(V3 o, V3 d, V3 v0, V3 e1, V3 e2, float &distance) {
    const V3 h = cross(d, e2);
    const float a = dot(e1, h);
    if (a > -1.19209290e-7f && a < 1.19209290e-7f) return false;
    const float f = 1.0f / a;
    const V3 s = o - v0;
    const float u = f * dot(s, h);
    if (u < T_NEG_EPS || u > T_ONE_EPS) return false;
    const V3 q = cross(s, e1);
    const float v = f * dot(d, q);
    if (v < T_NEG_EPS || u + v > T_ONE_EPS) return false;
    const float t = f * dot(e2, q);
    if (t > T_POS_EPS && t < __builtin_inff()) {
        distance = t;
        return true;
    }
    return false;
}

// Moller-Trumbore on a wide-BVH triangle record (wide_bvh.h: v0, v1, v2 in
// r0..r2): the edges v1-v0, v2-v0 are the reference's own float subtractions
// (intersect.h:26-101), so this is intersect_triangle on the same operands.
__device__ __forceinline__ bool intersect_record(V3 o, V3 d, float4 r0, float4 r1, float4 r2, float &distance) {
    const V3 v0 = v3(r0.x, r0.y, r0.z), v1 = v3(r0.w, r1.x, r1.y), v2 = v3(r1.z, r1.w, r2.x);
    return intersect_triangle(o, d, v0, v1 - v0, v2 - v0, distance);
}
// the record index of a wide-BVH triangle record pointer: what the wide walks
// return for a hit (finish_fill<true> reads the triangle id and normal from it)
__device__ __forceinline__ int rec_of(const DevGeom &g, const float4 *r) { return (int)((r - g.wtri) >> 2); }

}  // namespace chr
