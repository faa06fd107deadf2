// walk_ref.h -- intersect_mesh: the exact-order walk of the reference BVH (mesh.h), the
// walk every other walker is checked against.  It knows the geometry and a ray, and
// nothing of photons, PropagateArgs or queues.
#pragma once
#include "photon_state.h"

namespace chr {

// mesh.h:45-126 -- nearest triangle != last_hit; reference DFS order.
// The children of a popped group are fetched BATCH at a time (independent
// 16-byte loads in flight together), their slab tests computed up front, and
// then walked strictly in index order with the reference's prune / accept /
// push decisions, so the result (including tie-breaking) is unchanged.
template <int BATCH>
__device__ __forceinline__ int intersect_mesh(const DevGeom &g, V3 o, V3 d, float &min_distance, int last_hit,
                                              Stack st, uint32_t &overflow) {
    uint32_t spill[STACK_SIZE - STACK_LDS];
    int triangle_index = -1;
    min_distance = -1.0f;
    const V3 noid = v3(-o.x / d.x, -o.y / d.y, -o.z / d.z);
    const V3 inv = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    const uint4 root = gld(g.nodes);
    {
        V3 lo, hi;
        float bd;
        node_bounds(g, root, lo, hi);
        if (!intersect_box(noid, inv, lo, hi, bd)) return -1;
    }
    stack_put(st, spill, 0, root.w);
    int curr = 0;
    const uint32_t last = (uint32_t)last_hit;
    while (curr >= 0) {
        const uint32_t w = stack_get(st, spill, curr);
        curr--;
        const uint32_t end = (w & 0x0FFFFFFFu) + (w >> 28);
        for (uint32_t i = w & 0x0FFFFFFFu; i < end; i += BATCH) {
            uint4 nd[BATCH];
#pragma unroll
            for (int k = 0; k < BATCH; ++k)
                if (i + k < end) nd[k] = gld(g.nodes + i + k);
            float bd[BATCH];
            bool hit[BATCH];
#pragma unroll
            for (int k = 0; k < BATCH; ++k) {
                V3 lo, hi;
                node_bounds(g, nd[k], lo, hi);
                hit[k] = (i + k < end) && intersect_box(noid, inv, lo, hi, bd[k]);
            }
#pragma unroll
            for (int k = 0; k < BATCH; ++k) {
                if (!hit[k]) continue;
                if (min_distance >= 0.0f && bd[k] > min_distance) continue;
                const uint32_t child = nd[k].w & 0x0FFFFFFFu;
                if ((nd[k].w >> 28) == 0) {
                    if (child != last) {
                        const float4 *r = g.tri + 3 * (size_t)child;
                        const float4 r0 = gld(r), r1 = gld(r + 1), r2 = gld(r + 2);
                        float dist;
                        if (intersect_triangle(o, d, v3(r0.x, r0.y, r0.z), v3(r0.w, r1.x, r1.y), v3(r1.z, r1.w, r2.x),
                                               dist)) {
                            if (triangle_index == -1 || dist < min_distance) {
                                triangle_index = (int)child;
                                min_distance = dist;
                            }
                        }
                    }
                } else {
                    if (curr + 1 >= STACK_SIZE) {
                        overflow++;
                        return triangle_index;
                    }
                    curr++;
                    stack_put(st, spill, curr, nd[k].w);
                }
            }
        }
    }
    return triangle_index;
}

}  // namespace chr
