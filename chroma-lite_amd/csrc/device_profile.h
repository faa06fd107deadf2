// device_profile.h -- the device region profile and the photon / ray watch of
// libchroma_amd_prof.so (-DCHR_DEVICE_PROFILE=1): Prof, Watch, CHR_WEV, LoneProf and
// LongProf, each with the empty form every other build compiles, and the entry points
// that read them back (host code, at the end).  It knows State and the region ids of
// chroma_amd.h, and nothing of the kernels that carry the probes.
#pragma once
#include "photon_state.h"

namespace chr {

// ---------------------------------------------------------------- device profile
// The reference's CHROMA_DEVICE_PROFILE regions (profile.h:9-37: per-call
// clock64 spans atomically added to per-region counters) for the split step
// kernels, built only into libchroma_amd_prof.so (-DCHR_DEVICE_PROFILE=1).
// Instead of two global atomics per call, each work-item keeps its region
// lane-cycles and calls in registers and a wave adds its sums once at exit.
// A kernel marks region boundaries with tick(next): the wave time since the
// last tick goes to the region the work-item was in (a work-item masked off in
// a branch keeps its region, so the time it waits is charged there).
#ifdef CHR_DEVICE_PROFILE
__device__ unsigned long long chr_prof_calls[CHR_PROF_COUNT];
__device__ unsigned long long chr_prof_cycles[CHR_PROF_COUNT];

// one wave's sum of (calls, cycles) added to region id; every lane of the wave active
__device__ __forceinline__ void prof_add(int id, unsigned long long calls, unsigned long long cycles) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        calls += __shfl_xor(calls, o);
        cycles += __shfl_xor(cycles, o);
    }
    if (__lane_id() == 0) {
        if (calls) atomicAdd(&chr_prof_calls[id], calls);
        if (cycles) atomicAdd(&chr_prof_cycles[id], cycles);
    }
}
template <int N>
struct Prof {
    uint32_t cyc[N], calls[N];
    unsigned long long t, t0;
    int cur;
    __device__ __forceinline__ void start(int c) {
        t0 = t = __builtin_amdgcn_s_memtime();
        cur = c;
#pragma unroll
        for (int i = 0; i < N; ++i) cyc[i] = calls[i] = 0u;
    }
    __device__ __forceinline__ void tick(int next) {
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        const uint32_t dt = (uint32_t)(now - t);
        t = now;
#pragma unroll
        for (int i = 0; i < N; ++i) cyc[i] += cur == i ? dt : 0u;
        cur = next;
    }
    __device__ __forceinline__ void set(int c) { cur = c; }
    __device__ __forceinline__ void call(int i, uint32_t k = 1u) { calls[i] += k; }
    __device__ __forceinline__ unsigned long long total() const { return t - t0; }
};
#else
template <int N>
struct Prof {
    __device__ __forceinline__ void start(int) {}
    __device__ __forceinline__ void tick(int) {}
    __device__ __forceinline__ void set(int) {}
    __device__ __forceinline__ void call(int, uint32_t = 1u) {}
};
#endif

// Photon watch (profile build only, chr_watch_set / chr_watch_fetch): every step
// of one photon (its index in one batch's arrays) recorded by the kernel that ran
// it, in the layout of the oracle's orc_set_watch, so a parity mismatch can be
// followed step by step on both sides.  Words: kind (1 shade, 2 tail), queue
// position, hit triangle (-1: none), walk distance, pos in (3), dir in (3), last
// hit in, material1, absorption length, scattering length, pos out (3), history
// out, time out, RNG slot.
#ifdef CHR_DEVICE_PROFILE
constexpr uint32_t CHR_WATCH_WORDS = 20, CHR_WATCH_MAX = 4096;
__device__ uint32_t chr_watch_pid = 0xFFFFFFFFu;
__device__ unsigned long long chr_watch_array = 0ull;   // the batch's pos array (0: any batch)
__device__ uint32_t chr_watch_n = 0u;
__device__ uint32_t chr_watch_buf[CHR_WATCH_MAX * CHR_WATCH_WORDS];
struct Watch {
    uint32_t w[CHR_WATCH_WORDS];
    bool on;
    __device__ __forceinline__ void begin(uint32_t kind, uint32_t pid, const float *pos_array, uint32_t q,
                                          uint32_t slot, V3 pos, V3 dir, int last_in) {
        on = chr_watch_pid != 0xFFFFFFFFu && pid == chr_watch_pid && (chr_watch_array == 0ull || chr_watch_array == (unsigned long long)pos_array);
        if (!on) return;
        w[0] = kind; w[1] = q; w[19] = slot;
        w[4] = __float_as_uint(pos.x); w[5] = __float_as_uint(pos.y); w[6] = __float_as_uint(pos.z);
        w[7] = __float_as_uint(dir.x); w[8] = __float_as_uint(dir.y); w[9] = __float_as_uint(dir.z);
        w[10] = (uint32_t)last_in;
    }
    __device__ __forceinline__ void filled(int tri, const State &s) {
        if (!on) return;
        w[2] = (uint32_t)tri; w[3] = __float_as_uint(s.distance); w[11] = (uint32_t)s.material1;
        w[12] = __float_as_uint(s.absorption_length); w[13] = __float_as_uint(s.scattering_length);
    }
    __device__ __forceinline__ void end(V3 pos, uint32_t history, float time) {
        if (!on) return;
        w[14] = __float_as_uint(pos.x); w[15] = __float_as_uint(pos.y); w[16] = __float_as_uint(pos.z);
        w[17] = history; w[18] = __float_as_uint(time);
        const uint32_t i = atomicAdd(&chr_watch_n, 1u);
        if (i < CHR_WATCH_MAX)
            for (uint32_t k = 0; k < CHR_WATCH_WORDS; ++k) chr_watch_buf[i * CHR_WATCH_WORDS + k] = w[k];
        on = false;
    }
};
// trace_kernel's walk of the watched ray (origin bits chr_wray_o, chr_watch_ray):
// one 8-word event per step of its lane -- kind, then kind-specific words.
constexpr uint32_t CHR_WEV_MAX = 8192;
__device__ uint32_t chr_wray_on = 0u;
__device__ uint32_t chr_wray_o[3];
__device__ uint32_t chr_wev_n = 0u;
__device__ uint32_t chr_wev_buf[CHR_WEV_MAX * 8];
__device__ __forceinline__ bool wray_match(V3 o) {
    return chr_wray_on && __float_as_uint(o.x) == chr_wray_o[0] && __float_as_uint(o.y) == chr_wray_o[1] &&
           __float_as_uint(o.z) == chr_wray_o[2];
}
__device__ __forceinline__ void wev(uint32_t k, uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e,
                                    uint32_t f, uint32_t h) {
    const uint32_t i = atomicAdd(&chr_wev_n, 1u);
    if (i >= CHR_WEV_MAX) return;
    uint32_t *w = chr_wev_buf + 8 * i;
    w[0] = k; w[1] = a; w[2] = b; w[3] = c; w[4] = d; w[5] = e; w[6] = f; w[7] = h;
}
#define CHR_WEV(on, ...) do { if (on) wev(__VA_ARGS__); } while (0)
#else
#define CHR_WEV(on, ...) do { } while (0)
struct Watch {
    __device__ __forceinline__ void begin(uint32_t, uint32_t, const float *, uint32_t, uint32_t, V3, V3, int) {}
    __device__ __forceinline__ void filled(int, const State &) {}
    __device__ __forceinline__ void end(V3, uint32_t, float) {}
};
#endif

// Where the lone walker's iteration goes (walk_segment<64>, the tail's
// long-lived photon; device profile build only): wave-cycles of its stack
// refill, its fetch (the loads issued and waited for at once, so the expansion
// after it is compute only), the children's slab tests + near child + pushes +
// triangle list, and the triangle tests + hit reduction; calls = iterations.
template <bool ON>
struct LoneProf {
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void tick(int) {}
    __device__ __forceinline__ void wait_loads() {}
    __device__ __forceinline__ void flush() {}
};
#ifdef CHR_DEVICE_PROFILE
template <>
struct LoneProf<true> {
    unsigned long long cyc[4] = {0ull, 0ull, 0ull, 0ull}, iters = 0ull, t = 0ull;
    __device__ __forceinline__ void begin() { t = __builtin_amdgcn_s_memtime(); iters++; }
    __device__ __forceinline__ void tick(int i) {
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        cyc[i] += now - t;
        t = now;
    }
    __device__ __forceinline__ void wait_loads() { __builtin_amdgcn_s_waitcnt(0); }
    __device__ __forceinline__ void flush() {
        if (__lane_id() == 0) {
            for (int i = 0; i < 4; ++i) atomicAdd(&chr_prof_cycles[CHR_PROF_LONE_REFILL + i], cyc[i]);
            atomicAdd(&chr_prof_calls[CHR_PROF_LONE_WALK], iters);
            atomicAdd(&chr_prof_cycles[CHR_PROF_LONE_WALK], cyc[0] + cyc[1] + cyc[2] + cyc[3]);
        }
    }
};
#endif

// Where a long-lived photon's tail step goes (profile build: CHR_PROF_LONG_*):
// wave cycles per phase of the steps beyond the 64th of each photon, counted by its
// group's first lane.  mark(i) closes phase i at the current clock.
enum { LP_WALK, LP_FILL, LP_TO_BOUNDARY, LP_AT_BOUNDARY, LP_OTHER, LP_N };
template <bool ON>
struct LongProf {
    __device__ __forceinline__ void step(bool) {}
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ void flush() {}
};
#ifdef CHR_DEVICE_PROFILE
template <>
struct LongProf<true> {
    unsigned long long cyc[LP_N] = {0ull, 0ull, 0ull, 0ull, 0ull}, steps = 0ull, t = 0ull;
    bool on = false;
    // a step begins (on: this lane's photon is long and walks this step); the time
    // since the last phase closed is OTHER (the loop, the ballots, the walk's set-up)
    __device__ __forceinline__ void step(bool long_walk) {
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        if (on) cyc[LP_OTHER] += now - t;
        on = long_walk;
        if (on) steps++;
        t = now;
    }
    __device__ __forceinline__ void mark(int i) {
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        if (on) cyc[i] += now - t;
        t = now;
    }
    __device__ __forceinline__ void flush() {
        prof_add(CHR_PROF_LONG_WALK, steps, cyc[LP_WALK]);
        prof_add(CHR_PROF_LONG_FILL, 0ull, cyc[LP_FILL]);
        prof_add(CHR_PROF_LONG_TO_BOUNDARY, 0ull, cyc[LP_TO_BOUNDARY]);
        prof_add(CHR_PROF_LONG_AT_BOUNDARY, 0ull, cyc[LP_AT_BOUNDARY]);
        prof_add(CHR_PROF_LONG_OTHER, 0ull, cyc[LP_OTHER]);
    }
};
#endif

}  // namespace chr

// ---------------------------------------------------------------- host only: the C ABI
// These are definitions, not inline: include this header from propagate.hip alone.
// Device profile counters (profile.h; profiler.py:217-262 device_fetch / device_reset)
extern "C" int chr_device_profile_enabled(void) {
#ifdef CHR_DEVICE_PROFILE
    return 1;
#else
    return 0;
#endif
}

extern "C" int chr_device_profile_reset(void *stream) {
#ifdef CHR_DEVICE_PROFILE
    void *calls = nullptr, *cycles = nullptr;
    CHR_HIP_CHECK(hipGetSymbolAddress(&calls, HIP_SYMBOL(chr::chr_prof_calls)));
    CHR_HIP_CHECK(hipGetSymbolAddress(&cycles, HIP_SYMBOL(chr::chr_prof_cycles)));
    CHR_HIP_CHECK(hipMemsetAsync(calls, 0, sizeof(unsigned long long) * CHR_PROF_COUNT, (hipStream_t)stream));
    CHR_HIP_CHECK(hipMemsetAsync(cycles, 0, sizeof(unsigned long long) * CHR_PROF_COUNT, (hipStream_t)stream));
    return CHR_OK;
#else
    (void)stream;
    return chr::fail(CHR_ERR_INVALID, "device profiling symbols not found: load libchroma_amd_prof.so "
                                      "(built with -DCHR_DEVICE_PROFILE=1; CHROMA_DEVICE_PROFILE=1)");
#endif
}

extern "C" int chr_device_profile_fetch(uint64_t *h_calls, uint64_t *h_cycles, int32_t n, uint32_t *clock_khz) {
#ifdef CHR_DEVICE_PROFILE
    if (!h_calls || !h_cycles || n < 0 || n > CHR_PROF_COUNT)
        return chr::fail(CHR_ERR_INVALID, "device_profile_fetch: bad arguments");
    CHR_HIP_CHECK(hipDeviceSynchronize());
    unsigned long long c[CHR_PROF_COUNT], y[CHR_PROF_COUNT];
    CHR_HIP_CHECK(hipMemcpyFromSymbol(c, HIP_SYMBOL(chr::chr_prof_calls), sizeof(c)));
    CHR_HIP_CHECK(hipMemcpyFromSymbol(y, HIP_SYMBOL(chr::chr_prof_cycles), sizeof(y)));
    for (int i = 0; i < n; ++i) { h_calls[i] = c[i]; h_cycles[i] = y[i]; }
    if (clock_khz) {
        int dev = 0, khz = 0;
        CHR_HIP_CHECK(hipGetDevice(&dev));
        CHR_HIP_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, dev));
        *clock_khz = (uint32_t)khz;
    }
    return CHR_OK;
#else
    (void)h_calls; (void)h_cycles; (void)n; (void)clock_khz;
    return chr::fail(CHR_ERR_INVALID, "device profiling symbols not found: load libchroma_amd_prof.so "
                                      "(built with -DCHR_DEVICE_PROFILE=1; CHROMA_DEVICE_PROFILE=1)");
#endif
}

extern "C" int chr_watch_set(uint32_t photon, const float *d_pos_array) {
#ifdef CHR_DEVICE_PROFILE
    const unsigned long long arr = (unsigned long long)d_pos_array;
    const uint32_t zero = 0u;
    CHR_HIP_CHECK(hipDeviceSynchronize());
    CHR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(chr::chr_watch_pid), &photon, sizeof(photon)));
    CHR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(chr::chr_watch_array), &arr, sizeof(arr)));
    CHR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(chr::chr_watch_n), &zero, sizeof(zero)));
    return CHR_OK;
#else
    (void)photon; (void)d_pos_array;
    return chr::fail(CHR_ERR_INVALID, "photon watch: load libchroma_amd_prof.so (CHROMA_DEVICE_PROFILE=1)");
#endif
}

extern "C" int chr_watch_ray(const float *h_origin, uint32_t *h_events, uint32_t max_events, uint32_t *nevents) {
#ifdef CHR_DEVICE_PROFILE
    CHR_HIP_CHECK(hipDeviceSynchronize());
    if (h_origin) {   // arm: the walk of the ray with this origin (bit-exact) is logged
        const uint32_t on = 1u, zero = 0u;
        CHR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(chr::chr_wray_o), h_origin, 3 * sizeof(float)));
        CHR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(chr::chr_wev_n), &zero, sizeof(zero)));
        CHR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(chr::chr_wray_on), &on, sizeof(on)));
        return CHR_OK;
    }
    if (!h_events || !nevents) return chr::fail(CHR_ERR_INVALID, "watch_ray: bad arguments");
    uint32_t n = 0;
    CHR_HIP_CHECK(hipMemcpyFromSymbol(&n, HIP_SYMBOL(chr::chr_wev_n), sizeof(n)));
    *nevents = n;
    uint32_t k = n < max_events ? n : max_events;
    if (k > chr::CHR_WEV_MAX) k = chr::CHR_WEV_MAX;
    if (k) CHR_HIP_CHECK(hipMemcpyFromSymbol(h_events, HIP_SYMBOL(chr::chr_wev_buf), sizeof(uint32_t) * 8 * k));
    return CHR_OK;
#else
    (void)h_origin; (void)h_events; (void)max_events; (void)nevents;
    return chr::fail(CHR_ERR_INVALID, "photon watch: load libchroma_amd_prof.so (CHROMA_DEVICE_PROFILE=1)");
#endif
}

extern "C" int chr_watch_fetch(uint32_t *h_out, uint32_t max_records, uint32_t *nrecords) {
#ifdef CHR_DEVICE_PROFILE
    if (!h_out || !nrecords) return chr::fail(CHR_ERR_INVALID, "watch_fetch: bad arguments");
    CHR_HIP_CHECK(hipDeviceSynchronize());
    uint32_t n = 0;
    CHR_HIP_CHECK(hipMemcpyFromSymbol(&n, HIP_SYMBOL(chr::chr_watch_n), sizeof(n)));
    *nrecords = n;
    uint32_t k = n < max_records ? n : max_records;
    if (k > chr::CHR_WATCH_MAX) k = chr::CHR_WATCH_MAX;
    if (k) CHR_HIP_CHECK(hipMemcpyFromSymbol(h_out, HIP_SYMBOL(chr::chr_watch_buf), sizeof(uint32_t) * k * chr::CHR_WATCH_WORDS));
    return CHR_OK;
#else
    (void)h_out; (void)max_records; (void)nrecords;
    return chr::fail(CHR_ERR_INVALID, "photon watch: load libchroma_amd_prof.so (CHROMA_DEVICE_PROFILE=1)");
#endif
}
