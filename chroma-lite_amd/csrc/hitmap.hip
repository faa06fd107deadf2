// hitmap.hip -- gfx950 hit-map accumulation (chr_hitmap_accumulate, chr_hitmap_clear).
//
// One work-item per photon of a 256-photon tile; a workgroup walks a contiguous
// range of tiles.  The per-photon rule is hitmap.h's (shared with the host twin);
// this file only decides where each word is added:
//
//  emitted   gensteps number photons step-major, so a source's photons are
//            consecutive.  Each wave finds its runs of equal evidx (one ballot) and
//            the run's first lane adds the run length: into an LDS word while the
//            run belongs to the workgroup's current source (the evidx of the tile's
//            first photon), else into global memory.  The LDS word goes out with
//            one global atomic when the current source changes and at the end, so
//            a workgroup inside one source issues one atomic for it, not one per
//            photon or per wave.
//  direct    (PRIVATE = false) the words of rule steps 4-7 go to global memory.
//  private   (PRIVATE = true) the row of the current source is kept in LDS
//            (ds_add_u32, ds_min_u32, ds_add_u64); lanes of another source go the
//            direct way.  When the current source changes, and at the end, the
//            workgroup sweeps the row into global memory, work-item i taking words
//            i, i + 256, ... (consecutive lanes on consecutive words), and clears
//            it.  Needs the row to fit CHR_HITMAP_LDS_WORDS (use_private below).
//
// Every update is an integer add or an unsigned min, so both paths and every
// photon order give the same words; only the speed depends on the order.  All
// loops are bounded by the range and the row; no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "common.h"
#include "hitmap.h"

namespace chr_hitmap {

constexpr int BLOCK = 256;
constexpr uint32_t LDS_WORDS = CHR_HITMAP_LDS_WORDS;

typedef unsigned long long u64;

struct MapArrays {
    u64 *emitted, *wsum, *skipped;
    uint32_t *counts, *tmin, *thist;
};

__global__ __launch_bounds__(BLOCK) void clear_kernel(MapArrays m, uint32_t nsources, uint32_t words, uint32_t hwords) {
    const uint32_t stride = gridDim.x * BLOCK;
    const uint32_t first = blockIdx.x * BLOCK + threadIdx.x;
    for (uint32_t i = first; i < nsources; i += stride) m.emitted[i] = 0ull;
    for (uint32_t i = first; i < words; i += stride) {
        m.counts[i] = 0u;
        if (m.tmin) m.tmin[i] = CHR_HITMAP_NO_KEY;
        if (m.wsum) m.wsum[i] = 0ull;
    }
    for (uint32_t i = first; i < hwords; i += stride) m.thist[i] = 0u;
    if (first == 0) *m.skipped = 0ull;
}

// rule steps 4-7 into global memory
__device__ __forceinline__ void add_global(const MapArrays &m, const chr_hitmap_par &par, const chr_hitmap_update &u) {
    const size_t w = (size_t)u.source * par.nchannels + (uint32_t)u.channel;
    atomicAdd(m.counts + w, 1u);
    if (u.key != CHR_HITMAP_NO_KEY) atomicMin(m.tmin + w, u.key);
    if (u.bin >= 0) atomicAdd(m.thist + w * par.ntbins + (uint32_t)u.bin, 1u);
    if (par.has_wsum) atomicAdd(m.wsum + w, (u64)u.q);
}

// The LDS row of one source: wsum (two words per channel, first for its alignment),
// counts, tmin, thist; nchannels * (2*[wsum] + 1 + [tmin] + ntbins) <= LDS_WORDS words.
struct Row {
    u64 *wsum;
    uint32_t *counts, *tmin, *thist;
};

__device__ __forceinline__ Row row_of(uint32_t *lds, const chr_hitmap_par &par) {
    Row r;
    uint32_t *at = lds;
    r.wsum = (u64 *)at;
    if (par.has_wsum) at += 2 * par.nchannels;
    r.counts = at;
    at += par.nchannels;
    r.tmin = at;
    if (par.has_tmin) at += par.nchannels;
    r.thist = at;
    return r;
}

// The workgroup's LDS words of source `cur` into global memory, cleared as they go.
// sweep_all: also the words that hold nothing (A/B; the default leaves them out).
template <bool PRIVATE>
__device__ __forceinline__ void sweep(const MapArrays &m, const chr_hitmap_par &par, const Row &row, u64 *cur_emitted,
                                      uint32_t cur, bool sweep_all) {
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        const u64 n = *cur_emitted;
        *cur_emitted = 0ull;
        if (n) atomicAdd(cur < par.nsources ? m.emitted + cur : m.skipped, n);
    }
    if (!PRIVATE || cur >= par.nsources) return;     // a skipped source never wrote its row
    const size_t base = (size_t)cur * par.nchannels;
    for (uint32_t c = tid; c < par.nchannels; c += BLOCK) {
        const uint32_t v = row.counts[c];
        row.counts[c] = 0u;
        if (v || sweep_all) atomicAdd(m.counts + base + c, v);
    }
    if (par.has_tmin)
        for (uint32_t c = tid; c < par.nchannels; c += BLOCK) {
            const uint32_t v = row.tmin[c];
            row.tmin[c] = CHR_HITMAP_NO_KEY;
            if (v != CHR_HITMAP_NO_KEY || sweep_all) atomicMin(m.tmin + base + c, v);
        }
    if (par.has_wsum)
        for (uint32_t c = tid; c < par.nchannels; c += BLOCK) {
            const u64 v = row.wsum[c];
            row.wsum[c] = 0ull;
            if (v || sweep_all) atomicAdd(m.wsum + base + c, v);
        }
    const uint32_t hwords = par.nchannels * par.ntbins;
    for (uint32_t i = tid; i < hwords; i += BLOCK) {
        const uint32_t v = row.thist[i];
        row.thist[i] = 0u;
        if (v || sweep_all) atomicAdd(m.thist + base * par.ntbins + i, v);
    }
}

// Photons [start + wg*tiles_per_wg*BLOCK, ...) of [start, start + n), one tile at a time.
template <bool PRIVATE>
__global__ __launch_bounds__(BLOCK) void accumulate_kernel(chr_hitmap_inputs in, chr_hitmap_par par, MapArrays m,
                                                           uint32_t start, uint32_t n, uint32_t tiles_per_wg,
                                                           int sweep_all) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[PRIVATE ? LDS_WORDS : 2];
    __shared__ u64 cur_emitted;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const Row row = row_of(lds, par);
    const uint64_t span = (uint64_t)tiles_per_wg * BLOCK;
    const uint64_t begin = (uint64_t)blockIdx.x * span;
    if (begin >= n) return;                                   // whole workgroup: before any barrier
    const uint64_t end = begin + span < n ? begin + span : n;

    if (tid == 0) cur_emitted = 0ull;
    if (PRIVATE) {
        const uint32_t words = par.nchannels * ((par.has_wsum ? 2u : 0u) + 1u + (par.has_tmin ? 1u : 0u) + par.ntbins);
        for (uint32_t i = tid; i < words; i += BLOCK) lds[i] = 0u;
        __syncthreads();
        if (par.has_tmin)
            for (uint32_t c = tid; c < par.nchannels; c += BLOCK) row.tmin[c] = CHR_HITMAP_NO_KEY;
    }
    __syncthreads();

    uint32_t cur = in.evidx[(size_t)start + begin];
    for (uint64_t tile = begin; tile < end; tile += BLOCK) {
        const uint32_t first = in.evidx[(size_t)start + tile];      // the same word in every work-item
        if (first != cur) {
            __syncthreads();
            sweep<PRIVATE>(m, par, row, &cur_emitted, cur, sweep_all);
            __syncthreads();
            cur = first;
        }
        const uint64_t i = tile + tid;
        const bool active = i < end;
        chr_hitmap_update u;
        u.source = 0u;
        int counted = 0;
        if (active) counted = chr_hitmap_photon(&par, &in, (size_t)start + i, &u);

        // rule steps 1-2: one add per run of equal evidx in the wave (active lanes are a prefix of it)
        const uint32_t prev = __shfl_up(u.source, 1);
        const bool head = active && (lane == 0 || prev != u.source);
        const u64 heads = __ballot(head), act = __ballot(active);
        if (head) {
            const u64 above = lane == 63u ? 0ull : heads & ~((2ull << lane) - 1ull);
            const uint32_t next = above ? (uint32_t)__builtin_ctzll(above) : (uint32_t)__builtin_popcountll(act);
            const u64 len = next - lane;
            if (u.source == cur) atomicAdd(&cur_emitted, len);
            else atomicAdd(u.source < par.nsources ? m.emitted + u.source : m.skipped, len);
        }

        // rule steps 4-7
        if (counted && u.channel >= 0) {
            if (PRIVATE && u.source == cur) {
                const uint32_t c = (uint32_t)u.channel;
                atomicAdd(row.counts + c, 1u);
                if (u.key != CHR_HITMAP_NO_KEY) atomicMin(row.tmin + c, u.key);
                if (u.bin >= 0) atomicAdd(row.thist + c * par.ntbins + (uint32_t)u.bin, 1u);
                if (par.has_wsum) atomicAdd(row.wsum + c, (u64)u.q);
            } else {
                add_global(m, par, u);
            }
        }
    }
    __syncthreads();
    sweep<PRIVATE>(m, par, row, &cur_emitted, cur, sweep_all);
}

MapArrays arrays_of(const chr_hitmap_desc *d) {
    return MapArrays{(u64 *)d->d_emitted, (u64 *)d->d_wsum, (u64 *)d->d_skipped, d->d_counts, d->d_tmin, d->d_thist};
}

// words of one source's row in LDS
uint64_t row_words(const chr_hitmap_desc *d) {
    return (uint64_t)(uint32_t)d->nchannels * (1u + (d->d_tmin ? 1u : 0u) + (uint64_t)d->ntbins + (d->d_wsum ? 2u : 0u));
}

// The path of a call.  A row over the LDS budget goes the direct way whatever is asked;
// CHR_HITMAP_PATH=d|l forces the direct / the privatised path (A/B, tests).  Default, from
// the measurements of DESIGN.md section 19 (300 channels, 10^3 sources of 10^4 photons):
// privatised when the map keeps a time histogram or weight sums (four updates per detected
// photon: 120 us against 156 us direct), direct for counts and tmin alone (82 us against
// 96 us: two updates do not pay for the sweep and the 32 KB of LDS per workgroup).
bool use_private(const chr_hitmap_desc *d) {
    if (row_words(d) > LDS_WORDS) return false;
    const char *e = getenv("CHR_HITMAP_PATH");
    if (e && (e[0] == 'd' || e[0] == 'l')) return e[0] == 'l';
    return d->ntbins > 0 || d->d_wsum != nullptr;
}

// CHR_HITMAP_SWEEP=a: the sweep also adds the words that hold nothing (A/B)
bool sweep_everything() {
    const char *e = getenv("CHR_HITMAP_SWEEP");
    return e && e[0] == 'a';
}

thread_local int last_path = -1;

// workgroups that run at once: the device's CUs x the workgroups of BLOCK a CU holds
// (8 by its 2048 work-items; 4 by the private path's 32 KB + 8 B of the CU's 160 KB LDS)
int resident_workgroups(bool priv, uint32_t *out) {
    int dev = 0, cus = 0;
    CHR_HIP_CHECK(hipGetDevice(&dev));
    CHR_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    *out = (uint32_t)std::max(cus, 1) * (priv ? 4u : 8u);
    return CHR_OK;
}

}  // namespace chr_hitmap

using namespace chr_hitmap;

extern "C" int chr_hitmap_clear(const chr_hitmap_desc *desc, void *stream) {
    CHR_TRY(chr::hitmap_check_desc("chr_hitmap_clear", desc));
    const uint32_t words = desc->nsources * (uint32_t)desc->nchannels;       // <= 2^31 each (checked)
    const uint32_t hwords = words * desc->ntbins;
    const uint32_t most = std::max(std::max(words, hwords), desc->nsources);
    const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)most + BLOCK - 1) / BLOCK, 4096u);
    hipLaunchKernelGGL(clear_kernel, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, arrays_of(desc), desc->nsources,
                       words, hwords);
    CHR_HIP_CHECK(hipGetLastError());
    return CHR_OK;
}

extern "C" int chr_hitmap_accumulate(const chr_photons *ph, int32_t start_photon, int32_t nphotons,
                                     uint32_t detection_state, const uint32_t *d_solid_map,
                                     const int32_t *d_solid_id_to_channel_index, const chr_hitmap_desc *desc,
                                     void *stream) {
    chr_hitmap_par par;
    chr_hitmap_inputs in;
    CHR_TRY(chr::hitmap_check("chr_hitmap_accumulate", ph, start_photon, detection_state, d_solid_map,
                              d_solid_id_to_channel_index, desc, &par, &in));
    if (nphotons <= 0) return CHR_OK;
    const bool priv = use_private(desc);
    uint32_t resident = 0;
    CHR_TRY(resident_workgroups(priv, &resident));
    const uint32_t n = (uint32_t)nphotons;
    const uint32_t tiles = (n + BLOCK - 1) / BLOCK;
    const uint32_t tiles_per_wg = (tiles + resident - 1) / resident;
    const uint32_t grid = (tiles + tiles_per_wg - 1) / tiles_per_wg;
    const int all = sweep_everything() ? 1 : 0;
    if (priv)
        hipLaunchKernelGGL(accumulate_kernel<true>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, in, par,
                           arrays_of(desc), (uint32_t)start_photon, n, tiles_per_wg, all);
    else
        hipLaunchKernelGGL(accumulate_kernel<false>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, in, par,
                           arrays_of(desc), (uint32_t)start_photon, n, tiles_per_wg, all);
    CHR_HIP_CHECK(hipGetLastError());
    last_path = priv ? 1 : 0;
    return CHR_OK;
}

extern "C" int chr_hitmap_last_path(void) { return last_path; }
