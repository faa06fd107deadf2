// library.hip -- gfx950 photon-library lookup (chr_library_expect, chr_library_sample,
// chr_library_loglike).
//
// expect   the hot path: per event, the rows counts[s, :] (and tmin[s, :]) of its
//          entries' sources are gathered and folded, channel by channel, into mu and
//          tfirst by library.h's step.  Lanes run along channels, so a wave reads
//          contiguous row bytes; the grid is channel tiles x events, so a few events on
//          a large detector still fill the chip.  An entry's (source, nphotons, t) and
//          its emitted[s] are the same in every lane of a workgroup: they are loaded
//          through uniform addresses and pinned to scalar registers (readfirstlane).
//          The fmaf chain of a channel is serial in the entries, the row loads are not:
//          the entry loop is unrolled (UNROLL_WIDE / UNROLL_NARROW entries) with every
//          row load of a group issued before the first fold; the group's weights and
//          times and the next group's sources are fetched while those rows are on their
//          way, so a row's address never waits for more than one load.  A slot that adds
//          nothing (source out of range, emitted == 0, past the event's end) still loads a
//          row -- row 0, or the source's own -- and folds nothing, so the loads stay
//          unconditional; an event without entries loads nothing at all.
//            wide    nchannels a multiple of 4 and 16-byte aligned arrays: 4 channels
//                    per lane through 16-byte loads, 1024 channels per workgroup;
//            narrow  1 channel per lane, 256 channels per workgroup; the same words.
//          One work-item owns an output word; no LDS, no atomics but `skipped` (one
//          add per event, from the first channel tile's first work-item).
// sample   one work-item per rng slot walks its pairs j, j + T, ... in ascending order
//          through library.h's chr_library_sample_pair: the draw counts differ from
//          pair to pair, so there is nothing to share between lanes.
// loglike  expect's structure with another ending: instead of storing mu, each lane
//          turns its channels' mu (and, with observed times, the histogram words
//          gathered on the way) into fixed-point words, which are summed as integers
//          over the wave, the workgroup (LDS) and the channel tiles (one 64-bit atomic
//          per workgroup and hypothesis); see loglike_kernel.
//
// All loops are bounded by the table; no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "common.h"
#include "library.h"

namespace chr_library {

constexpr int BLOCK = 256;
constexpr int UNROLL_WIDE = 4, UNROLL_NARROW = 8;    // rows in flight per lane: 16 B x 4, 4 B x 8
constexpr uint32_t MAX_GRID_Y = 65535u;

typedef unsigned long long u64;

struct Entries {
    const uint32_t *offsets, *source, *nphotons;
    const float *t;
    uint32_t nevents;
};

__device__ __forceinline__ uint32_t uniform_u32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ float uniform_f32(float x) { return chr_u2f(uniform_u32(chr_f2u(x))); }

template <int W> struct Words;
template <> struct Words<1> { typedef uint32_t u; typedef float f; };
template <> struct Words<4> { typedef uint4 u; typedef float4 f; };

__device__ __forceinline__ uint32_t word_of(const uint32_t &v, int) { return v; }
__device__ __forceinline__ uint32_t word_of(const uint4 &v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// slot u's row from its source word s (`have`: the slot is an entry): the source, or row 0 for a source that
// is none; counts the entry in nskipped then, and sets bit u of `known` for an entry of a source that exists
__device__ __forceinline__ uint32_t row_of(const chr_library_map &lib, uint32_t s, bool have, int u, uint32_t &known,
                                           uint32_t &nskipped) {
    const bool is_source = s < lib.nsources;
    if (have && !is_source) nskipped += 1u;
    if (have && is_source) known |= 1u << u;
    return is_source ? s : 0u;
}

// The rows of entries i .. i + U - 1 of the non-empty range [first, last), the same in every lane: the
// entry's source, or row 0 for a source that is none and for a slot past the end (which reads the last
// entry, so no index leaves the range).  Bit u of `known`: the slot is an entry of a source that exists.
// Each source is pinned to a scalar register as it arrives.
template <int U>
__device__ __forceinline__ void load_rows(const chr_library_map &lib, const Entries &en, uint32_t i, uint32_t last,
                                          uint32_t (&row)[U], uint32_t &known, uint32_t &nskipped) {
    known = 0u;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool have = i + u < last;
        row[u] = row_of(lib, uniform_u32(en.source[have ? i + u : last - 1u]), have, u, known, nskipped);
    }
}

// W channels per lane: c0 = (blockIdx.x * BLOCK + threadIdx.x) * W; events blockIdx.y, + gridDim.y, ...;
// U entries' rows in flight at a time
template <int W, int U, bool TMIN>
__global__ __launch_bounds__(BLOCK) void expect_kernel(chr_library_map lib, Entries en, float *__restrict__ mu_out,
                                                       float *__restrict__ tfirst_out, u64 *skipped) {
    typedef typename Words<W>::u UW;
    const uint32_t c0 = (blockIdx.x * BLOCK + threadIdx.x) * W;
    const bool lane_in = c0 < lib.nchannels;                       // wide: nchannels % 4 == 0, so c0 + 3 is in too
    const uint32_t cl = lane_in ? c0 : 0u;                         // lanes past the row read its first words
    const bool counts_skipped = blockIdx.x == 0 && threadIdx.x == 0;
    for (uint32_t e = blockIdx.y; e < en.nevents; e += gridDim.y) {
        const uint32_t first = uniform_u32(en.offsets[e]), last = uniform_u32(en.offsets[e + 1]);
        float mu[W], tf[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            mu[j] = 0.0f;
            tf[j] = chr_u2f(0x7f800000u);
        }
        uint32_t nskipped = 0u;
        uint32_t cur[U] = {}, next[U] = {}, cur_known = 0u, next_known = 0u;
        if (first < last) load_rows<U>(lib, en, first, last, cur, cur_known, nskipped);
        for (uint32_t i = first; i < last; i += U) {
            UW k[U], key[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t word = (size_t)cur[u] * lib.nchannels + cl;
                k[u] = *reinterpret_cast<const UW *>(lib.counts + word);
                if (TMIN) key[u] = *reinterpret_cast<const UW *>(lib.tmin + word);
            }
            // while those rows are on their way: this group's weights and times (emitted[] of the
            // sources fetched a group ago) and the next group's sources
            float w[U], t[U];
            uint32_t ok = 0u;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t at = i + u < last ? i + u : last - 1u;
                const uint32_t lo = uniform_u32((uint32_t)lib.emitted[cur[u]]);
                const uint32_t hi = uniform_u32((uint32_t)(lib.emitted[cur[u]] >> 32));
                const uint64_t em = ((uint64_t)hi << 32) | lo;
                if ((cur_known >> u & 1u) && em != 0u) ok |= 1u << u;
                w[u] = chr_library_weight(uniform_u32(en.nphotons[at]), em != 0u ? em : 1u);
                t[u] = uniform_f32(en.t[at]);
            }
            if (i + U < last) load_rows<U>(lib, en, i + U, last, next, next_known, nskipped);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (ok >> u & 1u) {
#pragma unroll
                    for (int j = 0; j < W; ++j)
                        chr_library_expect_step(w[u], t[u], word_of(k[u], j),
                                                TMIN ? word_of(key[u], j) : CHR_LIBRARY_NO_KEY, &mu[j], &tf[j]);
                }
                cur[u] = next[u];
            }
            cur_known = next_known;
        }
        if (lane_in) {
            const size_t out = (size_t)e * lib.nchannels + c0;
            if (W == 4) {
                *reinterpret_cast<float4 *>(mu_out + out) = make_float4(mu[0], mu[W > 1 ? 1 : 0], mu[W > 2 ? 2 : 0], mu[W > 3 ? 3 : 0]);
                if (TMIN)
                    *reinterpret_cast<float4 *>(tfirst_out + out) = make_float4(tf[0], tf[W > 1 ? 1 : 0], tf[W > 2 ? 2 : 0], tf[W > 3 ? 3 : 0]);
            } else {
                mu_out[out] = mu[0];
                if (TMIN) tfirst_out[out] = tf[0];
            }
        }
        if (counts_skipped && nskipped) atomicAdd(skipped, (u64)nskipped);
    }
}

struct Observed {
    const uint32_t *nobs;
    const float *tobs;
    uint32_t mode;
    float floor, tfloor;
};

__device__ __forceinline__ float word_of(const float &v, int) { return v; }
__device__ __forceinline__ float word_of(const float4 &v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// load_rows' rows and the entries' times, which the histogram gather's addresses wait for (slot u past the
// end has the last entry's): every load of the group is requested before the first word is pinned to a
// scalar register, so the group costs one round trip, not one per slot
template <int U>
__device__ __forceinline__ void load_rows_times(const chr_library_map &lib, const Entries &en, uint32_t i,
                                                uint32_t last, uint32_t (&row)[U], float (&t)[U], uint32_t &known,
                                                uint32_t &nskipped) {
    uint32_t s[U];
    float tv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t at = i + u < last ? i + u : last - 1u;
        s[u] = en.source[at];
        tv[u] = en.t[at];
    }
    known = 0u;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        row[u] = row_of(lib, uniform_u32(s[u]), i + u < last, u, known, nskipped);
        t[u] = uniform_f32(tv[u]);
    }
}

// chr_library_loglike.  Lanes, grid and the entry groups as in expect_kernel (hypothesis = event).  The
// tile's nobs / tobs are loaded once, ahead of the hypothesis loop.  A group's histogram words -- one per
// (entry of a source that exists, channel with nobs > 0 whose time falls into a bin), the bin differing
// from lane to lane -- are requested with the group's rows, their addresses being known from the times
// fetched a group ago.  Each lane turns its channels' terms into words; the words (0 past nchannels) are
// added over the wave with integer cross-lane adds, over the waves through LDS (two sets of slots used
// in turn, so one barrier per hypothesis), and work-item 0 adds the workgroup's sum to ll[h] with one
// 64-bit atomic; bad likewise.  Only integers cross lanes.
template <int W, int U, bool TIMED>
__global__ __launch_bounds__(BLOCK) void loglike_kernel(chr_library_map lib, Entries en, Observed ob,
                                                        long long *__restrict__ ll_out,
                                                        uint32_t *__restrict__ bad_out, u64 *skipped) {
    typedef typename Words<W>::u UW;
    typedef typename Words<W>::f FW;
    constexpr int WAVES = BLOCK / 64;
    __shared__ long long wave_ll[2][WAVES];
    __shared__ uint32_t wave_bad[2][WAVES];
    const uint32_t c0 = (blockIdx.x * BLOCK + threadIdx.x) * W;
    const bool lane_in = c0 < lib.nchannels;                       // wide: nchannels % 4 == 0, so c0 + 3 is in too
    const uint32_t cl = lane_in ? c0 : 0u;
    uint32_t n[W];
    float tobs[W];
    {
        const UW nw = *reinterpret_cast<const UW *>(ob.nobs + cl);
        FW tw = {};
        if (TIMED) tw = *reinterpret_cast<const FW *>(ob.tobs + cl);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            n[j] = lane_in ? word_of(nw, j) : 0u;                  // a lane past the row gathers nothing
            tobs[j] = word_of(tw, j);
        }
    }
    uint32_t slot = 0u, nskipped = 0u;                             // of all this workgroup's hypotheses: below 2^32 entries
    for (uint32_t h = blockIdx.y; h < en.nevents; h += gridDim.y, slot ^= 1u) {
        const uint32_t first = uniform_u32(en.offsets[h]), last = uniform_u32(en.offsets[h + 1]);
        float mu[W], a[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            mu[j] = a[j] = 0.0f;
            // the lane masks the observed words decide (n > 0, tobs a NaN) are made again for each hypothesis:
            // kept across the loop, a dozen 64-bit masks are more than the scalar registers hold
            asm volatile("" : "+v"(n[j]), "+v"(tobs[j]));
        }
        uint32_t cur[U] = {}, next[U] = {}, cur_known = 0u, next_known = 0u;
        float tcur[U] = {}, tnext[U] = {};
        if (first < last) load_rows_times<U>(lib, en, first, last, cur, tcur, cur_known, nskipped);
        for (uint32_t i = first; i < last; i += U) {
            UW k[U];
            uint32_t hw[U][W], binned = 0u;                        // bit u * W + j: hw[u][j] is a bin's word
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t word = (size_t)cur[u] * lib.nchannels + cl;
                k[u] = *reinterpret_cast<const UW *>(lib.counts + word);
                if (TIMED) {
#pragma unroll
                    for (int j = 0; j < W; ++j) {
                        hw[u][j] = 0u;
                        if ((cur_known >> u & 1u) && n[j] > 0u) {
                            const int32_t b = chr_library_loglike_bin(&lib, tobs[j], tcur[u]);
                            if (b >= 0) {
                                hw[u][j] = lib.thist[(word + j) * lib.ntbins + (uint32_t)b];
                                binned |= 1u << (u * W + j);
                            }
                        }
                    }
                }
            }
            float w[U];
            uint32_t ok = 0u;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t at = i + u < last ? i + u : last - 1u;
                const uint32_t lo = uniform_u32((uint32_t)lib.emitted[cur[u]]);
                const uint32_t hi = uniform_u32((uint32_t)(lib.emitted[cur[u]] >> 32));
                const uint64_t em = ((uint64_t)hi << 32) | lo;
                if ((cur_known >> u & 1u) && em != 0u) ok |= 1u << u;
                w[u] = chr_library_weight(uniform_u32(en.nphotons[at]), em != 0u ? em : 1u);
            }
            if (i + U < last) load_rows_times<U>(lib, en, i + U, last, next, tnext, next_known, nskipped);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (ok >> u & 1u) {
#pragma unroll
                    for (int j = 0; j < W; ++j) {
                        float no_time = 0.0f;
                        chr_library_expect_step(w[u], tcur[u], word_of(k[u], j), CHR_LIBRARY_NO_KEY, &mu[j], &no_time);
                        if (TIMED && (binned >> (u * W + j) & 1u)) chr_library_loglike_time_step(w[u], hw[u][j], &a[j]);
                    }
                }
                cur[u] = next[u];
                tcur[u] = tnext[u];
            }
            cur_known = next_known;
        }
        long long q = 0;
        uint32_t bad = 0u;
        if (lane_in) {
#pragma unroll
            for (int j = 0; j < W; ++j)
                q += chr_library_loglike_word(chr_library_loglike_term(mu[j], a[j], n[j], TIMED, tobs[j], ob.mode,
                                                                       ob.floor, ob.tfloor, lib.inv), &bad);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            q += __shfl_xor(q, off);
            bad += __shfl_xor(bad, off);
        }
        if ((threadIdx.x & 63u) == 0u) {
            wave_ll[slot][threadIdx.x >> 6] = q;
            wave_bad[slot][threadIdx.x >> 6] = bad;
        }
        __syncthreads();                                           // h depends on blockIdx alone: every wave arrives
        if (threadIdx.x == 0) {
            long long sum = 0;
            uint32_t nbad = 0u;
#pragma unroll
            for (int v = 0; v < WAVES; ++v) {
                sum += wave_ll[slot][v];
                nbad += wave_bad[slot][v];
            }
            if (sum) atomicAdd(reinterpret_cast<u64 *>(ll_out + h), (u64)sum);
            if (nbad) atomicAdd(bad_out + h, nbad);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && nskipped) atomicAdd(skipped, (u64)nskipped);
}

// work-item j < T: rng slot j, pairs j, j + T, ...
__global__ __launch_bounds__(BLOCK) void sample_kernel(chr_library_map lib, Entries en, uint32_t *rng_states,
                                                       uint32_t nslots, uint32_t T, uint32_t npairs, uint32_t *n_out,
                                                       float *t_out, u64 *skipped) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= T) return;
    const size_t ns = nslots;
    chr_xorwow rng = {rng_states[j], rng_states[ns + j], rng_states[2 * ns + j], rng_states[3 * ns + j],
                      rng_states[4 * ns + j], rng_states[5 * ns + j]};
    for (uint64_t pair = j; pair < npairs; pair += T) {
        const uint32_t e = (uint32_t)(pair / lib.nchannels), c = (uint32_t)(pair % lib.nchannels);
        const uint32_t first = en.offsets[e], last = en.offsets[e + 1];
        chr_library_sample_pair(&lib, en.source, en.nphotons, en.t, first, last, c, &rng, n_out + pair, t_out + pair);
        if (c == 0u) {                                             // the event's entries of no source, once
            uint32_t nskipped = 0u;
            for (uint32_t i = first; i < last; ++i) nskipped += en.source[i] >= lib.nsources ? 1u : 0u;
            if (nskipped) atomicAdd(skipped, (u64)nskipped);
        }
    }
    rng_states[j] = rng.d;
    rng_states[ns + j] = rng.v0;
    rng_states[2 * ns + j] = rng.v1;
    rng_states[3 * ns + j] = rng.v2;
    rng_states[4 * ns + j] = rng.v3;
    rng_states[5 * ns + j] = rng.v4;
}

Entries entries_of(const chr_library_entries *en) {
    return Entries{en->offsets, en->source, en->nphotons, en->t, en->nevents};
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

bool narrow_forced() {
    const char *e = getenv("CHR_LIBRARY_PATH");
    return e && e[0] == 'n';
}

// CHR_LIBRARY_PATH=n forces the narrow path (A/B, tests); the wide one needs its alignment
bool use_wide(const chr_library_map &lib, const float *mu, const float *tfirst) {
    if (lib.nchannels % 4u != 0u || !aligned16(lib.counts) || !aligned16(mu)) return false;
    if (lib.tmin && (!aligned16(lib.tmin) || !aligned16(tfirst))) return false;
    return !narrow_forced();
}

// with observed times the call is bound by the histogram gather, one word per (entry, hit channel) whatever
// the lane's width, and four channels per lane only cost workgroups: the wide path is for calls without times
bool loglike_wide(const chr_library_map &lib, const chr_library_observed *obs) {
    if (obs->tobs || lib.nchannels % 4u != 0u || !aligned16(lib.counts) || !aligned16(obs->nobs)) return false;
    return !narrow_forced();
}

thread_local int last_path = -1, loglike_last_path = -1;

template <int W, int U, bool TIMED>
void launch_loglike(const chr_library_map &lib, const chr_library_entries *hyp, const chr_library_observed *obs,
                    int64_t *ll, uint32_t *bad, u64 *skipped, hipStream_t stream) {
    const uint32_t per_wg = BLOCK * W;
    const dim3 grid((lib.nchannels + per_wg - 1) / per_wg, std::min(hyp->nevents, MAX_GRID_Y));
    const Observed ob{obs->nobs, obs->tobs, obs->mode, obs->floor, obs->tfloor};
    hipLaunchKernelGGL((loglike_kernel<W, U, TIMED>), grid, dim3(BLOCK), 0, stream, lib, entries_of(hyp), ob,
                       (long long *)ll, bad, skipped);
}

template <int W, int U>
void launch_expect(const chr_library_map &lib, const chr_library_entries *en, float *mu, float *tfirst, u64 *skipped,
                   hipStream_t stream) {
    const uint32_t per_wg = BLOCK * W;
    const dim3 grid((lib.nchannels + per_wg - 1) / per_wg, std::min(en->nevents, MAX_GRID_Y));
    if (lib.tmin)
        hipLaunchKernelGGL((expect_kernel<W, U, true>), grid, dim3(BLOCK), 0, stream, lib, entries_of(en), mu, tfirst,
                           skipped);
    else
        hipLaunchKernelGGL((expect_kernel<W, U, false>), grid, dim3(BLOCK), 0, stream, lib, entries_of(en), mu, tfirst,
                           skipped);
}

}  // namespace chr_library

using namespace chr_library;

extern "C" int chr_library_expect(const chr_hitmap_desc *desc, const chr_library_entries *entries, float *d_mu,
                                  float *d_tfirst, uint64_t *d_skipped, void *stream) {
    chr_library_map lib;
    CHR_TRY(chr::library_check("chr_library_expect", desc, entries, d_mu, d_tfirst, d_skipped, 0, nullptr, 0, &lib));
    if (entries->nevents == 0) return CHR_OK;
    const bool wide = use_wide(lib, d_mu, d_tfirst);
    if (wide) launch_expect<4, UNROLL_WIDE>(lib, entries, d_mu, d_tfirst, (u64 *)d_skipped, (hipStream_t)stream);
    else launch_expect<1, UNROLL_NARROW>(lib, entries, d_mu, d_tfirst, (u64 *)d_skipped, (hipStream_t)stream);
    CHR_HIP_CHECK(hipGetLastError());
    last_path = wide ? 1 : 0;
    return CHR_OK;
}

extern "C" int chr_library_last_path(void) { return last_path; }

extern "C" int chr_library_loglike(const chr_hitmap_desc *desc, const chr_library_entries *hyp,
                                   const chr_library_observed *obs, int64_t *d_ll, uint32_t *d_bad,
                                   uint64_t *d_skipped, void *stream) {
    chr_library_map lib;
    CHR_TRY(chr::library_loglike_check("chr_library_loglike", desc, hyp, obs, d_ll, d_bad, d_skipped, &lib));
    if (hyp->nevents == 0) return CHR_OK;
    CHR_HIP_CHECK(hipMemsetAsync(d_ll, 0, sizeof(int64_t) * (size_t)hyp->nevents, (hipStream_t)stream));
    CHR_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(uint32_t) * (size_t)hyp->nevents, (hipStream_t)stream));
    const bool wide = loglike_wide(lib, obs);
    // with times, half the entries per group: each brings its histogram words, and the scalar registers are few
    if (wide) launch_loglike<4, UNROLL_WIDE, false>(lib, hyp, obs, d_ll, d_bad, (u64 *)d_skipped, (hipStream_t)stream);
    else if (obs->tobs)
        launch_loglike<1, UNROLL_NARROW / 2, true>(lib, hyp, obs, d_ll, d_bad, (u64 *)d_skipped, (hipStream_t)stream);
    else launch_loglike<1, UNROLL_NARROW, false>(lib, hyp, obs, d_ll, d_bad, (u64 *)d_skipped, (hipStream_t)stream);
    CHR_HIP_CHECK(hipGetLastError());
    loglike_last_path = wide ? 1 : 0;
    return CHR_OK;
}

extern "C" int chr_library_loglike_last_path(void) { return loglike_last_path; }

extern "C" int chr_library_sample(const chr_hitmap_desc *desc, const chr_library_entries *entries,
                                  uint32_t *d_rng_states, uint32_t nslots, uint32_t *d_n, float *d_t,
                                  uint64_t *d_skipped, void *stream) {
    chr_library_map lib;
    CHR_TRY(chr::library_check("chr_library_sample", desc, entries, d_n, d_t, d_skipped, 1, d_rng_states, nslots, &lib));
    if (entries->nevents == 0) return CHR_OK;
    const uint64_t npairs = (uint64_t)entries->nevents * lib.nchannels;          // <= 2^31 (checked)
    const uint32_t T = (uint32_t)std::min<uint64_t>(nslots, npairs);
    hipLaunchKernelGGL(sample_kernel, dim3((T + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, (hipStream_t)stream, lib,
                       entries_of(entries), d_rng_states, nslots, T, (uint32_t)npairs, d_n, d_t, (u64 *)d_skipped);
    CHR_HIP_CHECK(hipGetLastError());
    return CHR_OK;
}
