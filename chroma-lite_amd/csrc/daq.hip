// daq.hip -- gfx950 DAQ kernels (the consumer of propagate's output) + C ABI.
//
// Reference: chroma/cuda/daq.cu (run_daq 35-83, run_daq_many 85-145,
// reset_earliest_time_int 25-33, convert_* 147-172) driven by GPUDaq
// (chroma/gpu/daq.py:37-101) with the Detector struct of detector.h:4-22.
//
// MI355X layout: the per-channel accumulators are three u32 arrays
// (ndaq*nchannels each; 29k channels = 116 KB, L2-resident), updated with
// device atomics whose results are order-independent (unsigned min of the
// time's bit pattern, integer charge sum, history OR).  A DAQ pass reads
// 20 B per photon (t, flags, last_hit, weight + the solid map entry of hit
// photons) and is HBM/launch bound; the chunked launches of the reference are
// folded into one launch in which work-item `slot` walks chunk positions
// slot, slot+cap, ... with its RNG state in registers (same draws, same order).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "../../include/chroma_amd.h"
#include "../../include/chroma_fmath.h"
#include "../../include/chroma_rng.h"
#include "common.h"

namespace chr_daq {

constexpr int BLOCK = 256;

// interpolate.h:32-58 (interp), as used by random.h:26-30 sample_cdf(x, y)
__device__ float interp(float x, int n, const float *xp, const float *fp) {
    int lower = 0, upper = n - 1;
    if (x <= xp[lower]) return fp[lower];
    if (x >= xp[upper]) return fp[upper];
    while (lower < upper - 1) {
        const int half = (lower + upper) / 2;
        if (x < xp[half]) upper = half; else lower = half;
    }
    const float df = fp[upper] - fp[lower];
    const float dx = xp[upper] - xp[lower];
    return fp[lower] + (df * (x - xp[lower])) / dx;
}

__device__ __forceinline__ float sample_cdf_xy(chr_xorwow &rng, int ncdf, const float *cdf_x, const float *cdf_y) {
    return interp(chr_uniform01(&rng), ncdf, cdf_y, cdf_x);
}

__device__ __forceinline__ void load_rng(const uint32_t *st, uint32_t ns, uint32_t s, chr_xorwow &r) {
    r.d = st[s]; r.v0 = st[ns + s]; r.v1 = st[2 * ns + s]; r.v2 = st[3 * ns + s]; r.v3 = st[4 * ns + s];
    r.v4 = st[5 * ns + s];
}
__device__ __forceinline__ void store_rng(uint32_t *st, uint32_t ns, uint32_t s, const chr_xorwow &r) {
    st[s] = r.d; st[ns + s] = r.v0; st[2 * ns + s] = r.v1; st[3 * ns + s] = r.v2; st[4 * ns + s] = r.v3;
    st[5 * ns + s] = r.v4;
}

struct DaqPhotons {
    const float *t, *weights;
    const uint32_t *flags;
    const int32_t *last_hit;
};

// daq.cu:25-33 + the zero fills of daq.py:56-60
__global__ __launch_bounds__(BLOCK) void begin_kernel(uint32_t *time_int, uint32_t *q_int, uint32_t *hist, uint32_t n,
                                                      uint32_t maxtime_bits) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    time_int[i] = maxtime_bits;
    q_int[i] = 0u;
    hist[i] = 0u;
}

// daq.cu:61-76: the draws for one detected photon on a channel (one uniform, two more
// when accepted) and the three atomics on that channel's words.  True when the photon
// was accepted, with the photoelectron's time and charge word in pe_time and pe_q.
__device__ __forceinline__ bool draw_hit(chr_xorwow &rng, const DaqPhotons &ph, uint32_t photon_id, uint32_t history,
                                         const chr_daq_detector &det, float global_weight, uint32_t *time_word,
                                         uint32_t *q_word, uint32_t *hist_word, float &pe_time, uint32_t &pe_q) {
    const float weight = ph.weights[photon_id] * global_weight;
    if (chr_uniform01(&rng) < weight) {
        const float time = ph.t[photon_id] + sample_cdf_xy(rng, det.time_cdf_len, det.d_time_cdf_x, det.d_time_cdf_y);
        const float charge = sample_cdf_xy(rng, det.charge_cdf_len, det.d_charge_cdf_x, det.d_charge_cdf_y);
        const uint32_t charge_int = chr_sat_u32(__builtin_roundf(charge / det.charge_unit));
        atomicMin(time_word, __float_as_uint(time));
        atomicAdd(q_word, charge_int);
        atomicOr(hist_word, history);
        pe_time = time;
        pe_q = charge_int;
        return true;
    }
    return false;
}

// daq.cu:35-83 over all chunks of [start, start+n): slot loops over chunk positions
__global__ __launch_bounds__(BLOCK) void run_daq_kernel(uint32_t *rng_states, uint32_t nslots, uint32_t detection_state,
                                                        int32_t start, uint32_t n, uint32_t cap, DaqPhotons ph,
                                                        const uint32_t *solid_map, chr_daq_detector det,
                                                        uint32_t *time_int, uint32_t *q_int, uint32_t *hist,
                                                        float global_weight) {
    const uint32_t slot = blockIdx.x * BLOCK + threadIdx.x;
    if (slot >= cap || slot >= n) return;
    chr_xorwow rng;
    bool loaded = false;
    for (uint32_t pos = slot; pos < n; pos += cap) {
        const uint32_t photon_id = (uint32_t)start + pos;
        const int triangle_id = ph.last_hit[photon_id];
        if (triangle_id <= -1) continue;
        const int solid_id = (int)solid_map[triangle_id];
        const uint32_t history = ph.flags[photon_id];
        const int channel_index = det.d_solid_id_to_channel_index[solid_id];
        if (!(channel_index >= 0 && (history & detection_state))) continue;
        if (!loaded) { load_rng(rng_states, nslots, slot, rng); loaded = true; }
        float pe_time;
        uint32_t pe_q;
        draw_hit(rng, ph, photon_id, history, det, global_weight, time_int + channel_index, q_int + channel_index,
                 hist + channel_index, pe_time, pe_q);
    }
    if (loaded) store_rng(rng_states, nslots, slot, rng);
}

// ---- every event of a batch in one launch (chr_daq_acquire_events)

// The channel of photon p where run_daq_kernel would draw for it, else -1 (daq.cu:52-59).
// A channel index beyond the detector's channels, which run_daq_kernel would write through,
// counts as "not detected" here: it would land in another event's row.
__device__ __forceinline__ int candidate_channel(const DaqPhotons &ph, uint32_t p, const uint32_t *solid_map,
                                                 const chr_daq_detector &det, uint32_t detection_state) {
    const int triangle_id = ph.last_hit[p];
    if (triangle_id <= -1) return -1;
    const int channel_index = det.d_solid_id_to_channel_index[(int)solid_map[triangle_id]];
    if (channel_index < 0 || channel_index >= det.nchannels || !(ph.flags[p] & detection_state)) return -1;
    return channel_index;
}

// The photoelectron records of chr_daq_acquire_events_pe, one per photon of the span
// [bounds[0], bounds[nevents]) and indexed from its first photon.
struct PeRecords {
    int32_t *channel;
    float *time;
    uint32_t *q;
};

// shape (b), pass 1: candidate_channel of photons [first, first+n), one work-item each
__global__ __launch_bounds__(BLOCK) void candidates_kernel(DaqPhotons ph, uint32_t first, uint32_t n,
                                                           const uint32_t *solid_map, chr_daq_detector det,
                                                           uint32_t detection_state, int32_t *cand) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    cand[i] = candidate_channel(ph, first + i, solid_map, det, detection_state);
}

// the same pass for the photoelectron variant: every record of the span starts as "no
// photoelectron" (-1, the 1e9 no-hit time, 0); the draws overwrite those of accepted photons
__global__ __launch_bounds__(BLOCK) void candidates_pe_kernel(DaqPhotons ph, uint32_t first, uint32_t n,
                                                              const uint32_t *solid_map, chr_daq_detector det,
                                                              uint32_t detection_state, int32_t *cand, PeRecords pe) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    cand[i] = candidate_channel(ph, first + i, solid_map, det, detection_state);
    pe.channel[i] = -1;
    pe.time[i] = 1e9f;
    pe.q[i] = 0u;
}

// The draws of run_daq_kernel for events e = 0 .. nevents-1 over photons
// [bounds[e], bounds[e+1]), into row e of the accumulators.  The work-item is the RNG
// slot: it takes part in event e iff slot < min(cap, n_e), visits positions slot,
// slot+cap, ... there, and carries its state in registers from event to event (the
// per-event launches' draw order).  The event loop and its skip are wave-uniform
// (bounds through uniform loads, the wave's first slot in an SGPR).  Only the RNG
// chain is serial across events: the candidate word of the slot's first position
// (CAND: read from pass 1's array, shape (b); else computed through last_hit ->
// solid_map -> channel, shape (a)) is read one event ahead of the draws.  PE: an accepted
// photon's record is also written (chr_daq_acquire_events_pe; a photon has one visitor,
// so plain stores); the walk, the draws and the atomics are the same text.
template <bool CAND, bool PE>
__global__ __launch_bounds__(BLOCK) void run_daq_events_kernel(uint32_t *rng_states, uint32_t nslots,
                                                               uint32_t detection_state,
                                                               const uint32_t *__restrict__ bounds, uint32_t nevents,
                                                               uint32_t cap, DaqPhotons ph, const uint32_t *solid_map,
                                                               chr_daq_detector det, const int32_t *__restrict__ cand,
                                                               uint32_t *time_int, uint32_t *q_int, uint32_t *hist,
                                                               float global_weight, PeRecords pe) {
    const uint32_t slot = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t wave_slot = __builtin_amdgcn_readfirstlane(slot);
    const uint32_t first = bounds[0];
    auto channel_of = [&](uint32_t p) -> int {
        if (CAND) return cand[p - first];
        return candidate_channel(ph, p, solid_map, det, detection_state);
    };
    auto head = [&](uint32_t e) -> int {
        const uint32_t b0 = bounds[e], lim = min(cap, bounds[e + 1] - b0);
        if (wave_slot >= lim) return -1;
        return slot < lim ? channel_of(b0 + slot) : -1;
    };
    chr_xorwow rng;
    bool loaded = false;
    int next = head(0);
    for (uint32_t e = 0; e < nevents; ++e) {
        int channel_index = next;
        if (e + 1 < nevents) next = head(e + 1);
        const uint32_t b0 = bounds[e], n = bounds[e + 1] - b0, lim = min(cap, n);
        if (wave_slot >= lim) continue;
        if (slot >= lim) continue;
        const size_t row = (size_t)e * (uint32_t)det.nchannels;
        for (uint32_t pos = slot; pos < n; pos += cap) {
            if (pos != slot) channel_index = channel_of(b0 + pos);
            if (channel_index < 0) continue;
            if (!loaded) { load_rng(rng_states, nslots, slot, rng); loaded = true; }
            const size_t w = row + (uint32_t)channel_index;
            float pe_time;
            uint32_t pe_q;
            const bool accepted = draw_hit(rng, ph, b0 + pos, ph.flags[b0 + pos], det, global_weight, time_int + w,
                                           q_int + w, hist + w, pe_time, pe_q);
            if (PE && accepted) {
                const uint32_t i = b0 + pos - first;
                pe.channel[i] = channel_index;
                pe.time[i] = pe_time;
                pe.q[i] = pe_q;
            }
        }
    }
    if (loaded) store_rng(rng_states, nslots, slot, rng);
}

// convert_charge_int_to_float (daq.cu:164-172) over every row
__global__ __launch_bounds__(BLOCK) void convert_charge_kernel(const uint32_t *q_int, float *q, uint32_t n,
                                                               float charge_unit) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) q[i] = (float)q_int[i] * charge_unit;
}

// Device and pinned host words for the event bounds, and the candidate words of shape (b)
// (per host thread and device, grown on demand).
struct EventBuffers {
    uint32_t *d_bounds = nullptr, *h_bounds = nullptr;
    int32_t *d_cand = nullptr;
    size_t nbounds = 0, ncand = 0;
};

int event_buffers(size_t nbounds, size_t ncand, EventBuffers **out) {
    static thread_local EventBuffers s[16];
    int dev = 0;
    CHR_HIP_CHECK(hipGetDevice(&dev));
    EventBuffers &x = s[dev & 15];
    if (x.nbounds < nbounds) {
        if (x.d_bounds) CHR_HIP_CHECK(hipFree(x.d_bounds));
        x.d_bounds = nullptr;
        if (x.h_bounds) CHR_HIP_CHECK(hipHostFree(x.h_bounds));
        x.h_bounds = nullptr;
        x.nbounds = 0;
        const size_t grown = nbounds + nbounds / 2;
        CHR_HIP_CHECK(hipMalloc((void **)&x.d_bounds, grown * 4));
        CHR_HIP_CHECK(hipHostMalloc((void **)&x.h_bounds, grown * 4, hipHostMallocDefault));
        x.nbounds = grown;
    }
    if (x.ncand < ncand) {
        if (x.d_cand) CHR_HIP_CHECK(hipFree(x.d_cand));
        x.d_cand = nullptr;
        x.ncand = 0;
        const size_t grown = ncand + ncand / 2;
        CHR_HIP_CHECK(hipMalloc((void **)&x.d_cand, grown * 4));
        x.ncand = grown;
    }
    *out = &x;
    return CHR_OK;
}

// CHR_DAQ_EVENTS_SHAPE=a: one kernel that computes each event's candidate word one event
// ahead of the draws (A/B; default b: the parallel candidate pass, then the draws)
static bool events_candidate_pass() {
    const char *e = getenv("CHR_DAQ_EVENTS_SHAPE");
    return !(e && e[0] == 'a');
}

// daq.cu:85-145: one photon per workgroup of `ntpb` slots; workgroup b runs
// photons b, b+max_blocks, ... (the reference's successive chunks)
__global__ void run_daq_many_kernel(uint32_t *rng_states, uint32_t nslots, uint32_t *normal_cache,
                                    uint32_t detection_state, int32_t start, uint32_t n, uint32_t max_blocks,
                                    DaqPhotons ph, const uint32_t *solid_map, chr_daq_detector det,
                                    uint32_t *time_int, uint32_t *q_int, uint32_t *hist, int32_t ndaq,
                                    int32_t channel_stride, float global_weight) {
    const uint32_t b = blockIdx.x;
    const uint32_t slot = threadIdx.x + blockDim.x * b;
    chr_xorwow rng;
    uint32_t nflag = 0, nextra = 0;
    bool loaded = false;
    for (uint32_t pos = b; pos < n; pos += max_blocks) {
        const uint32_t photon_id = (uint32_t)start + pos;
        const int triangle_id = ph.last_hit[photon_id];
        // daq.cu:120-122; a wire-plane hit (-2) leaves the reference's shared
        // solid/channel words unset (UB): defined here as "not detected"
        if (triangle_id <= -1) continue;
        const int solid_id = (int)solid_map[triangle_id];
        const uint32_t history = ph.flags[photon_id];
        const int channel_index = det.d_solid_id_to_channel_index[solid_id];
        if (channel_index < 0 || !(history & detection_state)) continue;
        const float photon_time = ph.t[photon_id];
        const float weight = ph.weights[photon_id] * global_weight;
        if (!loaded) {
            load_rng(rng_states, nslots, slot, rng);
            nflag = normal_cache[slot];
            nextra = normal_cache[nslots + slot];
            loaded = true;
        }
        for (int i = (int)threadIdx.x; i < ndaq; i += (int)blockDim.x) {
            const int channel_offset = channel_index + i * channel_stride;
            if (chr_uniform01(&rng) < weight) {
                float time = photon_time + chr_normal(&rng, &nflag, &nextra);
                time = time + sample_cdf_xy(rng, det.time_cdf_len, det.d_time_cdf_x, det.d_time_cdf_y);
                const float charge = sample_cdf_xy(rng, det.charge_cdf_len, det.d_charge_cdf_x, det.d_charge_cdf_y);
                const uint32_t charge_int = chr_sat_u32(__builtin_roundf(charge / det.charge_unit));
                atomicMin(time_int + channel_offset, __float_as_uint(time));
                atomicAdd(q_int + channel_offset, charge_int);
                atomicOr(hist + channel_offset, history);
            }
        }
    }
    if (loaded) {
        store_rng(rng_states, nslots, slot, rng);
        normal_cache[slot] = nflag;
        normal_cache[nslots + slot] = nextra;
    }
}

// ---- ndaq > 1 for every event of a batch in one launch (chr_daq_acquire_events_many)

// The draws of run_daq_many_kernel for events e = 0 .. nevents-1 over photons
// [bounds[e], bounds[e+1]), into row e (ndaq copies of nchannels words) of the
// accumulators.  Only the slots that can draw are launched: slot (b, tid) = tid +
// ntpb*b with tid < tids = min(ntpb, ndaq) and b < nb = min(max_blocks, max n_e).
// `width` consecutive work-items share one b: tids rounded up to a power of two below
// a wave (several b per wave when ndaq < 64) or to whole waves above it, so a photon's
// candidate word, time, weight and history are uniform over the lanes that share a b.
// Slot (b, tid) takes part in event e iff b < min(max_blocks, n_e), visits positions
// b, b + max_blocks, ... there and draws for copies tid, tid + ntpb, ... of a detected
// photon; its xorwow state and normal-cache pair stay in registers from its first
// draw to the one store.  The event loop and its skip are wave-uniform (the wave's
// lowest b in an SGPR, bounds through uniform loads); the candidate word of the
// slot's first position is read one event ahead, as in run_daq_events_kernel.
__global__ __launch_bounds__(BLOCK) void run_daq_events_many_kernel(
    uint32_t *rng_states, uint32_t nslots, uint32_t *normal_cache, const uint32_t *__restrict__ bounds,
    uint32_t nevents, uint32_t ntpb, uint32_t max_blocks, uint32_t tids, uint32_t width, uint32_t nb, DaqPhotons ph,
    chr_daq_detector det, const int32_t *__restrict__ cand, uint32_t *time_int, uint32_t *q_int, uint32_t *hist,
    uint32_t ndaq, float global_weight) {
    const uint32_t g = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t b = g / width, tid = g - b * width;
    const uint32_t wave_b = __builtin_amdgcn_readfirstlane(b);   // b ascends with g: the wave's lowest
    const bool mine = tid < tids && b < nb;
    const uint32_t slot = tid + ntpb * b;
    const uint32_t first = bounds[0];
    const uint32_t nch = (uint32_t)det.nchannels;
    auto head = [&](uint32_t e) -> int {
        const uint32_t b0 = bounds[e], lim = min(max_blocks, bounds[e + 1] - b0);
        if (wave_b >= lim) return -1;
        return mine && b < lim ? cand[b0 - first + b] : -1;
    };
    chr_xorwow rng;
    uint32_t nflag = 0, nextra = 0;
    bool loaded = false;
    int next = head(0);
    for (uint32_t e = 0; e < nevents; ++e) {
        int channel_index = next;
        if (e + 1 < nevents) next = head(e + 1);
        const uint32_t b0 = bounds[e], n = bounds[e + 1] - b0, lim = min(max_blocks, n);
        if (wave_b >= lim) continue;
        if (!mine || b >= lim) continue;
        const size_t row = (size_t)e * ndaq * nch;
        for (uint32_t pos = b; pos < n; pos += max_blocks) {
            if (pos != b) channel_index = cand[b0 - first + pos];
            if (channel_index < 0) continue;
            const uint32_t photon_id = b0 + pos;
            const float photon_time = ph.t[photon_id];
            const float weight = ph.weights[photon_id] * global_weight;
            const uint32_t history = ph.flags[photon_id];
            if (!loaded) {
                load_rng(rng_states, nslots, slot, rng);
                nflag = normal_cache[slot];
                nextra = normal_cache[nslots + slot];
                loaded = true;
            }
            for (uint32_t i = tid; i < ndaq; i += ntpb) {
                if (chr_uniform01(&rng) < weight) {
                    float time = photon_time + chr_normal(&rng, &nflag, &nextra);
                    time = time + sample_cdf_xy(rng, det.time_cdf_len, det.d_time_cdf_x, det.d_time_cdf_y);
                    const float charge =
                        sample_cdf_xy(rng, det.charge_cdf_len, det.d_charge_cdf_x, det.d_charge_cdf_y);
                    const uint32_t charge_int = chr_sat_u32(__builtin_roundf(charge / det.charge_unit));
                    const size_t w = row + (size_t)i * nch + (uint32_t)channel_index;
                    atomicMin(time_int + w, __float_as_uint(time));
                    atomicAdd(q_int + w, charge_int);
                    atomicOr(hist + w, history);
                }
            }
        }
    }
    if (loaded) {
        store_rng(rng_states, nslots, slot, rng);
        normal_cache[slot] = nflag;
        normal_cache[nslots + slot] = nextra;
    }
}

// what chr_daq_end and begin_acquire's fill leave in the float charges of every row of
// `row_words` = ndaq*nchannels words: the first nchannels converted, the rest 0
__global__ __launch_bounds__(BLOCK) void convert_charge_rows_kernel(const uint32_t *q_int, float *q, uint32_t n,
                                                                    uint32_t row_words, uint32_t nchannels,
                                                                    float charge_unit) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) q[i] = (i % row_words) < nchannels ? (float)q_int[i] * charge_unit : 0.0f;
}

// daq.cu:147-172
__global__ __launch_bounds__(BLOCK) void end_kernel(const uint32_t *time_int, float *time, const uint32_t *q_int,
                                                    float *q, uint32_t n, int32_t nchannels, float charge_unit) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    time[i] = __uint_as_float(time_int[i]);
    if ((int32_t)i < nchannels) q[i] = (float)q_int[i] * charge_unit;
}

// detected photons per channel (the selection of count_photon_hits,
// propagate.cu:172-199, histogrammed by channel): the per-rank array that the
// photon-sharded run reduces over RCCL
__global__ __launch_bounds__(BLOCK) void channel_counts_kernel(const uint32_t *flags, const int32_t *last_hit,
                                                               int32_t start, uint32_t n, uint32_t detection_state,
                                                               const uint32_t *solid_map, const int32_t *s2c,
                                                               int32_t nchannels, uint32_t *counts) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = (uint32_t)start + i;
    if (!(flags[p] & detection_state)) return;
    const int tri = last_hit[p];
    if (tri <= -1) return;
    const int c = s2c[solid_map[tri]];
    if (c >= 0 && c < nchannels) atomicAdd(counts + c, 1u);
}

inline unsigned grid_for(uint64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

}  // namespace chr_daq

using namespace chr_daq;

extern "C" int chr_daq_begin(uint32_t *d_time_int, uint32_t *d_q_int, uint32_t *d_history, uint32_t n, float maxtime,
                             void *stream) {
    if (!d_time_int || !d_q_int || !d_history) return chr::fail(CHR_ERR_INVALID, "chr_daq_begin: null argument");
    if (n == 0) return CHR_OK;
    hipLaunchKernelGGL(begin_kernel, dim3(grid_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, d_time_int, d_q_int,
                       d_history, n, __builtin_bit_cast(uint32_t, maxtime));
    CHR_HIP_CHECK(hipGetLastError());
    return CHR_OK;
}

extern "C" int chr_daq_acquire(const chr_photons *ph, uint32_t *d_rng_states, uint32_t rng_nslots,
                               uint32_t *d_normal_cache, uint32_t detection_state, int32_t start_photon,
                               int32_t nphotons, const uint32_t *d_solid_map, const chr_daq_detector *det,
                               uint32_t *d_time_int, uint32_t *d_q_int, uint32_t *d_history, int32_t ndaq,
                               int32_t stride, float global_weight, int32_t ntpb, int32_t max_blocks, void *vstream) {
    if (!ph || !ph->d_t || !ph->d_flags || !ph->d_last_hit_triangles || !ph->d_weights || !d_rng_states ||
        !d_solid_map || !det || !det->d_solid_id_to_channel_index || !d_time_int || !d_q_int || !d_history)
        return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire: null argument");
    if (!det->d_time_cdf_x || !det->d_time_cdf_y || !det->d_charge_cdf_x || !det->d_charge_cdf_y ||
        det->time_cdf_len < 2 || det->charge_cdf_len < 2)
        return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire: time/charge CDFs missing");
    if (ndaq < 1 || ntpb <= 0 || max_blocks <= 0 || start_photon < 0)
        return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire: bad ndaq / launch shape");
    if (nphotons <= 0) return CHR_OK;
    hipStream_t stream = (hipStream_t)vstream;
    DaqPhotons p{ph->d_t, ph->d_weights, ph->d_flags, ph->d_last_hit_triangles};
    if (ndaq == 1) {
        const uint64_t cap = (uint64_t)ntpb * max_blocks;
        if (cap > rng_nslots && (uint64_t)nphotons > rng_nslots)
            return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire: %d photons per chunk but only %u rng states",
                             (int)std::min<uint64_t>(cap, nphotons), rng_nslots);
        const uint32_t threads = (uint32_t)std::min<uint64_t>(cap, (uint64_t)nphotons);
        hipLaunchKernelGGL(run_daq_kernel, dim3(grid_for(threads)), dim3(BLOCK), 0, stream, d_rng_states, rng_nslots,
                           detection_state, start_photon, (uint32_t)nphotons, (uint32_t)std::min<uint64_t>(cap, 0xFFFFFFFFu),
                           p, d_solid_map, *det, d_time_int, d_q_int, d_history, global_weight);
    } else {
        if (!d_normal_cache) return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire: ndaq > 1 needs the normal cache");
        if (ntpb > 1024) return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire: nthreads_per_block > 1024");
        const uint32_t blocks = (uint32_t)std::min<int64_t>(max_blocks, nphotons);
        if ((uint64_t)ntpb * blocks > rng_nslots)
            return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire: %u slots needed, %u rng states",
                             (unsigned)(ntpb * blocks), rng_nslots);
        if (stride < 0) return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire: negative stride");
        hipLaunchKernelGGL(run_daq_many_kernel, dim3(blocks), dim3(ntpb), 0, stream, d_rng_states, rng_nslots,
                           d_normal_cache, detection_state, start_photon, (uint32_t)nphotons, (uint32_t)max_blocks, p,
                           d_solid_map, *det, d_time_int, d_q_int, d_history, ndaq, stride, global_weight);
    }
    CHR_HIP_CHECK(hipGetLastError());
    CHR_HIP_CHECK(hipStreamSynchronize(stream));   // daq.py:91
    return CHR_OK;
}

extern "C" int chr_daq_end(const uint32_t *d_time_int, float *d_time, const uint32_t *d_q_int, float *d_q, uint32_t n,
                           int32_t nchannels, float charge_unit, void *stream) {
    if (!d_time_int || !d_time || !d_q_int || !d_q) return chr::fail(CHR_ERR_INVALID, "chr_daq_end: null argument");
    if (n == 0) return CHR_OK;
    hipLaunchKernelGGL(end_kernel, dim3(grid_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, d_time_int, d_time, d_q_int,
                       d_q, n, nchannels, charge_unit);
    CHR_HIP_CHECK(hipGetLastError());
    CHR_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return CHR_OK;
}

// chr_daq_acquire_events (pe null) and chr_daq_acquire_events_pe (pe: the three record
// arrays): one text for the refusals, the walk and the launches
static int acquire_events(const char *who, const chr_photons *ph, int32_t nphotons, const int64_t *h_bounds,
                          int32_t nevents, uint32_t *d_rng_states, uint32_t rng_nslots, uint32_t detection_state,
                          const uint32_t *d_solid_map, const chr_daq_detector *det, uint32_t *d_time_int,
                          uint32_t *d_q_int, uint32_t *d_history, float *d_q, float global_weight, int32_t ntpb,
                          int32_t max_blocks, void *vstream, const PeRecords *pe) {
    if (pe && (!pe->channel || !pe->time || !pe->q))
        return chr::fail(CHR_ERR_INVALID, "%s: null photoelectron array", who);
    if (!ph || !ph->d_t || !ph->d_flags || !ph->d_last_hit_triangles || !ph->d_weights || !h_bounds ||
        !d_rng_states || !d_solid_map || !det || !det->d_solid_id_to_channel_index || !d_time_int || !d_q_int ||
        !d_history || !d_q)
        return chr::fail(CHR_ERR_INVALID, "%s: null argument", who);
    if (!det->d_time_cdf_x || !det->d_time_cdf_y || !det->d_charge_cdf_x || !det->d_charge_cdf_y ||
        det->time_cdf_len < 2 || det->charge_cdf_len < 2)
        return chr::fail(CHR_ERR_INVALID, "%s: time/charge CDFs missing", who);
    if (nevents < 0 || nphotons < 0 || ntpb <= 0 || max_blocks <= 0 || det->nchannels <= 0)
        return chr::fail(CHR_ERR_INVALID, "%s: bad event count / launch shape / channel count", who);
    if (h_bounds[0] < 0 || h_bounds[nevents] > nphotons)
        return chr::fail(CHR_ERR_INVALID, "%s: bounds [%lld, %lld] outside the %d photons", who,
                         (long long)h_bounds[0], (long long)h_bounds[nevents], nphotons);
    int64_t max_n = 0;
    for (int32_t e = 0; e < nevents; ++e) {
        if (h_bounds[e + 1] < h_bounds[e])
            return chr::fail(CHR_ERR_INVALID, "%s: bounds decrease at event %d", who, e);
        max_n = std::max(max_n, h_bounds[e + 1] - h_bounds[e]);
    }
    // positions stay below 2^31, so a larger cap visits the same ones (and pos + cap cannot wrap)
    const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)ntpb * max_blocks, 0x80000000u);
    const uint32_t threads = (uint32_t)std::min<int64_t>(cap, max_n);
    if (threads > rng_nslots)
        return chr::fail(CHR_ERR_INVALID, "%s: %u photons per chunk but only %u rng states", who,
                         threads, rng_nslots);
    const uint64_t words = (uint64_t)nevents * (uint32_t)det->nchannels;
    if (words > 0x80000000u)
        return chr::fail(CHR_ERR_INVALID, "%s: %d events of %d channels exceed 2^31 words", who,
                         nevents, det->nchannels);
    if (nevents == 0) return CHR_OK;

    hipStream_t stream = (hipStream_t)vstream;
    hipLaunchKernelGGL(begin_kernel, dim3(grid_for(words)), dim3(BLOCK), 0, stream, d_time_int, d_q_int, d_history,
                       (uint32_t)words, __builtin_bit_cast(uint32_t, 1e9f));
    CHR_HIP_CHECK(hipGetLastError());
    if (threads > 0) {
        const bool pass = pe || events_candidate_pass();     // the photoelectron variant is shape (b) always
        const uint32_t first = (uint32_t)h_bounds[0], span = (uint32_t)(h_bounds[nevents] - h_bounds[0]);
        EventBuffers *buf = nullptr;
        CHR_TRY(event_buffers((size_t)nevents + 1, pass ? span : 0, &buf));
        for (int32_t e = 0; e <= nevents; ++e) buf->h_bounds[e] = (uint32_t)h_bounds[e];
        CHR_HIP_CHECK(hipMemcpyAsync(buf->d_bounds, buf->h_bounds, ((size_t)nevents + 1) * 4, hipMemcpyHostToDevice,
                                     stream));
        DaqPhotons p{ph->d_t, ph->d_weights, ph->d_flags, ph->d_last_hit_triangles};
        const PeRecords none{nullptr, nullptr, nullptr};
        if (pe) {
            hipLaunchKernelGGL(candidates_pe_kernel, dim3(grid_for(span)), dim3(BLOCK), 0, stream, p, first, span,
                               d_solid_map, *det, detection_state, buf->d_cand, *pe);
            CHR_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL((run_daq_events_kernel<true, true>), dim3(grid_for(threads)), dim3(BLOCK), 0, stream,
                               d_rng_states, rng_nslots, detection_state, buf->d_bounds, (uint32_t)nevents, cap, p,
                               d_solid_map, *det, buf->d_cand, d_time_int, d_q_int, d_history, global_weight, *pe);
        } else if (pass) {
            hipLaunchKernelGGL(candidates_kernel, dim3(grid_for(span)), dim3(BLOCK), 0, stream, p, first, span,
                               d_solid_map, *det, detection_state, buf->d_cand);
            CHR_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL((run_daq_events_kernel<true, false>), dim3(grid_for(threads)), dim3(BLOCK), 0, stream,
                               d_rng_states, rng_nslots, detection_state, buf->d_bounds, (uint32_t)nevents, cap, p,
                               d_solid_map, *det, buf->d_cand, d_time_int, d_q_int, d_history, global_weight, none);
        } else {
            hipLaunchKernelGGL((run_daq_events_kernel<false, false>), dim3(grid_for(threads)), dim3(BLOCK), 0, stream,
                               d_rng_states, rng_nslots, detection_state, buf->d_bounds, (uint32_t)nevents, cap, p,
                               d_solid_map, *det, (const int32_t *)nullptr, d_time_int, d_q_int, d_history,
                               global_weight, none);
        }
        CHR_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(convert_charge_kernel, dim3(grid_for(words)), dim3(BLOCK), 0, stream, d_q_int, d_q,
                       (uint32_t)words, det->charge_unit);
    CHR_HIP_CHECK(hipGetLastError());
    // the pinned bounds are rewritten by the next call, and GPUDaq.acquire synchronises too (daq.py:91)
    CHR_HIP_CHECK(hipStreamSynchronize(stream));
    return CHR_OK;
}

extern "C" int chr_daq_acquire_events(const chr_photons *ph, int32_t nphotons, const int64_t *h_bounds,
                                      int32_t nevents, uint32_t *d_rng_states, uint32_t rng_nslots,
                                      uint32_t detection_state, const uint32_t *d_solid_map,
                                      const chr_daq_detector *det, uint32_t *d_time_int, uint32_t *d_q_int,
                                      uint32_t *d_history, float *d_q, float global_weight, int32_t ntpb,
                                      int32_t max_blocks, void *stream) {
    return acquire_events("chr_daq_acquire_events", ph, nphotons, h_bounds, nevents, d_rng_states, rng_nslots,
                          detection_state, d_solid_map, det, d_time_int, d_q_int, d_history, d_q, global_weight, ntpb,
                          max_blocks, stream, nullptr);
}

extern "C" int chr_daq_acquire_events_pe(const chr_photons *ph, int32_t nphotons, const int64_t *h_bounds,
                                         int32_t nevents, uint32_t *d_rng_states, uint32_t rng_nslots,
                                         uint32_t detection_state, const uint32_t *d_solid_map,
                                         const chr_daq_detector *det, uint32_t *d_time_int, uint32_t *d_q_int,
                                         uint32_t *d_history, float *d_q, int32_t *d_pe_channel, float *d_pe_time,
                                         uint32_t *d_pe_q, float global_weight, int32_t ntpb, int32_t max_blocks,
                                         void *stream) {
    const PeRecords pe{d_pe_channel, d_pe_time, d_pe_q};
    return acquire_events("chr_daq_acquire_events_pe", ph, nphotons, h_bounds, nevents, d_rng_states, rng_nslots,
                          detection_state, d_solid_map, det, d_time_int, d_q_int, d_history, d_q, global_weight, ntpb,
                          max_blocks, stream, &pe);
}

extern "C" int chr_daq_acquire_events_many(const chr_photons *ph, int32_t nphotons, const int64_t *h_bounds,
                                           int32_t nevents, uint32_t *d_rng_states, uint32_t rng_nslots,
                                           uint32_t *d_normal_cache, uint32_t detection_state,
                                           const uint32_t *d_solid_map, const chr_daq_detector *det,
                                           uint32_t *d_time_int, uint32_t *d_q_int, uint32_t *d_history, float *d_q,
                                           int32_t ndaq, float global_weight, int32_t ntpb, int32_t max_blocks,
                                           void *vstream) {
    if (!ph || !ph->d_t || !ph->d_flags || !ph->d_last_hit_triangles || !ph->d_weights || !h_bounds ||
        !d_rng_states || !d_normal_cache || !d_solid_map || !det || !det->d_solid_id_to_channel_index ||
        !d_time_int || !d_q_int || !d_history || !d_q)
        return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire_events_many: null argument");
    if (!det->d_time_cdf_x || !det->d_time_cdf_y || !det->d_charge_cdf_x || !det->d_charge_cdf_y ||
        det->time_cdf_len < 2 || det->charge_cdf_len < 2)
        return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire_events_many: time/charge CDFs missing");
    if (ndaq < 2)
        return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire_events_many: ndaq = %d (chr_daq_acquire_events runs ndaq = 1)",
                         ndaq);
    if (nevents < 0 || nphotons < 0 || ntpb <= 0 || max_blocks <= 0 || det->nchannels <= 0)
        return chr::fail(CHR_ERR_INVALID,
                         "chr_daq_acquire_events_many: bad event count / launch shape / channel count");
    if (ntpb > 1024) return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire_events_many: nthreads_per_block > 1024");
    if (h_bounds[0] < 0 || h_bounds[nevents] > nphotons)
        return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire_events_many: bounds [%lld, %lld] outside the %d photons",
                         (long long)h_bounds[0], (long long)h_bounds[nevents], nphotons);
    int64_t max_n = 0;
    for (int32_t e = 0; e < nevents; ++e) {
        if (h_bounds[e + 1] < h_bounds[e])
            return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire_events_many: bounds decrease at event %d", e);
        max_n = std::max(max_n, h_bounds[e + 1] - h_bounds[e]);
    }
    // the slots of the per-event launches: blocks b < min(max_blocks, n_e) of ntpb each
    const uint32_t nb = (uint32_t)std::min<int64_t>(max_blocks, max_n);
    if ((uint64_t)ntpb * nb > rng_nslots)
        return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire_events_many: %llu slots needed, %u rng states",
                         (unsigned long long)ntpb * nb, rng_nslots);
    const uint64_t row_words = (uint64_t)ndaq * (uint32_t)det->nchannels;
    if (nevents > 0 && row_words > 0x80000000u / (uint32_t)nevents)      // the product may not fit 64 bits
        return chr::fail(CHR_ERR_INVALID,
                         "chr_daq_acquire_events_many: %d events of %d copies of %d channels exceed 2^31 words",
                         nevents, ndaq, det->nchannels);
    const uint64_t words = (uint64_t)nevents * row_words;
    // only the work-items that can draw: tid < min(ntpb, ndaq); `width` of them share a b
    const uint32_t tids = (uint32_t)std::min(ntpb, ndaq);
    uint32_t width = 1;
    if (tids >= 64) width = (tids + 63u) & ~63u;
    else while (width < tids) width <<= 1;
    if ((uint64_t)nb * width > 0xFFFFFF00u)      // width < 2 * ntpb: only with more than 2^31 rng states
        return chr::fail(CHR_ERR_INVALID, "chr_daq_acquire_events_many: %u blocks of %u work-items exceed one launch",
                         nb, width);
    if (nevents == 0) return CHR_OK;

    hipStream_t stream = (hipStream_t)vstream;
    hipLaunchKernelGGL(begin_kernel, dim3(grid_for(words)), dim3(BLOCK), 0, stream, d_time_int, d_q_int, d_history,
                       (uint32_t)words, __builtin_bit_cast(uint32_t, 1e9f));
    CHR_HIP_CHECK(hipGetLastError());
    if (nb > 0) {
        const uint32_t first = (uint32_t)h_bounds[0], span = (uint32_t)(h_bounds[nevents] - h_bounds[0]);
        EventBuffers *buf = nullptr;
        CHR_TRY(event_buffers((size_t)nevents + 1, span, &buf));
        for (int32_t e = 0; e <= nevents; ++e) buf->h_bounds[e] = (uint32_t)h_bounds[e];
        CHR_HIP_CHECK(hipMemcpyAsync(buf->d_bounds, buf->h_bounds, ((size_t)nevents + 1) * 4, hipMemcpyHostToDevice,
                                     stream));
        DaqPhotons p{ph->d_t, ph->d_weights, ph->d_flags, ph->d_last_hit_triangles};
        hipLaunchKernelGGL(candidates_kernel, dim3(grid_for(span)), dim3(BLOCK), 0, stream, p, first, span,
                           d_solid_map, *det, detection_state, buf->d_cand);
        CHR_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(run_daq_events_many_kernel, dim3(grid_for((uint64_t)nb * width)), dim3(BLOCK), 0, stream,
                           d_rng_states, rng_nslots, d_normal_cache, buf->d_bounds, (uint32_t)nevents, (uint32_t)ntpb,
                           (uint32_t)max_blocks, tids, width, nb, p, *det, buf->d_cand, d_time_int, d_q_int,
                           d_history, (uint32_t)ndaq, global_weight);
        CHR_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(convert_charge_rows_kernel, dim3(grid_for(words)), dim3(BLOCK), 0, stream, d_q_int, d_q,
                       (uint32_t)words, (uint32_t)row_words, (uint32_t)det->nchannels, det->charge_unit);
    CHR_HIP_CHECK(hipGetLastError());
    // the pinned bounds are rewritten by the next call, and GPUDaq.acquire synchronises too (daq.py:91)
    CHR_HIP_CHECK(hipStreamSynchronize(stream));
    return CHR_OK;
}

extern "C" int chr_channel_hit_counts(const chr_photons *ph, int32_t start_photon, int32_t nphotons,
                                      uint32_t detection_state, const uint32_t *d_solid_map,
                                      const int32_t *d_solid_id_to_channel_index, uint32_t *d_counts,
                                      int32_t nchannels, void *stream) {
    if (!ph || !ph->d_flags || !ph->d_last_hit_triangles || !d_solid_map || !d_solid_id_to_channel_index || !d_counts)
        return chr::fail(CHR_ERR_INVALID, "chr_channel_hit_counts: null argument");
    if (nphotons <= 0 || nchannels <= 0) return CHR_OK;
    hipLaunchKernelGGL(channel_counts_kernel, dim3(grid_for((uint32_t)nphotons)), dim3(BLOCK), 0, (hipStream_t)stream,
                       ph->d_flags, ph->d_last_hit_triangles, start_photon, (uint32_t)nphotons, detection_state,
                       d_solid_map, d_solid_id_to_channel_index, nchannels, d_counts);
    CHR_HIP_CHECK(hipGetLastError());
    return CHR_OK;
}
