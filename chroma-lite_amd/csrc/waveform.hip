// waveform.hip -- gfx950 charge trains and digitiser (chr_daq_pe_trains, chr_daq_digitise).
//
// The rules are waveform.h's (shared with the host twins); this file only decides
// where each word is added or stored.
//
//  trains    one work-item per photoelectron record of the span.  A record's event is
//            found by bisection of the event bounds (a few uniform-ish loads of an
//            L2-resident array); its charge word goes to the train word of its time
//            bin, or to the row's outside word, with one global integer atomic.  The
//            records of one event and channel are spread over a whole event of photons
//            and a row of a zero-suppressed read-out belongs to no workgroup, so the
//            adds are not staged in LDS; integer sums give the same words in any order.
//  digitise  one wave (a workgroup of 64) per row.  The row's train and the taps a
//            sample can reach are staged in LDS; lane l digitises samples l, l + 64, ...
//            and the wave stores consecutive u16 words.  A row that holds no charge is
//            found while it is staged (one wave-wide OR) and takes the pedestal word
//            without the convolution.  Rows are independent; no wave waits for another.
//
// All loops are bounded by the span, the row and the taps.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "waveform.h"

namespace chr_wave {

constexpr int BLOCK = 256;
constexpr int WAVE = 64;

__global__ __launch_bounds__(BLOCK) void trains_kernel(chr_wave_inputs in, chr_wave_par par, uint32_t span,
                                                       uint32_t *trains, uint32_t *outside_q, uint32_t *dropped) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= span) return;
    chr_wave_update u;
    switch (chr_wave_pe(&par, &in, i, &u)) {
        case CHR_WAVE_DROPPED: atomicAdd(dropped, 1u); break;
        case CHR_WAVE_INSIDE: atomicAdd(trains + u.word, u.q); break;
        case CHR_WAVE_OUTSIDE: atomicAdd(outside_q + u.word, u.q); break;
        default: break;
    }
}

// LDS: nsamples train words, then par.ntaps (<= nsamples) taps
__global__ __launch_bounds__(WAVE) void digitise_kernel(const uint32_t *__restrict__ trains,
                                                        const float *__restrict__ taps, chr_digitise_par par,
                                                        uint16_t *__restrict__ adc, uint32_t *bad) {
    extern __shared__ uint32_t lds[];
    uint32_t *train = lds;
    float *tap = (float *)(lds + par.nsamples);
    const uint32_t row = blockIdx.x, lane = threadIdx.x;
    const uint32_t *src = trains + (size_t)row * par.nsamples;
    uint32_t any = 0u;
    for (uint32_t s = lane; s < par.nsamples; s += WAVE) {
        const uint32_t q = src[s];
        train[s] = q;
        any |= q;
    }
    for (uint32_t k = lane; k < par.ntaps; k += WAVE) tap[k] = taps[k];
    const int charged = __syncthreads_or(any != 0u);      // also the barrier after the staging
    uint16_t *dst = adc + (size_t)row * par.nsamples;
    uint32_t nbad = 0u;
    for (uint32_t s = lane; s < par.nsamples; s += WAVE)
        dst[s] = chr_wave_adc(charged ? chr_wave_convolve(train, tap, par.ntaps, s) : 0.0f, &par, &nbad);
    if (nbad) atomicAdd(bad, nbad);
}

// The event bounds as u32 on the device, through pinned host words (per host thread and
// device, grown on demand).
struct BoundsBuffer {
    uint32_t *d = nullptr, *h = nullptr;
    size_t n = 0;
};

int bounds_buffer(size_t n, BoundsBuffer **out) {
    static thread_local BoundsBuffer s[16];
    int dev = 0;
    CHR_HIP_CHECK(hipGetDevice(&dev));
    BoundsBuffer &x = s[dev & 15];
    if (x.n < n) {
        if (x.d) CHR_HIP_CHECK(hipFree(x.d));
        x.d = nullptr;
        if (x.h) CHR_HIP_CHECK(hipHostFree(x.h));
        x.h = nullptr;
        x.n = 0;
        const size_t grown = n + n / 2;
        CHR_HIP_CHECK(hipMalloc((void **)&x.d, grown * 4));
        CHR_HIP_CHECK(hipHostMalloc((void **)&x.h, grown * 4, hipHostMallocDefault));
        x.n = grown;
    }
    *out = &x;
    return CHR_OK;
}

inline unsigned grid_for(uint64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

}  // namespace chr_wave

using namespace chr_wave;

extern "C" int chr_daq_pe_trains(const int32_t *d_pe_channel, const float *d_pe_time, const uint32_t *d_pe_q,
                                 const int64_t *h_bounds, int32_t nevents, int32_t nchannels,
                                 const int32_t *d_row_of_word, uint32_t nrows, float t_lo, float inv,
                                 uint32_t nsamples, uint32_t *d_trains, uint32_t *d_outside_q, uint32_t *d_dropped,
                                 void *vstream) {
    chr_wave_par par;
    uint32_t span = 0;
    CHR_TRY(chr::trains_check("chr_daq_pe_trains", d_pe_channel, d_pe_time, d_pe_q, h_bounds, nevents, nchannels,
                              nrows, t_lo, inv, nsamples, d_trains, d_outside_q, d_dropped, &par, &span));
    if (!d_row_of_word && nrows != par.nevents * par.nchannels)
        return chr::fail(CHR_ERR_INVALID, "chr_daq_pe_trains: %u rows without a map of the %u words", nrows,
                         par.nevents * par.nchannels);
    hipStream_t stream = (hipStream_t)vstream;
    const size_t words = (size_t)nrows * nsamples;     // <= 2^31 (checked)
    if (words) CHR_HIP_CHECK(hipMemsetAsync(d_trains, 0, words * 4, stream));
    if (nrows) CHR_HIP_CHECK(hipMemsetAsync(d_outside_q, 0, (size_t)nrows * 4, stream));
    CHR_HIP_CHECK(hipMemsetAsync(d_dropped, 0, 4, stream));
    if (span > 0) {
        BoundsBuffer *buf = nullptr;
        CHR_TRY(bounds_buffer((size_t)nevents + 1, &buf));
        for (int32_t e = 0; e <= nevents; ++e) buf->h[e] = (uint32_t)h_bounds[e];
        CHR_HIP_CHECK(hipMemcpyAsync(buf->d, buf->h, ((size_t)nevents + 1) * 4, hipMemcpyHostToDevice, stream));
        const chr_wave_inputs in{d_pe_channel, d_pe_time, d_pe_q, buf->d, d_row_of_word};
        hipLaunchKernelGGL(trains_kernel, dim3(grid_for(span)), dim3(BLOCK), 0, stream, in, par, span, d_trains,
                           d_outside_q, d_dropped);
        CHR_HIP_CHECK(hipGetLastError());
    }
    // the pinned bounds are rewritten by the next call
    CHR_HIP_CHECK(hipStreamSynchronize(stream));
    return CHR_OK;
}

extern "C" int chr_daq_digitise(const uint32_t *d_trains, uint32_t nrows, uint32_t nsamples, const float *d_template,
                                uint32_t ntaps, float scale, float pedestal, uint32_t adc_max, uint16_t *d_adc,
                                uint32_t *d_bad, void *vstream) {
    chr_digitise_par par;
    CHR_TRY(chr::digitise_check("chr_daq_digitise", d_trains, nrows, nsamples, d_template, ntaps, scale, pedestal,
                                adc_max, d_adc, d_bad, &par));
    hipStream_t stream = (hipStream_t)vstream;
    CHR_HIP_CHECK(hipMemsetAsync(d_bad, 0, 4, stream));
    if (nrows == 0) return CHR_OK;
    const size_t lds_bytes = ((size_t)par.nsamples + par.ntaps) * 4;      // <= 4 * CHR_WAVE_LDS_WORDS (checked)
    hipLaunchKernelGGL(digitise_kernel, dim3(nrows), dim3(WAVE), lds_bytes, stream, d_trains, d_template, par, d_adc,
                       d_bad);
    CHR_HIP_CHECK(hipGetLastError());
    return CHR_OK;
}
