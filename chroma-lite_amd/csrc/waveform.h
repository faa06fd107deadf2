// waveform.h -- charge trains and digitised waveforms of the photoelectron records
// chr_daq_acquire_events_pe leaves (include/chroma_amd.h, "waveforms"): what one
// photoelectron adds to the trains and what one sample of a row digitises to,
// decided by one text for the gfx950 kernels (waveform.hip) and their host twins
// (waveform_host.cpp, the host compiler).  CHR_FN code over chroma_fmath.h only.
// The functions work out the words; the callers only add or store them, the
// device with integer atomics, the host with plain integers, so trains are a
// function of the records alone.  The time bin is hitmap.h's (one float subtract
// and one float multiply, separately rounded); the digitiser's multiply-adds are
// single-rounded chr_fmaf (-ffp-contract=off on both sides).
#ifndef CHROMA_WAVEFORM_H
#define CHROMA_WAVEFORM_H

#include "../../include/chroma_amd.h"
#include "../../include/chroma_fmath.h"
#include "hitmap.h"

// the scalar part of a chr_daq_pe_trains call
typedef struct chr_wave_par {
    uint32_t nevents, nchannels, nrows, nsamples;
    float t_lo, inv;
} chr_wave_par;

// the records and what places them; bounds[0 .. nevents] are the events' photon
// offsets, the records are indexed from bounds[0]
typedef struct chr_wave_inputs {
    const int32_t *pe_channel;
    const float *pe_time;
    const uint32_t *pe_q;
    const uint32_t *bounds;
    const int32_t *row_of_word;       // null: row = event * nchannels + channel
} chr_wave_inputs;

#define CHR_WAVE_NONE 0      /* no photoelectron in this record */
#define CHR_WAVE_DROPPED 1   /* a photoelectron without a row: dropped += 1 */
#define CHR_WAVE_INSIDE 2    /* trains[word] += q */
#define CHR_WAVE_OUTSIDE 3   /* outside_q[word] += q */

typedef struct chr_wave_update {
    uint32_t word;       // INSIDE: row * nsamples + bin; OUTSIDE: row
    uint32_t q;
} chr_wave_update;

// step 2: the event of span position i, the e with bounds[e] <= bounds[0] + i < bounds[e+1]
// (events without photons are passed over); i is below the span
CHR_FN uint32_t chr_wave_event(const uint32_t *bounds, uint32_t nevents, uint32_t i) {
    const uint32_t p = bounds[0] + i;
    uint32_t lo = 0u, hi = nevents;           // bounds[lo] <= p < bounds[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (bounds[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// Rule steps 1-5 for record i of the span; fills *u for INSIDE and OUTSIDE.
CHR_FN int chr_wave_pe(const chr_wave_par *par, const chr_wave_inputs *in, uint32_t i, chr_wave_update *u) {
    const int32_t c = in->pe_channel[i];
    if (c < 0) return CHR_WAVE_NONE;
    if ((uint32_t)c >= par->nchannels) return CHR_WAVE_DROPPED;
    const uint32_t e = chr_wave_event(in->bounds, par->nevents, i);
    const uint32_t w = e * par->nchannels + (uint32_t)c;
    const int32_t row = in->row_of_word ? in->row_of_word[w] : (int32_t)w;
    if (row < 0 || (uint32_t)row >= par->nrows) return CHR_WAVE_DROPPED;
    u->q = in->pe_q[i];
    const int32_t b = chr_hitmap_time_bin(in->pe_time[i], par->t_lo, par->inv, par->nsamples);
    if (b >= 0) {
        u->word = (uint32_t)row * par->nsamples + (uint32_t)b;
        return CHR_WAVE_INSIDE;
    }
    u->word = (uint32_t)row;
    return CHR_WAVE_OUTSIDE;
}

// the scalar part of a chr_daq_digitise call
typedef struct chr_digitise_par {
    uint32_t nrows, nsamples, ntaps;
    float scale, pedestal;
    uint32_t adc_max;
} chr_digitise_par;

// Digitiser steps 2-3: the convolution at sample s of one row's train, taps ascending
CHR_FN float chr_wave_convolve(const uint32_t *train, const float *taps, uint32_t ntaps, uint32_t s) {
    float v = 0.0f;
    const uint32_t last = ntaps - 1u < s ? ntaps - 1u : s;
    for (uint32_t k = 0u; k <= last; ++k) v = chr_fmaf(taps[k], (float)train[s - k], v);
    return v;
}

// Digitiser steps 4-5: the ADC word of the convolved value; *bad counts a NaN
CHR_FN uint16_t chr_wave_adc(float v, const chr_digitise_par *par, uint32_t *bad) {
    const float x = chr_fmaf(v, par->scale, par->pedestal);
    if (chr_isnan(x)) {
        *bad += 1u;
        return 0u;
    }
    const uint32_t a = chr_sat_u32(x + 0.5f);
    return (uint16_t)(a < par->adc_max ? a : par->adc_max);
}

#ifdef __cplusplus
namespace chr {
// The refusals the device entries and their host twins share (waveform_host.cpp), made
// before anything is read through a pointer of the records, the trains or the template;
// they fill *par, and trains_check *span = bounds[nevents] - bounds[0] as well.
int trains_check(const char *who, const int32_t *pe_channel, const float *pe_time, const uint32_t *pe_q,
                 const int64_t *h_bounds, int32_t nevents, int32_t nchannels, uint32_t nrows, float t_lo, float inv,
                 uint32_t nsamples, const uint32_t *trains, const uint32_t *outside_q, const uint32_t *dropped,
                 chr_wave_par *par, uint32_t *span);
int digitise_check(const char *who, const uint32_t *trains, uint32_t nrows, uint32_t nsamples, const float *taps,
                   uint32_t ntaps, float scale, float pedestal, uint32_t adc_max, const uint16_t *adc,
                   const uint32_t *bad, chr_digitise_par *par);
}  // namespace chr
#endif

#endif /* CHROMA_WAVEFORM_H */
