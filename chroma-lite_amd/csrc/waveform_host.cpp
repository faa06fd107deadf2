// waveform_host.cpp -- the host side of the charge trains and the digitiser: the
// refusals shared with the device entries (waveform.hip) and the host twins
// chr_daq_pe_trains_host and chr_daq_digitise_host (waveform.h's rules built by the
// host compiler: the device's words without a GPU).
#include <cstdint>
#include <vector>

#include "common.h"
#include "waveform.h"

int chr::trains_check(const char *who, const int32_t *pe_channel, const float *pe_time, const uint32_t *pe_q,
                      const int64_t *h_bounds, int32_t nevents, int32_t nchannels, uint32_t nrows, float t_lo,
                      float inv, uint32_t nsamples, const uint32_t *trains, const uint32_t *outside_q,
                      const uint32_t *dropped, chr_wave_par *par, uint32_t *span) {
    if (!pe_channel || !pe_time || !pe_q || !h_bounds || !trains || !outside_q || !dropped)
        return chr::fail(CHR_ERR_INVALID, "%s: null argument", who);
    if (nevents < 0 || nchannels <= 0)
        return chr::fail(CHR_ERR_INVALID, "%s: %d events of %d channels", who, nevents, nchannels);
    if (nsamples == 0) return chr::fail(CHR_ERR_INVALID, "%s: no samples", who);
    if (!chr_isfinite(t_lo) || !(chr_isfinite(inv) && inv > 0.0f))
        return chr::fail(CHR_ERR_INVALID, "%s: t_lo = %g must be finite, inv = %g finite and positive", who,
                         (double)t_lo, (double)inv);
    const uint64_t limit = 0x80000000ull;
    const uint64_t words = (uint64_t)nevents * (uint32_t)nchannels;
    if (words > limit)
        return chr::fail(CHR_ERR_INVALID, "%s: %d events of %d channels exceed 2^31 words", who, nevents, nchannels);
    if ((uint64_t)nrows * nsamples > limit)
        return chr::fail(CHR_ERR_INVALID, "%s: %u rows of %u samples exceed 2^31 train words", who, nrows, nsamples);
    if (h_bounds[0] < 0 || h_bounds[nevents] - h_bounds[0] >= (int64_t)limit || h_bounds[nevents] >= (int64_t)limit)
        return chr::fail(CHR_ERR_INVALID, "%s: bounds [%lld, %lld] outside 2^31 photons", who, (long long)h_bounds[0],
                         (long long)h_bounds[nevents]);
    for (int32_t e = 0; e < nevents; ++e)
        if (h_bounds[e + 1] < h_bounds[e])
            return chr::fail(CHR_ERR_INVALID, "%s: bounds decrease at event %d", who, e);
    *par = chr_wave_par{(uint32_t)nevents, (uint32_t)nchannels, nrows, nsamples, t_lo, inv};
    *span = (uint32_t)(h_bounds[nevents] - h_bounds[0]);
    return CHR_OK;
}

int chr::digitise_check(const char *who, const uint32_t *trains, uint32_t nrows, uint32_t nsamples, const float *taps,
                        uint32_t ntaps, float scale, float pedestal, uint32_t adc_max, const uint16_t *adc,
                        const uint32_t *bad, chr_digitise_par *par) {
    if (!trains || !taps || !adc || !bad) return chr::fail(CHR_ERR_INVALID, "%s: null argument", who);
    if (nsamples == 0 || ntaps == 0)
        return chr::fail(CHR_ERR_INVALID, "%s: %u samples, %u taps", who, nsamples, ntaps);
    if ((uint64_t)nrows * nsamples > 0x80000000ull)
        return chr::fail(CHR_ERR_INVALID, "%s: %u rows of %u samples exceed 2^31 train words", who, nrows, nsamples);
    // a sample reads taps 0 .. min(ntaps - 1, s): those beyond the row are never used
    const uint32_t used = ntaps < nsamples ? ntaps : nsamples;
    if ((uint64_t)nsamples + used > CHR_WAVE_LDS_WORDS)
        return chr::fail(CHR_ERR_INVALID, "%s: %u samples and %u taps exceed the %u words of a row in LDS", who,
                         nsamples, used, (unsigned)CHR_WAVE_LDS_WORDS);
    if (adc_max > 65535u) return chr::fail(CHR_ERR_INVALID, "%s: adc_max = %u above 65535", who, adc_max);
    *par = chr_digitise_par{nrows, nsamples, used, scale, pedestal, adc_max};
    return CHR_OK;
}

extern "C" int chr_daq_pe_trains_host(const int32_t *h_pe_channel, const float *h_pe_time, const uint32_t *h_pe_q,
                                      const int64_t *h_bounds, int32_t nevents, int32_t nchannels,
                                      const int32_t *h_row_of_word, uint32_t nrows, float t_lo, float inv,
                                      uint32_t nsamples, uint32_t *h_trains, uint32_t *h_outside_q,
                                      uint32_t *h_dropped) {
    chr_wave_par par;
    uint32_t span = 0;
    CHR_TRY(chr::trains_check("chr_daq_pe_trains_host", h_pe_channel, h_pe_time, h_pe_q, h_bounds, nevents, nchannels,
                              nrows, t_lo, inv, nsamples, h_trains, h_outside_q, h_dropped, &par, &span));
    if (!h_row_of_word && nrows != par.nevents * par.nchannels)
        return chr::fail(CHR_ERR_INVALID, "chr_daq_pe_trains_host: %u rows without a map of the %u words", nrows,
                         par.nevents * par.nchannels);
    for (size_t i = 0, n = (size_t)nrows * nsamples; i < n; ++i) h_trains[i] = 0u;
    for (uint32_t r = 0; r < nrows; ++r) h_outside_q[r] = 0u;
    *h_dropped = 0u;
    std::vector<uint32_t> bounds((size_t)nevents + 1);
    for (int32_t e = 0; e <= nevents; ++e) bounds[e] = (uint32_t)h_bounds[e];
    const chr_wave_inputs in{h_pe_channel, h_pe_time, h_pe_q, bounds.data(), h_row_of_word};
    for (uint32_t i = 0; i < span; ++i) {
        chr_wave_update u;
        switch (chr_wave_pe(&par, &in, i, &u)) {
            case CHR_WAVE_DROPPED: *h_dropped += 1u; break;
            case CHR_WAVE_INSIDE: h_trains[u.word] += u.q; break;
            case CHR_WAVE_OUTSIDE: h_outside_q[u.word] += u.q; break;
            default: break;
        }
    }
    return CHR_OK;
}

extern "C" int chr_daq_digitise_host(const uint32_t *h_trains, uint32_t nrows, uint32_t nsamples,
                                     const float *h_template, uint32_t ntaps, float scale, float pedestal,
                                     uint32_t adc_max, uint16_t *h_adc, uint32_t *h_bad) {
    chr_digitise_par par;
    CHR_TRY(chr::digitise_check("chr_daq_digitise_host", h_trains, nrows, nsamples, h_template, ntaps, scale, pedestal,
                                adc_max, h_adc, h_bad, &par));
    *h_bad = 0u;
    for (uint32_t r = 0; r < nrows; ++r) {
        const uint32_t *train = h_trains + (size_t)r * nsamples;
        uint16_t *adc = h_adc + (size_t)r * nsamples;
        uint32_t any = 0u;
        for (uint32_t s = 0; s < nsamples; ++s) any |= train[s];
        for (uint32_t s = 0; s < nsamples; ++s)          // digitiser step 1: an empty row skips the convolution
            adc[s] = chr_wave_adc(any ? chr_wave_convolve(train, h_template, par.ntaps, s) : 0.0f, &par, h_bad);
    }
    return CHR_OK;
}
