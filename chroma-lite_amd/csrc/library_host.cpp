// library_host.cpp -- the host side of the photon-library lookup: the refusals
// shared with the device entries (library.hip) and the host twins
// chr_library_expect_host / chr_library_sample_host / chr_library_loglike_host
// (library.h's rules built by the host compiler: the device's words without a GPU).
#include <cstdint>

#include "common.h"
#include "library.h"

int chr::library_check(const char *who, const chr_hitmap_desc *desc, const chr_library_entries *entries,
                       const void *out_a, const void *out_b, const void *skipped, int sampling, const void *rng,
                       uint32_t nslots, chr_library_map *lib) {
    if (!desc || !entries || !desc->d_emitted || !desc->d_counts || !out_a || !skipped)
        return chr::fail(CHR_ERR_INVALID, "%s: null argument", who);
    // the second output: sample's times always, expect's tfirst when the library keeps tmin
    if (!out_b && (sampling || desc->d_tmin)) return chr::fail(CHR_ERR_INVALID, "%s: null argument", who);
    if (sampling && !rng) return chr::fail(CHR_ERR_INVALID, "%s: null argument", who);
    if (desc->nsources == 0 || desc->nchannels <= 0)
        return chr::fail(CHR_ERR_INVALID, "%s: %u sources of %d channels", who, desc->nsources, desc->nchannels);
    if (desc->ntbins > 0 && !desc->d_thist)
        return chr::fail(CHR_ERR_INVALID, "%s: %u time bins but no histogram array", who, desc->ntbins);
    if (desc->ntbins == 0 && desc->d_thist)
        return chr::fail(CHR_ERR_INVALID, "%s: a histogram array but no time bins", who);
    const uint64_t limit = 0x80000000ull;
    const uint64_t words = (uint64_t)desc->nsources * (uint32_t)desc->nchannels;
    if (desc->nsources > limit || words > limit || (desc->ntbins && words * desc->ntbins > limit))
        return chr::fail(CHR_ERR_INVALID, "%s: %u sources x %d channels x %u bins exceed 2^31 words", who,
                         desc->nsources, desc->nchannels, desc->ntbins);
    if (desc->ntbins > 0 && !(chr_isfinite(desc->inv) && desc->inv > 0.0f))
        return chr::fail(CHR_ERR_INVALID, "%s: inv = %g must be finite and positive", who, (double)desc->inv);
    if ((uint64_t)entries->nevents * (uint32_t)desc->nchannels > limit)
        return chr::fail(CHR_ERR_INVALID, "%s: %u events x %d channels exceed 2^31 words", who, entries->nevents,
                         desc->nchannels);
    if (sampling && (nslots == 0 || 6ull * nslots > limit))
        return chr::fail(CHR_ERR_INVALID, "%s: %u rng slots", who, nslots);
    if (entries->nevents > 0 && (!entries->offsets || !entries->source || !entries->nphotons || !entries->t))
        return chr::fail(CHR_ERR_INVALID, "%s: null argument", who);
    *lib = chr_library_map{desc->nsources, (uint32_t)desc->nchannels, desc->ntbins, desc->t_lo, desc->inv,
                           desc->d_emitted, desc->d_counts, desc->d_tmin, desc->d_thist};
    return CHR_OK;
}

int chr::library_loglike_check(const char *who, const chr_hitmap_desc *desc, const chr_library_entries *hyp,
                               const chr_library_observed *obs, const void *ll, const void *bad, const void *skipped,
                               chr_library_map *lib) {
    // bad stands where expect's tfirst does, and is required whether or not the library keeps tmin
    if (!obs || !obs->nobs || !bad) return chr::fail(CHR_ERR_INVALID, "%s: null argument", who);
    CHR_TRY(chr::library_check(who, desc, hyp, ll, bad, skipped, 0, nullptr, 0, lib));
    if (obs->mode > 1u) return chr::fail(CHR_ERR_INVALID, "%s: mode %u is neither 0 (Poisson) nor 1 (hit)", who, obs->mode);
    if (!(obs->floor >= 0.0f) || !(obs->tfloor >= 0.0f))
        return chr::fail(CHR_ERR_INVALID, "%s: floor = %g and tfloor = %g must not be negative or NaN", who,
                         (double)obs->floor, (double)obs->tfloor);
    if (obs->tobs && !desc->d_thist)
        return chr::fail(CHR_ERR_INVALID, "%s: observed times but the library keeps no histogram", who);
    if ((uint32_t)desc->nchannels > CHR_LOGLIKE_MAX_CHANNELS)
        return chr::fail(CHR_ERR_INVALID, "%s: %d channels exceed 2^20", who, desc->nchannels);
    return CHR_OK;
}

// offsets[0 .. nevents] never decrease (host memory; the Python layer checks the device calls')
static int check_offsets(const char *who, const chr_library_entries *en) {
    for (uint32_t e = 0; e < en->nevents; ++e)
        if (en->offsets[e + 1] < en->offsets[e])
            return chr::fail(CHR_ERR_INVALID, "%s: offsets not ascending at event %u", who, e);
    return CHR_OK;
}

static uint64_t skipped_entries(const chr_library_map &lib, const chr_library_entries *en) {
    uint64_t n = 0;
    for (uint32_t i = en->offsets[0]; i < en->offsets[en->nevents]; ++i) n += en->source[i] >= lib.nsources;
    return n;
}

extern "C" int chr_library_expect_host(const chr_hitmap_desc *desc, const chr_library_entries *entries, float *h_mu,
                                       float *h_tfirst, uint64_t *h_skipped) {
    chr_library_map lib;
    CHR_TRY(chr::library_check("chr_library_expect_host", desc, entries, h_mu, h_tfirst, h_skipped, 0, nullptr, 0,
                               &lib));
    if (entries->nevents == 0) return CHR_OK;
    CHR_TRY(check_offsets("chr_library_expect_host", entries));
    for (uint32_t e = 0; e < entries->nevents; ++e)
        for (uint32_t c = 0; c < lib.nchannels; ++c) {
            float mu = 0.0f, tfirst = chr_u2f(0x7f800000u);
            for (uint32_t i = entries->offsets[e]; i < entries->offsets[e + 1]; ++i) {
                const uint32_t s = entries->source[i];
                if (s >= lib.nsources || lib.emitted[s] == 0u) continue;
                const size_t word = (size_t)s * lib.nchannels + c;
                chr_library_expect_step(chr_library_weight(entries->nphotons[i], lib.emitted[s]), entries->t[i],
                                        lib.counts[word], lib.tmin ? lib.tmin[word] : CHR_LIBRARY_NO_KEY, &mu, &tfirst);
            }
            h_mu[(size_t)e * lib.nchannels + c] = mu;
            if (lib.tmin) h_tfirst[(size_t)e * lib.nchannels + c] = tfirst;
        }
    *h_skipped += skipped_entries(lib, entries);
    return CHR_OK;
}

extern "C" int chr_library_sample_host(const chr_hitmap_desc *desc, const chr_library_entries *entries,
                                       uint32_t *h_rng_states, uint32_t nslots, uint32_t *h_n, float *h_t,
                                       uint64_t *h_skipped) {
    chr_library_map lib;
    CHR_TRY(chr::library_check("chr_library_sample_host", desc, entries, h_n, h_t, h_skipped, 1, h_rng_states, nslots,
                               &lib));
    if (entries->nevents == 0) return CHR_OK;
    CHR_TRY(check_offsets("chr_library_sample_host", entries));
    const uint64_t npairs = (uint64_t)entries->nevents * lib.nchannels;
    const uint32_t T = (uint32_t)(nslots < npairs ? nslots : npairs);
    uint32_t *st = h_rng_states;
    for (uint32_t j = 0; j < T; ++j) {
        chr_xorwow rng = {st[j], st[nslots + j], st[2 * (size_t)nslots + j], st[3 * (size_t)nslots + j],
                          st[4 * (size_t)nslots + j], st[5 * (size_t)nslots + j]};
        for (uint64_t k = j; k < npairs; k += T) {
            const uint32_t e = (uint32_t)(k / lib.nchannels), c = (uint32_t)(k % lib.nchannels);
            chr_library_sample_pair(&lib, entries->source, entries->nphotons, entries->t, entries->offsets[e],
                                    entries->offsets[e + 1], c, &rng, h_n + k, h_t + k);
        }
        st[j] = rng.d; st[nslots + j] = rng.v0; st[2 * (size_t)nslots + j] = rng.v1;
        st[3 * (size_t)nslots + j] = rng.v2; st[4 * (size_t)nslots + j] = rng.v3; st[5 * (size_t)nslots + j] = rng.v4;
    }
    *h_skipped += skipped_entries(lib, entries);
    return CHR_OK;
}

extern "C" int chr_library_loglike_host(const chr_hitmap_desc *desc, const chr_library_entries *hyp,
                                        const chr_library_observed *obs, int64_t *h_ll, uint32_t *h_bad,
                                        uint64_t *h_skipped) {
    chr_library_map lib;
    CHR_TRY(chr::library_loglike_check("chr_library_loglike_host", desc, hyp, obs, h_ll, h_bad, h_skipped, &lib));
    if (hyp->nevents == 0) return CHR_OK;
    CHR_TRY(check_offsets("chr_library_loglike_host", hyp));
    const int timed = obs->tobs != nullptr;
    for (uint32_t h = 0; h < hyp->nevents; ++h) {
        int64_t ll = 0;
        uint32_t bad = 0;
        for (uint32_t c = 0; c < lib.nchannels; ++c) {
            const uint32_t n = obs->nobs[c];
            const float tobs = timed ? obs->tobs[c] : 0.0f;
            float mu = 0.0f, a = 0.0f, unused = 0.0f;
            for (uint32_t i = hyp->offsets[h]; i < hyp->offsets[h + 1]; ++i) {
                const uint32_t s = hyp->source[i];
                if (s >= lib.nsources || lib.emitted[s] == 0u) continue;
                const float w = chr_library_weight(hyp->nphotons[i], lib.emitted[s]);
                const size_t word = (size_t)s * lib.nchannels + c;
                chr_library_expect_step(w, hyp->t[i], lib.counts[word], CHR_LIBRARY_NO_KEY, &mu, &unused);
                if (timed && n > 0u) {
                    const int32_t b = chr_library_loglike_bin(&lib, tobs, hyp->t[i]);
                    if (b >= 0) chr_library_loglike_time_step(w, lib.thist[word * lib.ntbins + (uint32_t)b], &a);
                }
            }
            ll += chr_library_loglike_word(
                chr_library_loglike_term(mu, a, n, timed, tobs, obs->mode, obs->floor, obs->tfloor, lib.inv), &bad);
        }
        h_ll[h] = ll;
        h_bad[h] = bad;
    }
    *h_skipped += skipped_entries(lib, hyp);
    return CHR_OK;
}
