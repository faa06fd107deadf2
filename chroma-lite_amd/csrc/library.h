// library.h -- the photon-library lookup (include/chroma_amd.h, "photon library"):
// what one (event, channel) pair takes from one entry of the event, for the
// expected values (chr_library_expect) and for the sampled channels
// (chr_library_sample), and what a channel adds to the log-likelihood of an
// observed event under a hypothesis (chr_library_loglike), decided by one text
// for the gfx950 kernels (library.hip) and for the host twins (library_host.cpp,
// the host compiler).  CHR_FN code over chroma_fmath.h and chroma_rng.h (and
// hitmap.h's time bin) only; every multiply-add is an explicit chr_fmaf and both
// sides are built with -ffp-contract=off, so the device, the host twin and the
// numpy restatements (tests/library_model.py, tests/loglike_model.py) give the
// same words.
#ifndef CHROMA_LIBRARY_H
#define CHROMA_LIBRARY_H

#include "../../include/chroma_amd.h"
#include "../../include/chroma_fmath.h"
#include "../../include/chroma_rng.h"
#include "hitmap.h"

#define CHR_LIBRARY_NO_KEY 0xFFFFFFFFu      /* CHR_HITMAP_NO_KEY: the cleared tmin word */
#define CHR_LIBRARY_POISSON_SPLIT 32.0f     /* below: Knuth's product; from here on: the normal form */
#define CHR_LIBRARY_MAX_FACTORS 1024u       /* factors of one Knuth product (never reached by chance: p < 1e-300) */
#define CHR_LIBRARY_NO_HIT_TIME 1e9f        /* the DAQ's time of a channel without a hit */
#define CHR_LIBRARY_NO_SOURCE 0xFFFFFFFFu   /* the source of an entry outside every grid */

// the library's arrays (read-only) and the scalar part of its chr_hitmap_desc
typedef struct chr_library_map {
    uint32_t nsources, nchannels, ntbins;
    float t_lo, inv;
    const uint64_t *emitted;
    const uint32_t *counts, *tmin, *thist;     // tmin, thist: null when not kept
} chr_library_map;

// the float of a tmin key (chr_hitmap_time_key inverted); the key is not CHR_LIBRARY_NO_KEY
CHR_FN float chr_library_time_of_key(uint32_t key) {
    return chr_u2f((key & 0x80000000u) ? (key ^ 0x80000000u) : (key ^ 0xFFFFFFFFu));
}

// expected-value step 4: one IEEE divide of two round-to-nearest conversions; emitted > 0
CHR_FN float chr_library_weight(uint32_t nphotons, uint64_t emitted) {
    return (float)nphotons / (float)emitted;
}

// expected-value steps 4-5 for one entry that counts (source in range, emitted > 0):
// k and key are the channel's counts and tmin words of the entry's source (key:
// CHR_LIBRARY_NO_KEY when tmin is not kept)
CHR_FN void chr_library_expect_step(float w, float t, uint32_t k, uint32_t key, float *mu, float *tfirst) {
    *mu = chr_fmaf(w, (float)k, *mu);
    if (k > 0u && key != CHR_LIBRARY_NO_KEY) {
        const float cand = t + chr_library_time_of_key(key);
        if (cand < *tfirst) *tfirst = cand;
    }
}

// sampled-channels step 2: the Poisson draw.  flag / extra: the pair's chr_normal cache.
CHR_FN uint32_t chr_library_poisson(float m, chr_xorwow *rng, uint32_t *flag, uint32_t *extra) {
    if (!(m > 0.0f)) return 0u;                                   // NaN, 0 and negatives: nothing is drawn
    if (m < CHR_LIBRARY_POISSON_SPLIT) {
        const float limit = chr_expf(-m);
        float p = 1.0f;
        uint32_t k = 0u;
        do {
            p = p * chr_uniform01(rng);
            k += 1u;
        } while (p > limit && k < CHR_LIBRARY_MAX_FACTORS);
        return k - 1u;
    }
    const float z = chr_normal(rng, flag, extra);
    return chr_sat_u32(chr_fmaf(chr_sqrtf(m), z, m) + 0.5f);
}

// sampled-channels step 3: the earliest of `draws` times from the histogram row `h`
// (ntbins words, of sum `total` > 0) of the entry's source and the channel, or *best
CHR_FN float chr_library_draw_times(const chr_library_map *lib, const uint32_t *h, uint32_t total, uint32_t draws,
                                    float t, float width, chr_xorwow *rng, float best) {
    for (uint32_t d = 0u; d < draws; ++d) {
        const float u = chr_uniform01(rng);
        uint32_t r = chr_sat_u32(u * (float)total);
        if (r > total - 1u) r = total - 1u;
        uint32_t b = 0u, run = h[0];
        while (run <= r && b + 1u < lib->ntbins) {                 // the first bin whose running sum exceeds r
            b += 1u;
            run += h[b];
        }
        const float x = (float)b + chr_uniform01(rng);
        const float cand = t + chr_fmaf(x, width, lib->t_lo);
        if (cand < best) best = cand;
    }
    return best;
}

// The sampled pair (e, c): entries [first, last) of the CSR table in order.  Returns the
// saturating sum of the draws in *n and the pair's time in *t (CHR_LIBRARY_NO_HIT_TIME
// when n == 0).  Draws from *rng; the chr_normal cache lives and dies here.
CHR_FN void chr_library_sample_pair(const chr_library_map *lib, const uint32_t *source, const uint32_t *nphotons,
                                    const float *tt, uint32_t first, uint32_t last, uint32_t c, chr_xorwow *rng,
                                    uint32_t *n_out, float *t_out) {
    uint32_t flag = 0u, extra = 0u, n = 0u;
    float mu = 0.0f, tfirst = chr_u2f(0x7f800000u), tdrawn = chr_u2f(0x7f800000u);
    const float width = lib->ntbins ? 1.0f / lib->inv : 0.0f;
    for (uint32_t i = first; i < last; ++i) {
        const uint32_t s = source[i];
        if (s >= lib->nsources) continue;
        const uint64_t em = lib->emitted[s];
        if (em == 0u) continue;
        const float w = chr_library_weight(nphotons[i], em);
        const size_t word = (size_t)s * lib->nchannels + c;
        const uint32_t k = lib->counts[word];
        chr_library_expect_step(w, tt[i], k, lib->tmin ? lib->tmin[word] : CHR_LIBRARY_NO_KEY, &mu, &tfirst);
        const float m = w * (float)k;
        const uint32_t ni = chr_library_poisson(m, rng, &flag, &extra);
        n = (ni > 0xFFFFFFFFu - n) ? 0xFFFFFFFFu : n + ni;
        if (lib->ntbins && ni > 0u) {
            const uint32_t *h = lib->thist + word * lib->ntbins;
            uint32_t total = 0u;
            for (uint32_t b = 0u; b < lib->ntbins; ++b) total += h[b];
            if (total > 0u)
                tdrawn = chr_library_draw_times(lib, h, total, ni < CHR_LIBRARY_MAX_TIME_DRAWS ? ni
                                                : CHR_LIBRARY_MAX_TIME_DRAWS, tt[i], width, rng, tdrawn);
        }
    }
    *n_out = n;
    *t_out = n == 0u ? CHR_LIBRARY_NO_HIT_TIME : (lib->ntbins ? tdrawn : tfirst);
}

// ---------------------------------------------------------------- the log-likelihood rule
#define CHR_LOGLIKE_LIMIT 8388608.0f        /* 2^23: a channel's term is clamped to +-LIMIT */
#define CHR_LOGLIKE_SCALE 1048576.0f        /* 2^20: the fixed-point unit of a word */
#define CHR_LOGLIKE_MAX_CHANNELS 0x100000u  /* 2^20 words of at most 2^43 each fit an int64 */

// log-likelihood step 1, the time part: the histogram bin of the observed time tobs for an
// entry made at t (the hit map's own bin function), -1 when there is none
CHR_FN int32_t chr_library_loglike_bin(const chr_library_map *lib, float tobs, float t) {
    return chr_hitmap_time_bin(tobs - t, lib->t_lo, lib->inv, lib->ntbins);
}

// log-likelihood step 1, the time part: one counted entry's histogram word h of the bin found
CHR_FN void chr_library_loglike_time_step(float w, uint32_t h, float *a) { *a = chr_fmaf(w, (float)h, *a); }

// log-likelihood steps 2-4: the channel's term from mu, the time fold a (0 without tobs) and
// the observed n and tobs; `timed`: tobs was given
CHR_FN float chr_library_loglike_term(float mu, float a, uint32_t n, int timed, float tobs, uint32_t mode,
                                      float floor, float tfloor, float inv) {
    const float m = mu + floor;
    if (!(m > 0.0f)) return n == 0u ? 0.0f : -CHR_LOGLIKE_LIMIT;
    if (n == 0u) return -m;
    float term;
    if (mode == 0u) {
        term = chr_fmaf((float)n, chr_logf(m), -m);
    } else {
        const float p = 1.0f - chr_expf(-m);
        term = p > 0.0f ? chr_logf(p) : -CHR_LOGLIKE_LIMIT;
    }
    if (timed && !chr_isnan(tobs)) {
        const float d = chr_fmaf(a, inv, tfloor);
        term = (term + (d > 0.0f ? chr_logf(d) : -CHR_LOGLIKE_LIMIT)) - chr_logf(m);
    }
    return term;
}

// log-likelihood step 5: the fixed-point word of a term; a NaN gives 0 and counts in *bad
CHR_FN int64_t chr_library_loglike_word(float term, uint32_t *bad) {
    if (chr_isnan(term)) {
        *bad += 1u;
        return 0;
    }
    if (term > CHR_LOGLIKE_LIMIT) term = CHR_LOGLIKE_LIMIT;
    if (term < -CHR_LOGLIKE_LIMIT) term = -CHR_LOGLIKE_LIMIT;
    return (int64_t)(term * CHR_LOGLIKE_SCALE);                   // |product| <= 2^43, exact
}

#ifdef __cplusplus
namespace chr {
// The refusals the entry points share (library_host.cpp), made before anything is
// read through a pointer; fills *lib.  rng: chr_library_sample's states, checked when
// `sampling`.
int library_check(const char *who, const chr_hitmap_desc *desc, const chr_library_entries *entries, const void *out_a,
                  const void *out_b, const void *skipped, int sampling, const void *rng, uint32_t nslots,
                  chr_library_map *lib);
// library_check and what chr_library_loglike refuses beyond it
int library_loglike_check(const char *who, const chr_hitmap_desc *desc, const chr_library_entries *hyp,
                          const chr_library_observed *obs, const void *ll, const void *bad, const void *skipped,
                          chr_library_map *lib);
}  // namespace chr
#endif

#endif /* CHROMA_LIBRARY_H */
