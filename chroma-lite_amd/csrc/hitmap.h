// hitmap.h -- one photon of a hit map (include/chroma_amd.h, chr_hitmap_desc):
// what photon p adds to the map, decided by one function for
// chr_hitmap_accumulate (hitmap.hip, gfx950) and for its host twin
// chr_hitmap_accumulate_host (hitmap_host.cpp, the host compiler), one text for
// both.  CHR_FN code over chroma_fmath.h only.  The function works out the
// words (rule steps 1-7 of the header); the callers only add them, the device
// with integer atomics (LDS or global), the host with plain integer
// arithmetic, so a map is a function of its photons alone.  The time bin is
// one float subtract and one float multiply, separately rounded
// (-ffp-contract=off on both sides).
#ifndef CHROMA_HITMAP_H
#define CHROMA_HITMAP_H

#include "../../include/chroma_amd.h"
#include "../../include/chroma_fmath.h"

#define CHR_HITMAP_NO_KEY 0xFFFFFFFFu   /* the cleared tmin word: above the key of every time that is not NaN */

// what the entry points take from chr_photons and the detector
typedef struct chr_hitmap_inputs {
    const uint32_t *evidx, *flags;
    const int32_t *last_hit;
    const float *t, *weights;         // t: read when tmin or thist is kept; weights: when wsum is
    const uint32_t *solid_map;
    const int32_t *s2c;
    uint32_t detection_state;
} chr_hitmap_inputs;

// the scalar part of chr_hitmap_desc and which optional arrays are kept
typedef struct chr_hitmap_par {
    uint32_t nsources, nchannels, ntbins;
    float t_lo, inv;
    int has_tmin, has_wsum;
} chr_hitmap_par;

typedef struct chr_hitmap_update {
    uint32_t source;     // evidx[p]; >= nsources: the photon is skipped
    int32_t channel;     // -1: emitted only (step 3 stopped)
    uint32_t key;        // step 5: the time's key, CHR_HITMAP_NO_KEY when none is taken
    int32_t bin;         // step 6: the time bin, -1 when none
    uint64_t q;          // step 7: the weight word
} chr_hitmap_update;

// step 3: the selection of channel_counts_kernel / candidate_channel (daq.hip), restated
CHR_FN int32_t chr_hitmap_channel(const chr_hitmap_inputs *in, int32_t nchannels, size_t p) {
    if (!(in->flags[p] & in->detection_state)) return -1;
    const int32_t tri = in->last_hit[p];
    if (tri <= -1) return -1;
    const int32_t c = in->s2c[in->solid_map[tri]];
    return (c >= 0 && c < nchannels) ? c : -1;
}

// step 5: unsigned order of the keys = order of the floats (-inf lowest, -0 below +0, +inf highest)
CHR_FN uint32_t chr_hitmap_time_key(float t) {
    const uint32_t b = chr_f2u(t);
    return (b & 0x80000000u) ? (b ^ 0xFFFFFFFFu) : (b ^ 0x80000000u);
}

// step 6: NaN fails both comparisons, -inf the first, +inf the second
CHR_FN int32_t chr_hitmap_time_bin(float t, float t_lo, float inv, uint32_t ntbins) {
    const float d = t - t_lo;
    const float x = d * inv;
    if (!(x >= 0.0f && x < (float)ntbins)) return -1;
    return (int32_t)(uint32_t)x;
}

// step 7: weight in units of 2^-24, truncated, saturating at 2^32 - 1
CHR_FN uint64_t chr_hitmap_weight_word(float weight) {
    const float x = weight * 16777216.0f;
    if (chr_isnan(x) || x < 0.0f) return 0u;
    if (x >= 4294967296.0f) return 0xFFFFFFFFull;
    return (uint64_t)x;
}

// Rule steps 1-7 for photon p.  Returns 0 when the photon is skipped (step 1), else 1
// with *u filled: u->channel < 0 means "emitted only".
CHR_FN int chr_hitmap_photon(const chr_hitmap_par *par, const chr_hitmap_inputs *in, size_t p,
                             chr_hitmap_update *u) {
    u->source = in->evidx[p];
    u->channel = -1;
    u->key = CHR_HITMAP_NO_KEY;
    u->bin = -1;
    u->q = 0u;
    if (u->source >= par->nsources) return 0;
    u->channel = chr_hitmap_channel(in, (int32_t)par->nchannels, p);
    if (u->channel < 0) return 1;
    if (par->has_tmin || par->ntbins) {
        const float t = in->t[p];
        if (par->has_tmin && !chr_isnan(t)) u->key = chr_hitmap_time_key(t);
        if (par->ntbins) u->bin = chr_hitmap_time_bin(t, par->t_lo, par->inv, par->ntbins);
    }
    if (par->has_wsum) u->q = chr_hitmap_weight_word(in->weights[p]);
    return 1;
}

#ifdef __cplusplus
namespace chr {
// The refusals chr_hitmap_accumulate and its host twin share (hitmap_host.cpp), made before
// anything is read through a pointer of the map or the photons; fills *par and *in.
int hitmap_check(const char *who, const chr_photons *ph, int32_t start_photon, uint32_t detection_state,
                 const uint32_t *solid_map, const int32_t *s2c, const chr_hitmap_desc *desc, chr_hitmap_par *par,
                 chr_hitmap_inputs *in);
// the map's own refusals (also chr_hitmap_clear's)
int hitmap_check_desc(const char *who, const chr_hitmap_desc *desc);
}  // namespace chr
#endif

#endif /* CHROMA_HITMAP_H */
