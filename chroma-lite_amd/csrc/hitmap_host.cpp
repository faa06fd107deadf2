// hitmap_host.cpp -- the host side of the hit map: the refusals shared with the
// device entry (hitmap.hip) and the host twin chr_hitmap_accumulate_host
// (hitmap.h's per-photon rule built by the host compiler: the device's words
// without a GPU).
#include <cstdint>

#include "common.h"
#include "hitmap.h"

int chr::hitmap_check_desc(const char *who, const chr_hitmap_desc *desc) {
    if (!desc || !desc->d_emitted || !desc->d_counts || !desc->d_skipped)
        return chr::fail(CHR_ERR_INVALID, "%s: null argument", who);
    if (desc->nsources == 0 || desc->nchannels <= 0)
        return chr::fail(CHR_ERR_INVALID, "%s: %u sources of %d channels", who, desc->nsources, desc->nchannels);
    if (desc->ntbins > 0 && !desc->d_thist)
        return chr::fail(CHR_ERR_INVALID, "%s: %u time bins but no histogram array", who, desc->ntbins);
    if (desc->ntbins == 0 && desc->d_thist)
        return chr::fail(CHR_ERR_INVALID, "%s: a histogram array but no time bins", who);
    const uint64_t limit = 0x80000000ull;
    const uint64_t words = (uint64_t)desc->nsources * (uint32_t)desc->nchannels;
    // words <= 2^31 before the product with ntbins < 2^32, so that cannot wrap either
    if (desc->nsources > limit || words > limit || (desc->ntbins && words * desc->ntbins > limit))
        return chr::fail(CHR_ERR_INVALID, "%s: %u sources x %d channels x %u bins exceed 2^31 words", who,
                         desc->nsources, desc->nchannels, desc->ntbins);
    if (desc->ntbins > 0 && !(chr_isfinite(desc->inv) && desc->inv > 0.0f))
        return chr::fail(CHR_ERR_INVALID, "%s: inv = %g must be finite and positive", who, (double)desc->inv);
    return CHR_OK;
}

int chr::hitmap_check(const char *who, const chr_photons *ph, int32_t start_photon, uint32_t detection_state,
                      const uint32_t *solid_map, const int32_t *s2c, const chr_hitmap_desc *desc,
                      chr_hitmap_par *par, chr_hitmap_inputs *in) {
    if (!ph || !ph->d_evidx || !ph->d_flags || !ph->d_last_hit_triangles || !solid_map || !s2c)
        return chr::fail(CHR_ERR_INVALID, "%s: null argument", who);
    CHR_TRY(chr::hitmap_check_desc(who, desc));
    if ((desc->d_tmin || desc->ntbins) && !ph->d_t)
        return chr::fail(CHR_ERR_INVALID, "%s: null photon times", who);
    if (desc->d_wsum && !ph->d_weights) return chr::fail(CHR_ERR_INVALID, "%s: null photon weights", who);
    if (start_photon < 0) return chr::fail(CHR_ERR_INVALID, "%s: negative start %d", who, start_photon);
    *par = chr_hitmap_par{desc->nsources, (uint32_t)desc->nchannels, desc->ntbins, desc->t_lo, desc->inv,
                          desc->d_tmin != nullptr, desc->d_wsum != nullptr};
    *in = chr_hitmap_inputs{ph->d_evidx, ph->d_flags, ph->d_last_hit_triangles, ph->d_t, ph->d_weights,
                            solid_map, s2c, detection_state};
    return CHR_OK;
}

extern "C" int chr_hitmap_accumulate_host(const chr_photons *ph, int32_t start_photon, int32_t nphotons,
                                          uint32_t detection_state, const uint32_t *h_solid_map,
                                          const int32_t *h_solid_id_to_channel_index, const chr_hitmap_desc *desc) {
    chr_hitmap_par par;
    chr_hitmap_inputs in;
    CHR_TRY(chr::hitmap_check("chr_hitmap_accumulate_host", ph, start_photon, detection_state, h_solid_map,
                              h_solid_id_to_channel_index, desc, &par, &in));
    if (nphotons <= 0) return CHR_OK;
    for (size_t p = (size_t)start_photon, end = (size_t)start_photon + (size_t)nphotons; p < end; ++p) {
        chr_hitmap_update u;
        if (!chr_hitmap_photon(&par, &in, p, &u)) {
            *desc->d_skipped += 1;
            continue;
        }
        desc->d_emitted[u.source] += 1;
        if (u.channel < 0) continue;
        const size_t w = (size_t)u.source * par.nchannels + (uint32_t)u.channel;
        desc->d_counts[w] += 1u;
        if (u.key != CHR_HITMAP_NO_KEY && u.key < desc->d_tmin[w]) desc->d_tmin[w] = u.key;
        if (u.bin >= 0) desc->d_thist[w * par.ntbins + (uint32_t)u.bin] += 1u;
        if (par.has_wsum) desc->d_wsum[w] += u.q;
    }
    return CHR_OK;
}
