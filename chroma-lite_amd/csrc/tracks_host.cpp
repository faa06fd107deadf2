// tracks_host.cpp -- downloaded track records (chr_tracks_copy) taken apart into the
// nine photon arrays on the host, in one pass over the records.
#include <cstdint>

#include "../../include/chroma_amd.h"
#include "common.h"

// replaces: the host side of photon.py:252-293's step_photons (one .get() per array and
// step gives the arrays directly; here one download gives records).  Record r goes to
// element r of every array of h_out (HOST arrays of nrecords photons; pos / dir / pol
// float3-packed) and its id to h_ids[r]; evidx is h_evidx[id].
extern "C" int chr_tracks_unpack(const uint32_t *h_records, uint64_t nrecords, const uint32_t *h_evidx,
                                 uint32_t nphotons, const chr_photons *h_out, uint32_t *h_ids) {
    if (nrecords == 0) return CHR_OK;
    if (!h_records || !h_evidx || !h_out || !h_ids || !h_out->d_pos || !h_out->d_dir || !h_out->d_pol ||
        !h_out->d_wavelengths || !h_out->d_t || !h_out->d_weights || !h_out->d_flags ||
        !h_out->d_last_hit_triangles || !h_out->d_evidx)
        return chr::fail(CHR_ERR_INVALID, "chr_tracks_unpack: null argument");
    uint32_t *pos = (uint32_t *)h_out->d_pos, *dir = (uint32_t *)h_out->d_dir, *pol = (uint32_t *)h_out->d_pol;
    uint32_t *wl = (uint32_t *)h_out->d_wavelengths, *t = (uint32_t *)h_out->d_t, *wt = (uint32_t *)h_out->d_weights;
    uint32_t *flags = h_out->d_flags, *last = (uint32_t *)h_out->d_last_hit_triangles, *evidx = h_out->d_evidx;
    uint64_t bad = 0;
    const int64_t n = (int64_t)nrecords;
#pragma omp parallel for num_threads(chr::host_threads()) schedule(static) reduction(+ : bad) if (n > 32768)
    for (int64_t r = 0; r < n; ++r) {
        const uint32_t *w = h_records + CHR_TRACK_WORDS * r;
        const uint32_t id = w[0];
        h_ids[r] = id;
        flags[r] = w[1];
        for (int a = 0; a < 3; ++a) {
            pos[3 * r + a] = w[2 + a];
            dir[3 * r + a] = w[5 + a];
            pol[3 * r + a] = w[8 + a];
        }
        wl[r] = w[11];
        t[r] = w[12];
        wt[r] = w[13];
        last[r] = w[14];
        if (id < nphotons) evidx[r] = h_evidx[id];
        else { evidx[r] = 0; bad++; }
    }
    if (bad)
        return chr::fail(CHR_ERR_INVALID, "chr_tracks_unpack: %llu records name no photon below %u",
                         (unsigned long long)bad, nphotons);
    return CHR_OK;
}
