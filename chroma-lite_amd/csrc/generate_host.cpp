// generate_host.cpp -- the host side of the genstep generator: record
// validation (shared with the device entry, generate.hip), the host twin
// chr_generate_photons_host (genstep.h's per-photon function built by the host
// compiler, -ffp-contract=off: the device's bits without a GPU) and the host
// form of the RNG slot initialisation.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <vector>

#include "common.h"
#include "device_geometry.h"
#include "genstep.h"

namespace {

bool finite_record(const chr_genstep &s) {
    const float v[11] = {s.x0[0], s.x0[1], s.x0[2], s.t0, s.dx[0], s.dx[1], s.dx[2], s.dt, s.wl_lo, s.wl_hi, s.beta};
    for (float x : v)
        if (!chr_isfinite(x)) return false;
    return true;
}

// the jump matrices of curand_init (chroma_rng.h), computed once
struct JumpMatrices {
    std::vector<uint32_t> seq, off;
    JumpMatrices() : seq((size_t)CHR_XW_MATWORDS * 32), off((size_t)CHR_XW_MATWORDS * 64) {
        chr_xw_sequence_matrices(seq.data(), 32);
        chr_xw_offset_matrices(off.data(), 64);
    }
};

}  // namespace

int chr::gensteps_prepare(const GenstepView &view, const chr_genstep *h_steps, uint32_t nsteps, uint32_t first_photon,
                          uint32_t capacity, uint32_t rng_nslots, std::vector<chr_genstep_dev> &dev,
                          std::vector<uint32_t> &offsets) {
    if (nsteps && !h_steps) return chr::fail(CHR_ERR_INVALID, "gensteps: null records");
    if (rng_nslots == 0) return chr::fail(CHR_ERR_INVALID, "gensteps: no rng states");
    if (first_photon > capacity)
        return chr::fail(CHR_ERR_INVALID, "gensteps: first photon %u beyond the capacity %u", first_photon, capacity);
    dev.resize(nsteps);
    offsets.assign((size_t)nsteps + 1, 0u);
    uint64_t total = 0;
    chr_gen_tables tb = {};
    tb.wl_n = view.wl_n; tb.wl_start = view.wl_start; tb.wl_step = view.wl_step;
    bool have_nmax = false;
    uint32_t nmax_material = 0;
    float nmax_lo = 0.0f, nmax_hi = 0.0f, n_max = 0.0f, wl_nmax = 0.0f;
    for (uint32_t i = 0; i < nsteps; ++i) {
        const chr_genstep &s = h_steps[i];
        chr_genstep_dev &d = dev[i];
        d.s = s;
        d.s2max = 0.0f; d.wl_nmax = 0.0f; d.pad[0] = d.pad[1] = 0u;
        if (s.kind > CHR_GEN_CHERENKOV) return chr::fail(CHR_ERR_INVALID, "genstep %u: unknown kind %u", i, s.kind);
        if (s.material >= view.nmaterials)
            return chr::fail(CHR_ERR_INVALID, "genstep %u: material %u of %u", i, s.material, view.nmaterials);
        if (!finite_record(s)) return chr::fail(CHR_ERR_INVALID, "genstep %u: non-finite field", i);
        if (s.kind == CHR_GEN_SCINTILLATION) {
            if (s.component >= view.num_comp[s.material])
                return chr::fail(CHR_ERR_INVALID, "genstep %u: component %u of material %u, which has %u", i,
                                 s.component, s.material, view.num_comp[s.material]);
        } else {   // the kinds that read the wavelength range (and no component)
            d.s.component = 0u;
            if (!(s.wl_lo > 0.0f) || !(s.wl_hi > 0.0f))
                return chr::fail(CHR_ERR_INVALID, "genstep %u: wavelength limits must be positive", i);
            if (s.wl_lo > s.wl_hi)
                return chr::fail(CHR_ERR_INVALID, "genstep %u: wl_lo %g > wl_hi %g", i, (double)s.wl_lo, (double)s.wl_hi);
        }
        if (s.kind == CHR_GEN_CHERENKOV) {
            const float len = chr_sqrtf(chr_fmaf(s.dx[2], s.dx[2], chr_fmaf(s.dx[1], s.dx[1], s.dx[0] * s.dx[0])));
            if (!(len > 0.0f) || !chr_isfinite(len))
                return chr::fail(CHR_ERR_INVALID, "genstep %u: a Cherenkov step needs a direction (|dx| = %g)", i,
                                 (double)len);
            if (!(s.beta > 0.0f) || s.beta > 1.0f)
                return chr::fail(CHR_ERR_INVALID, "genstep %u: beta %g outside (0, 1]", i, (double)s.beta);
            // n_max over [wl_lo, wl_hi]: n is piecewise linear, so it is reached at a limit or at a
            // grid point between them; evaluated with the kernel's own interpolation.  Steps
            // usually share their material and range: the last answer is kept.
            if (!(have_nmax && s.material == nmax_material && s.wl_lo == nmax_lo && s.wl_hi == nmax_hi)) {
                const float *ri = view.refractive_index[s.material];
                wl_nmax = s.wl_lo;
                n_max = chr_gs_interp_property(&tb, s.wl_lo, ri);
                const float n_hi = chr_gs_interp_property(&tb, s.wl_hi, ri);
                if (n_hi > n_max) { n_max = n_hi; wl_nmax = s.wl_hi; }
                for (uint32_t j = 0; j < view.wl_n; ++j) {
                    const float w = chr_fmaf((float)j, view.wl_step, view.wl_start);
                    if (!(w > s.wl_lo && w < s.wl_hi)) continue;
                    const float n = chr_gs_interp_property(&tb, w, ri);
                    if (n > n_max) { n_max = n; wl_nmax = w; }
                }
                have_nmax = true; nmax_material = s.material; nmax_lo = s.wl_lo; nmax_hi = s.wl_hi;
            }
            const float c = 1.0f / (s.beta * n_max);
            const float s2max = chr_fmaf(-c, c, 1.0f);
            if (!(s.beta * n_max > 1.0f) || !(s2max > 0.0f))
                return chr::fail(CHR_ERR_INVALID, "genstep %u: below the Cherenkov threshold (beta %g, n_max %g)", i,
                                 (double)s.beta, (double)n_max);
            d.s2max = s2max;
            d.wl_nmax = wl_nmax;
        }
        offsets[i] = (uint32_t)total;
        total += s.nphotons;
        if (total > 0x7fffffffull) return chr::fail(CHR_ERR_INVALID, "gensteps: more than 2^31 - 1 photons");
    }
    offsets[nsteps] = (uint32_t)total;
    if (total > (uint64_t)(capacity - first_photon))
        return chr::fail(CHR_ERR_INVALID, "gensteps: %llu photons from photon %u, capacity %u", (unsigned long long)total,
                         first_photon, capacity);
    return CHR_OK;
}

extern "C" int chr_gensteps_count(const chr_genstep *h_steps, uint32_t nsteps, uint64_t *total) {
    if (!total || (nsteps && !h_steps)) return chr::fail(CHR_ERR_INVALID, "chr_gensteps_count: null argument");
    uint64_t n = 0;
    for (uint32_t i = 0; i < nsteps; ++i) n += h_steps[i].nphotons;
    *total = n;
    return CHR_OK;
}

extern "C" int chr_init_rng_host(uint32_t *h_states, uint32_t nslots, uint64_t seed, uint64_t first_subsequence,
                                 uint64_t offset) {
    if (!h_states || nslots == 0) return chr::fail(CHR_ERR_INVALID, "chr_init_rng_host: empty state buffer");
    if (first_subsequence + nslots > (1ull << 32))
        return chr::fail(CHR_ERR_INVALID, "chr_init_rng_host: subsequences beyond 2^32 are not supported");
    static const JumpMatrices jm;
#pragma omp parallel for num_threads(chr::host_threads()) schedule(static)
    for (int64_t s = 0; s < (int64_t)nslots; ++s) {
        chr_xorwow r;
        chr_xorwow_init(&r, seed, first_subsequence + (uint64_t)s, offset, jm.seq.data(), 32, jm.off.data(), 64);
        h_states[s] = r.d; h_states[(size_t)nslots + s] = r.v0; h_states[2 * (size_t)nslots + s] = r.v1;
        h_states[3 * (size_t)nslots + s] = r.v2; h_states[4 * (size_t)nslots + s] = r.v3;
        h_states[5 * (size_t)nslots + s] = r.v4;
    }
    return CHR_OK;
}

extern "C" int chr_generate_photons_host(const chr_geometry_desc *desc, const chr_genstep *h_steps, uint32_t nsteps,
                                         const chr_photons *out, uint32_t first_photon, uint32_t capacity,
                                         uint32_t *h_rng_states, uint32_t rng_nslots, uint32_t *ngenerated,
                                         uint32_t *exhausted) {
    if (!desc || !desc->materials || !out || !h_rng_states || !ngenerated || !exhausted)
        return chr::fail(CHR_ERR_INVALID, "chr_generate_photons_host: null argument");
    if (!out->d_pos || !out->d_dir || !out->d_pol || !out->d_wavelengths || !out->d_t || !out->d_weights ||
        !out->d_flags || !out->d_last_hit_triangles || !out->d_evidx)
        return chr::fail(CHR_ERR_INVALID, "chr_generate_photons_host: null photon array");
    if (desc->wavelength_n < 2 || desc->time_n < 2)
        return chr::fail(CHR_ERR_INVALID, "chr_generate_photons_host: grids need >= 2 points");
    std::vector<uint32_t> num_comp(desc->nmaterials);
    std::vector<const float *> ri(desc->nmaterials);
    for (uint32_t m = 0; m < desc->nmaterials; ++m) {
        num_comp[m] = desc->materials[m].num_comp;
        ri[m] = desc->materials[m].refractive_index;
        if (!ri[m]) return chr::fail(CHR_ERR_INVALID, "material %u: missing table", m);
        if (num_comp[m] && (!desc->materials[m].comp_reemission_wvl_cdf || !desc->materials[m].comp_reemission_time_cdf))
            return chr::fail(CHR_ERR_INVALID, "material %u: missing component table", m);
    }
    const chr::GenstepView view = {desc->nmaterials, num_comp.data(), ri.data(), desc->wavelength_n,
                                   desc->wavelength_start, desc->wavelength_step};
    std::vector<chr_genstep_dev> dev;
    std::vector<uint32_t> offsets;
    CHR_TRY(chr::gensteps_prepare(view, h_steps, nsteps, first_photon, capacity, rng_nslots, dev, offsets));
    const uint32_t total = offsets[nsteps];
    *ngenerated = total;
    *exhausted = 0;
    if (total == 0) return CHR_OK;

    // the tables of every step, with the time CDFs' bucket index where the device geometry
    // holds one (chr_geometry_create builds it under the same rule, time_cdf_index)
    const uint32_t W1 = desc->wavelength_n + 1, T1 = desc->time_n + 1;
    std::map<uint32_t, std::vector<uint32_t>> index;   // material -> its components' indexes (empty: none)
    std::vector<chr_gen_tables> tables(nsteps);
    for (uint32_t i = 0; i < nsteps; ++i) {
        const chr_genstep &s = dev[i].s;
        const chr_material_desc &m = desc->materials[s.material];
        chr_gen_tables &tb = tables[i];
        tb = chr_gen_tables{};
        tb.refractive_index = m.refractive_index;
        tb.wl_n = desc->wavelength_n; tb.wl_start = desc->wavelength_start; tb.wl_step = desc->wavelength_step;
        tb.t_n = desc->time_n; tb.t_start = desc->time_start; tb.t_step = desc->time_step;
        tb.time_index_buckets = chr::TIME_INDEX_BUCKETS;
        if (s.kind != CHR_GEN_SCINTILLATION) continue;
        tb.wvl_cdf = m.comp_reemission_wvl_cdf + (size_t)s.component * W1;
        tb.time_cdf = m.comp_reemission_time_cdf + (size_t)s.component * T1;
        auto it = index.find(s.material);
        if (it == index.end()) {
            std::vector<uint32_t> idx;
            if (!chr::time_cdf_index(m.comp_reemission_time_cdf, m.num_comp, desc->time_n, T1, idx)) idx.clear();
            it = index.emplace(s.material, std::move(idx)).first;
        }
        if (!it->second.empty()) tb.time_index = it->second.data() + (size_t)s.component * (chr::TIME_INDEX_BUCKETS + 1);
    }

    const uint32_t active = total < rng_nslots ? total : rng_nslots;
    const size_t ns = rng_nslots;
    uint64_t nexhausted = 0;
#pragma omp parallel for num_threads(chr::host_threads()) schedule(static) reduction(+ : nexhausted)
    for (int64_t slot = 0; slot < (int64_t)active; ++slot) {
        chr_xorwow rng = {h_rng_states[slot], h_rng_states[ns + slot], h_rng_states[2 * ns + slot],
                          h_rng_states[3 * ns + slot], h_rng_states[4 * ns + slot], h_rng_states[5 * ns + slot]};
        for (uint64_t k = (uint64_t)slot; k < total; k += rng_nslots) {
            const uint32_t i = chr_genstep_of(offsets.data(), nsteps, (uint32_t)k);
            chr_gen_photon p;
            nexhausted += (uint64_t)chr_genstep_photon(&dev[i], &tables[i], &rng, &p);
            const size_t o = (size_t)first_photon + k;
            for (int c = 0; c < 3; ++c) {
                out->d_pos[3 * o + c] = p.pos[c];
                out->d_dir[3 * o + c] = p.dir[c];
                out->d_pol[3 * o + c] = p.pol[c];
            }
            out->d_wavelengths[o] = p.wavelength;
            out->d_t[o] = p.t;
            out->d_weights[o] = 1.0f;
            out->d_flags[o] = p.flags;
            out->d_last_hit_triangles[o] = -1;
            out->d_evidx[o] = dev[i].s.evidx;
        }
        h_rng_states[slot] = rng.d; h_rng_states[ns + slot] = rng.v0; h_rng_states[2 * ns + slot] = rng.v1;
        h_rng_states[3 * ns + slot] = rng.v2; h_rng_states[4 * ns + slot] = rng.v3;
        h_rng_states[5 * ns + slot] = rng.v4;
    }
    *exhausted = (uint32_t)nexhausted;
    return CHR_OK;
}
