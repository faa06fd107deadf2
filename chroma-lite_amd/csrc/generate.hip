// generate.hip -- photons from gensteps on gfx950 (chr_generate_photons).
//
// replaces: the reference's host light source (chroma/generator/: Geant4
// tracks a particle and hands every photon to the GPU through a 40-byte-per-
// photon upload).  Here a step is 64 bytes however many photons it makes, and
// the photons are drawn where they are consumed.
//
// Launch shape: one work-item per RNG slot (the draw order is part of the
// contract: photon k belongs to slot k mod nslots, a slot draws its photons in
// ascending k, chroma_amd.h).  A work-item keeps its XORWOW state in registers
// across its photons -- 24 B of state traffic per slot, not per photon -- and in
// pass j the wave's lanes write photons j*nslots + slot .. + 63: every array's
// stores are consecutive words of one 256 B (768 B for the float3 arrays) span.
// 40 B written per photon and nothing read but the step record and a few table
// words (L2 / scalar cache resident).  Measured: 10 M
// photons of one isotropic step in 0.12 ms (3.2 TB/s written, 40 % of the HBM
// peak), of 10^4 mixed steps in 0.24 ms, with the simulation's 524,288 slots
// (8192 waves; 67 VGPRs, no scratch, no LDS: 7 waves per SIMD fit).
//
// The step of a photon is found by a bounded bisection of the offsets.  A
// wave's 64 consecutive photons almost always belong to one step, so the record
// is read at a wave-uniform address (scalar loads) and the kind branch does not
// diverge; a wave that straddles step boundaries serves its steps one after
// the other (a waterfall over readfirstlane, at most 64 passes), so the record
// stays wave-uniform there too.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/chroma_amd.h"
#include "common.h"
#include "device_geometry.h"
#include "genstep.h"

namespace chr_generate {

constexpr int BLOCK = 256;

struct OutPtrs {
    float *pos, *dir, *pol, *wl, *t, *weights;
    uint32_t *flags;
    int32_t *last_hit;
    uint32_t *evidx;
};

__global__ __launch_bounds__(BLOCK) void generate_kernel(const chr::DevGeom *__restrict__ gp,
                                                         const chr_genstep_dev *__restrict__ steps,
                                                         const uint32_t *__restrict__ offsets, uint32_t nsteps,
                                                         uint32_t total, OutPtrs out, uint32_t first_photon,
                                                         uint32_t *__restrict__ rng_states, uint32_t nslots,
                                                         uint32_t *__restrict__ exhausted) {
    const uint32_t slot = blockIdx.x * BLOCK + threadIdx.x;
    if (slot >= nslots || slot >= total) return;
    const chr::DevGeom &g = *gp;
    const size_t ns = nslots;
    chr_xorwow rng = {rng_states[slot], rng_states[ns + slot], rng_states[2 * ns + slot],
                      rng_states[3 * ns + slot], rng_states[4 * ns + slot], rng_states[5 * ns + slot]};
    uint32_t nexhausted = 0;
    for (uint64_t k = slot; k < total; k += nslots) {
        const uint32_t i = chr_genstep_of(offsets, nsteps, (uint32_t)k);
        chr_gen_photon p = {};
        uint32_t evidx = 0;
        bool pending = true;
        // every pass serves the lanes of the first pending lane's step; a pass retires >= 1 lane
        for (int pass = 0; pass < 64 && pending; ++pass) {
            const uint32_t iu = __builtin_amdgcn_readfirstlane(i);
            if (i != iu) continue;
            const chr_genstep_dev &st = steps[iu];
            const chr::DevMaterial &m = g.materials[st.s.material];
            chr_gen_tables tb;
            tb.refractive_index = g.tables_g + m.refractive_index;
            tb.wvl_cdf = g.tables_g + m.comp_reemission_wvl_cdf + st.s.component * (g.wl_n + 1);
            tb.time_cdf = g.tables_g + m.comp_reemission_time_cdf + st.s.component * (g.t_n + 1);
            tb.time_index = m.comp_time_index != ~0u
                                ? (const uint32_t *)g.tables_g + m.comp_time_index +
                                      st.s.component * (chr::TIME_INDEX_BUCKETS + 1)
                                : nullptr;
            tb.time_index_buckets = chr::TIME_INDEX_BUCKETS;
            tb.wl_n = g.wl_n; tb.wl_start = g.wl_start; tb.wl_step = g.wl_step;
            tb.t_n = g.t_n; tb.t_start = g.t_start; tb.t_step = g.t_step;
            nexhausted += (uint32_t)chr_genstep_photon(&st, &tb, &rng, &p);
            evidx = st.s.evidx;
            pending = false;
        }
        const size_t o = (size_t)first_photon + k;
        out.pos[3 * o] = p.pos[0]; out.pos[3 * o + 1] = p.pos[1]; out.pos[3 * o + 2] = p.pos[2];
        out.dir[3 * o] = p.dir[0]; out.dir[3 * o + 1] = p.dir[1]; out.dir[3 * o + 2] = p.dir[2];
        out.pol[3 * o] = p.pol[0]; out.pol[3 * o + 1] = p.pol[1]; out.pol[3 * o + 2] = p.pol[2];
        out.wl[o] = p.wavelength;
        out.t[o] = p.t;
        out.weights[o] = 1.0f;
        out.flags[o] = p.flags;
        out.last_hit[o] = -1;
        out.evidx[o] = evidx;
    }
    rng_states[slot] = rng.d; rng_states[ns + slot] = rng.v0; rng_states[2 * ns + slot] = rng.v1;
    rng_states[3 * ns + slot] = rng.v2; rng_states[4 * ns + slot] = rng.v3; rng_states[5 * ns + slot] = rng.v4;
    if (nexhausted) atomicAdd(exhausted, nexhausted);
}

// Staging for the records, the offsets and the counter: a device buffer and a pinned
// host buffer of the same layout (per host thread and device, grown on demand).  A copy
// from pageable memory goes through the runtime's own staging and cost more than the
// kernel (2 ms of a 2.2 ms call for 10^4 steps); from pinned memory it is one DMA.
struct Staging {
    void *dev = nullptr, *host = nullptr;
    size_t bytes = 0;
};

int staging_get(size_t bytes, Staging **out) {
    static thread_local Staging s[16];
    int dev = 0;
    CHR_HIP_CHECK(hipGetDevice(&dev));
    Staging &x = s[dev & 15];
    if (x.bytes < bytes) {
        if (x.dev) CHR_HIP_CHECK(hipFree(x.dev));
        x.dev = nullptr;
        if (x.host) CHR_HIP_CHECK(hipHostFree(x.host));
        x.host = nullptr;
        x.bytes = 0;
        const size_t grown = bytes + bytes / 2;
        CHR_HIP_CHECK(hipMalloc(&x.dev, grown));
        CHR_HIP_CHECK(hipHostMalloc(&x.host, grown, hipHostMallocDefault));
        x.bytes = grown;
    }
    *out = &x;
    return CHR_OK;
}

}  // namespace chr_generate

using namespace chr_generate;

extern "C" int chr_generate_photons(const chr_geometry *g, const chr_genstep *h_steps, uint32_t nsteps,
                                    const chr_photons *out, uint32_t first_photon, uint32_t capacity,
                                    uint32_t *d_rng_states, uint32_t rng_nslots, uint32_t *ngenerated,
                                    uint32_t *exhausted, void *vstream) {
    if (!g || !out || !d_rng_states || !ngenerated || !exhausted)
        return chr::fail(CHR_ERR_INVALID, "chr_generate_photons: null argument");
    if (!out->d_pos || !out->d_dir || !out->d_pol || !out->d_wavelengths || !out->d_t || !out->d_weights ||
        !out->d_flags || !out->d_last_hit_triangles || !out->d_evidx)
        return chr::fail(CHR_ERR_INVALID, "chr_generate_photons: null photon array");
    if (!g->h_refractive_index || !g->h_num_comp)
        return chr::fail(CHR_ERR_INVALID, "chr_generate_photons: geometry without material tables");
    const uint32_t nmat = (uint32_t)g->h_num_comp->size(), W1 = g->dev.wl_n + 1;
    std::vector<const float *> ri(nmat);
    for (uint32_t m = 0; m < nmat; ++m) ri[m] = g->h_refractive_index->data() + (size_t)m * W1;
    const chr::GenstepView view = {nmat, g->h_num_comp->data(), ri.data(), g->dev.wl_n, g->dev.wl_start,
                                   g->dev.wl_step};
    std::vector<chr_genstep_dev> dev;
    std::vector<uint32_t> offsets;
    CHR_TRY(chr::gensteps_prepare(view, h_steps, nsteps, first_photon, capacity, rng_nslots, dev, offsets));
    const uint32_t total = offsets[nsteps];
    *ngenerated = total;
    *exhausted = 0;
    if (total == 0) return CHR_OK;

    hipStream_t stream = (hipStream_t)vstream;
    // [counter | offsets | records], each part 16-byte aligned, filled in pinned memory and
    // sent in one copy (the counter goes over as 0)
    const size_t off_bytes = (((size_t)nsteps + 1) * 4 + 15) & ~(size_t)15;
    const size_t rec_bytes = (size_t)nsteps * sizeof(chr_genstep_dev);
    const size_t bytes = 16 + off_bytes + rec_bytes;
    Staging *stg = nullptr;
    CHR_TRY(staging_get(bytes, &stg));
    std::memset(stg->host, 0, 16);
    std::memcpy((char *)stg->host + 16, offsets.data(), ((size_t)nsteps + 1) * 4);
    std::memcpy((char *)stg->host + 16 + off_bytes, dev.data(), rec_bytes);
    uint32_t *d_exhausted = (uint32_t *)stg->dev;
    const uint32_t *d_offsets = (const uint32_t *)((char *)stg->dev + 16);
    const chr_genstep_dev *d_steps = (const chr_genstep_dev *)((char *)stg->dev + 16 + off_bytes);
    CHR_HIP_CHECK(hipMemcpyAsync(stg->dev, stg->host, bytes, hipMemcpyHostToDevice, stream));
    const uint32_t active = total < rng_nslots ? total : rng_nslots;
    const OutPtrs o{out->d_pos, out->d_dir, out->d_pol, out->d_wavelengths, out->d_t, out->d_weights,
                    out->d_flags, out->d_last_hit_triangles, out->d_evidx};
    hipLaunchKernelGGL(generate_kernel, dim3((active + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream,
                       (const chr::DevGeom *)g->d_dev, d_steps, d_offsets, nsteps, total, o, first_photon, d_rng_states,
                       rng_nslots, d_exhausted);
    CHR_HIP_CHECK(hipGetLastError());
    // the count comes back into the pinned buffer's first word
    CHR_HIP_CHECK(hipMemcpyAsync(stg->host, d_exhausted, 4, hipMemcpyDeviceToHost, stream));
    CHR_HIP_CHECK(hipStreamSynchronize(stream));
    *exhausted = *(const uint32_t *)stg->host;
    return CHR_OK;
}
