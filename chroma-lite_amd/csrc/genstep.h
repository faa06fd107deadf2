// genstep.h -- one photon of a genstep (include/chroma_amd.h, chr_genstep): the
// per-photon function of chr_generate_photons (generate.hip, gfx950) and of its
// host twin chr_generate_photons_host (generate_host.cpp, the host compiler),
// one text for both.  CHR_FN code over chroma_fmath.h / chroma_rng.h only: every
// multiply-add is an explicit fmaf, everything else a separately rounded IEEE
// op (-ffp-contract=off on both sides), so the two compute the same bits.
//
// The few sampling / interpolation helpers it needs are restated here from
// sampling.h, photon_state.h and propagate.hip (which are device-only and stay as they are):
// same operations in the same order, so a generated photon's wavelength and
// delay are the values the propagator's bulk re-emission would draw from the
// same uniforms.
#ifndef CHROMA_GENSTEP_H
#define CHROMA_GENSTEP_H

#include "../../include/chroma_amd.h"
#include "../../include/chroma_fmath.h"
#include "../../include/chroma_rng.h"

// The device copy of a record: the public 16 words + what the host works out
// per step (gensteps_prepare): s2max = 1 - 1/(beta n_max)^2 and the wavelength
// of n_max (CHERENKOV; 0 otherwise).
typedef struct chr_genstep_dev {
    chr_genstep s;
    float s2max, wl_nmax;
    uint32_t pad[2];
} chr_genstep_dev;

// the tables of a step's material, resolved from DevGeom (device) or
// chr_geometry_desc (host)
typedef struct chr_gen_tables {
    const float *refractive_index;   // [wl_n + 1]
    const float *wvl_cdf;            // the component's comp_reemission_wvl_cdf [wl_n + 1] (SCINTILLATION)
    const float *time_cdf;           // the component's comp_reemission_time_cdf [t_n + 1]
    const uint32_t *time_index;      // its bucket index (time_cdf_index, nbuckets + 1 words) or NULL
    uint32_t time_index_buckets;
    uint32_t wl_n;
    float wl_start, wl_step;
    uint32_t t_n;
    float t_start, t_step;
} chr_gen_tables;

typedef struct chr_gen_photon {
    float pos[3], dir[3], pol[3];
    float wavelength, t;
    uint32_t flags;
} chr_gen_photon;

typedef struct { float x, y, z; } chr_gs_v3;

CHR_FN float chr_gs_dot(chr_gs_v3 a, chr_gs_v3 b) { return chr_fmaf(a.z, b.z, chr_fmaf(a.y, b.y, a.x * b.x)); }
CHR_FN chr_gs_v3 chr_gs_cross(chr_gs_v3 a, chr_gs_v3 b) {
    chr_gs_v3 r = {chr_fmaf(a.y, b.z, -(a.z * b.y)), chr_fmaf(a.z, b.x, -(a.x * b.z)),
                   chr_fmaf(a.x, b.y, -(a.y * b.x))};
    return r;
}
CHR_FN chr_gs_v3 chr_gs_unit(chr_gs_v3 a) {
    const float n = chr_sqrtf(chr_gs_dot(a, a));
    chr_gs_v3 r = {a.x / n, a.y / n, a.z / n};
    return r;
}

// photon_state.h interp_property (reference geometry.h:61-74)
CHR_FN float chr_gs_interp_property(const chr_gen_tables *tb, float x, const float *fp) {
    const float start = tb->wl_start, step = tb->wl_step;
    const int n = (int)tb->wl_n;
    if (x < start) return fp[0];
    if (x > chr_fmaf((float)(n - 1), step, start)) return fp[n - 1];
    const int jl = (int)((x - start) / step);
    const float base = chr_fmaf((float)jl, step, start);
    const float f0 = fp[jl], f1 = fp[jl + 1];
    return f0 + ((x - base) * (f1 - f0)) / step;
}

// sampling.h uniform_sphere (reference random.h:15-23)
CHR_FN chr_gs_v3 chr_gs_uniform_sphere(chr_xorwow *s) {
    const float theta = chr_uniform(s, 0.0f, 2 * CHR_PI_F);
    const float u = chr_uniform(s, -1.0f, 1.0f);
    const float c = chr_sqrtf(chr_fmaf(-u, u, 1.0f));
    float st, ct;
    chr_sincosf(theta, &st, &ct);
    chr_gs_v3 r = {c * ct, c * st, u};
    return r;
}

// sampling.h sample_cdf on a uniform grid (reference random.h:34-55); the
// bisection is the reference's, bounded by the 32 halvings an int range allows
CHR_FN float chr_gs_sample_cdf(chr_xorwow *rng, int ncdf, float x0, float delta, const float *cdf_y) {
    const float u = chr_uniform01(rng);
    int lower = 0, upper = ncdf - 1;
    for (int it = 0; it < 32 && lower < upper - 1; ++it) {
        const int half = (lower + upper) / 2;
        if (u < cdf_y[half]) upper = half; else lower = half;
    }
    const float dcy = cdf_y[upper] - cdf_y[lower];
    return chr_fmaf(delta, (float)lower, x0) + (delta * (u - cdf_y[lower])) / dcy;
}

// sampling.h sample_cdf_indexed: the same sample from a bisection of the bucket's range
CHR_FN float chr_gs_sample_cdf_indexed(chr_xorwow *rng, float x0, float delta, const float *cdf_y,
                                       const uint32_t *index, uint32_t nb) {
    const float u = chr_uniform01(rng);
    uint32_t b = (uint32_t)(u * (float)nb);
    if (b > nb - 1u) b = nb - 1u;
    int lower = (int)index[b], upper = (int)index[b + 1];
    for (int it = 0; it < 32 && lower < upper; ++it) {
        const int half = (lower + upper + 1) >> 1;
        if (cdf_y[half] <= u) lower = half; else upper = half - 1;
    }
    const float dcy = cdf_y[lower + 1] - cdf_y[lower];
    return chr_fmaf(delta, (float)lower, x0) + (delta * (u - cdf_y[lower])) / dcy;
}

// dir = uniform_sphere, pol = cross(uniform_sphere, dir) normalised: the bulk
// re-emission branch's form (propagate.hip, reference photon.h)
CHR_FN void chr_gs_isotropic_dir_pol(chr_xorwow *rng, chr_gen_photon *p) {
    const chr_gs_v3 d = chr_gs_uniform_sphere(rng);
    const chr_gs_v3 a = chr_gs_uniform_sphere(rng);
    const chr_gs_v3 c = chr_gs_cross(a, d);
    const float n = chr_sqrtf(chr_gs_dot(c, c));
    p->dir[0] = d.x; p->dir[1] = d.y; p->dir[2] = d.z;
    p->pol[0] = c.x / n; p->pol[1] = c.y / n; p->pol[2] = c.z / n;
}

// One photon of step st, drawn from rng in the order chroma_amd.h documents.
// Returns 1 when the Cherenkov rejection loop used up CHR_GEN_MAX_TRIES, else 0.
// The record was validated by gensteps_prepare (kind, material, component and
// ranges are good); an unknown kind here would draw as ISOTROPIC.
CHR_FN int chr_genstep_photon(const chr_genstep_dev *st, const chr_gen_tables *tb, chr_xorwow *rng,
                              chr_gen_photon *p) {
    const chr_genstep *s = &st->s;
    const float f = chr_uniform01(rng);
    p->pos[0] = chr_fmaf(f, s->dx[0], s->x0[0]);
    p->pos[1] = chr_fmaf(f, s->dx[1], s->x0[1]);
    p->pos[2] = chr_fmaf(f, s->dx[2], s->x0[2]);
    p->t = chr_fmaf(f, s->dt, s->t0);

    if (s->kind == CHR_GEN_SCINTILLATION) {
        p->wavelength = chr_gs_sample_cdf(rng, (int)tb->wl_n, tb->wl_start, tb->wl_step, tb->wvl_cdf);
        if (tb->time_index)
            p->t += chr_gs_sample_cdf_indexed(rng, tb->t_start, tb->t_step, tb->time_cdf, tb->time_index,
                                              tb->time_index_buckets);
        else
            p->t += chr_gs_sample_cdf(rng, (int)tb->t_n, tb->t_start, tb->t_step, tb->time_cdf);
        chr_gs_isotropic_dir_pol(rng, p);
        p->flags = CHR_SCINTILLATION;
        return 0;
    }

    if (s->kind == CHR_GEN_CHERENKOV) {
        const chr_gs_v3 dx = {s->dx[0], s->dx[1], s->dx[2]};
        const chr_gs_v3 u = chr_gs_unit(dx);
        const float inv_lo = 1.0f / s->wl_hi, inv_hi = 1.0f / s->wl_lo;
        float wl = st->wl_nmax, c = 0.0f, s2 = 0.0f;
        int accepted = 0;
        for (int i = 0; i < CHR_GEN_MAX_TRIES; ++i) {
            const float wi = 1.0f / chr_uniform(rng, inv_lo, inv_hi);
            const float n = chr_gs_interp_property(tb, wi, tb->refractive_index);
            const float ci = 1.0f / (s->beta * n);
            const float s2i = chr_fmaf(-ci, ci, 1.0f);
            if (s2i > chr_uniform01(rng) * st->s2max) {
                wl = wi; c = ci; s2 = s2i; accepted = 1;
                break;
            }
        }
        if (!accepted) {   // the wavelength of n_max: s2 == s2max > 0 there (gensteps_prepare)
            const float n = chr_gs_interp_property(tb, wl, tb->refractive_index);
            c = 1.0f / (s->beta * n);
            s2 = chr_fmaf(-c, c, 1.0f);
        }
        const float sn = chr_sqrtf(s2);
        const float phi = chr_uniform(rng, 0.0f, 2 * CHR_PI_F);
        float sp, cp;
        chr_sincosf(phi, &sp, &cp);
        // (e1, e2): e1 = cross(u, a) / |cross(u, a)| with a the coordinate axis along which u is
        // smallest (x before y before z on ties; |cross| >= sqrt(2/3)), e2 = cross(u, e1)
        const float ax = chr_fabsf(u.x), ay = chr_fabsf(u.y), az = chr_fabsf(u.z);
        chr_gs_v3 e1;
        if (ax <= ay && ax <= az) { e1.x = 0.0f; e1.y = u.z; e1.z = -u.y; }
        else if (ay <= az) { e1.x = -u.z; e1.y = 0.0f; e1.z = u.x; }
        else { e1.x = u.y; e1.y = -u.x; e1.z = 0.0f; }
        e1 = chr_gs_unit(e1);
        const chr_gs_v3 e2 = chr_gs_cross(u, e1);
        const chr_gs_v3 w = {chr_fmaf(sp, e2.x, cp * e1.x), chr_fmaf(sp, e2.y, cp * e1.y),
                             chr_fmaf(sp, e2.z, cp * e1.z)};
        p->dir[0] = chr_fmaf(sn, w.x, c * u.x);
        p->dir[1] = chr_fmaf(sn, w.y, c * u.y);
        p->dir[2] = chr_fmaf(sn, w.z, c * u.z);
        // c dir - u = s (c w - s u): the unit vector in the plane of u and dir, normal to dir
        chr_gs_v3 pol = {chr_fmaf(c, w.x, -(sn * u.x)), chr_fmaf(c, w.y, -(sn * u.y)),
                         chr_fmaf(c, w.z, -(sn * u.z))};
        pol = chr_gs_unit(pol);
        p->pol[0] = pol.x; p->pol[1] = pol.y; p->pol[2] = pol.z;
        p->wavelength = wl;
        p->flags = CHR_CHERENKOV;
        return accepted ? 0 : 1;
    }

    chr_gs_isotropic_dir_pol(rng, p);
    p->wavelength = chr_uniform(rng, s->wl_lo, s->wl_hi);
    p->flags = 0u;
    return 0;
}

// the step of photon k: the largest i in [0, nsteps) with offsets[i] <= k
// (offsets: nsteps + 1 words, the exclusive prefix sum of nphotons, k < offsets[nsteps];
// steps of no photons repeat an offset and are never chosen)
CHR_FN uint32_t chr_genstep_of(const uint32_t *offsets, uint32_t nsteps, uint32_t k) {
    uint32_t lo = 0, hi = nsteps;
    for (int it = 0; it < 32 && hi - lo > 1u; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
}

#if defined(__cplusplus)
#include <vector>
namespace chr {
// what the validation needs of a geometry, on the host
struct GenstepView {
    uint32_t nmaterials;
    const uint32_t *num_comp;               // [nmaterials]
    const float *const *refractive_index;   // [nmaterials] tables of wl_n + 1
    uint32_t wl_n;
    float wl_start, wl_step;
};
// Validate every record (the refusals chroma_amd.h lists; CHR_ERR_INVALID + message) and
// build the device copies and the offsets (nsteps + 1).  No device call.
int gensteps_prepare(const GenstepView &view, const chr_genstep *h_steps, uint32_t nsteps, uint32_t first_photon,
                     uint32_t capacity, uint32_t rng_nslots, std::vector<chr_genstep_dev> &dev,
                     std::vector<uint32_t> &offsets);
}  // namespace chr
#endif

#endif  // CHROMA_GENSTEP_H
