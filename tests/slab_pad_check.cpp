// slab_pad_check.cpp -- stand-alone host check of the padded one-FMA slab planes
// (chroma-lite_amd/csrc/slab_plane.h), built and run by tests/test_slab_pad.py.
//
// For every drawn plane (byte q of a wide node with origin org and quantum s = 2^e)
// and ray axis (origin o, direction component d) it computes, with the header's own
// functions and the host's fused fmaf,
//     T   = slab_t2(q, s, org, mult, off)                  two FMAs, unpadded
//     T'n = slab_t1(q, S, O'_near),  T'f = slab_t1(q, S, O'_far)     one FMA, padded
// and counts a violation unless T'n <= T <= T'f, with a NaN read as the walk's
// fmaxf/fminf chains read it (ignored: -inf for a near plane, +inf for a far one).
// On an axis that is not wild every value must be finite.  It also reports the
// largest |T - T'0| / eps of the unpadded one-FMA distance T'0 (the proof's bound
// is 0.5).  usage: slab_pad_check NDRAWS SEED; prints one line of key=value pairs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "slab_plane.h"

namespace {

struct Rng {
    uint64_t s;
    uint64_t next() {   // splitmix64
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

float pow2f(int e) {   // 2^e, e in [-126, 127]
    const uint32_t u = (uint32_t)(e + 127) << 23;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
float nudge(float x, int ulps) {
    for (; ulps > 0; --ulps) x = std::nextafterf(x, INFINITY);
    for (; ulps < 0; ++ulps) x = std::nextafterf(x, -INFINITY);
    return x;
}

// the exponent quantize_axis (wide_bvh.cpp) starts from, plus `bump` retries
int node_exponent(float lo, float hi, int bump) {
    const double ext = (double)hi - (double)lo;
    int e = ext > 0 ? (int)std::ceil(std::log2(ext / 255.0)) : -126;
    e = e < -126 ? -126 : (e > 127 ? 127 : e);
    e += bump;
    return e > 127 ? 127 : e;
}

// the node's quantum: quantize_axis' first exponent, raised by up to `bump` retries
// while the planes stay inside the bound wide_validate enforces
float node_quantum(float lo, float hi, int bump, float W) {
    for (; bump > 0; --bump)
        if (chr::slab_planes_within(lo, pow2f(node_exponent(lo, hi, bump)), W)) break;
    return pow2f(node_exponent(lo, hi, bump));
}

struct Tally {
    uint64_t planes = 0, wild = 0, violations = 0, nonfinite = 0, outside_bound = 0;
    double max_ratio = 0.0, max_pad_mm = 0.0;
    float worst[6] = {0, 0, 0, 0, 0, 0};   // q, s, org, o, d, W of the first violation
};

const float DIRS[] = {0.0f, 1e-45f, 1e-40f, 1.17549435e-38f, 1e-33f, 1e-30f, 1e-20f, 1e-10f, 1e-3f};
constexpr int NDIRS = sizeof(DIRS) / sizeof(DIRS[0]);

void check_plane(Tally &t, float q, float s, float org, float o, float d, float W) {
    using namespace chr;
    t.planes++;
    if (!slab_planes_within(org, s, W)) { t.outside_bound++; return; }   // wide_validate refuses such a node
    const float inv = 1.0f / d, noid = -o / d;
    const float mult = slab_mult(inv), off = slab_off(o, noid, inv);
    const float eps = slab_pad(mult, off, W);
    const float S = slab_scale(s, mult);
    const float On = slab_origin(org, mult, slab_near_off(off, eps));
    const float Of = slab_origin(org, mult, slab_far_off(off, eps));
    const float T = slab_t2(q, s, org, mult, off);
    const float Tn = slab_t1(q, S, On), Tf = slab_t1(q, S, Of);
    const bool wild = !(eps < INFINITY);
    bool bad = false;
    if (wild) {
        t.wild++;
        // never culls: -inf or NaN near, +inf or NaN far
        bad = !(std::isnan(Tn) || Tn == -INFINITY) || !(std::isnan(Tf) || Tf == INFINITY);
    } else {
        if (!std::isfinite(T) || !std::isfinite(Tn) || !std::isfinite(Tf) || !std::isfinite(S)) { t.nonfinite++; bad = true; }
        const float T0 = slab_t1(q, S, slab_origin(org, mult, off));
        const double ratio = std::fabs((double)T - (double)T0) / (double)eps;
        if (ratio > t.max_ratio) t.max_ratio = ratio;
        const double pad_mm = (double)eps / std::fabs((double)mult);
        if (pad_mm > t.max_pad_mm && W <= 2.0e5f && std::fabs(o) <= W) t.max_pad_mm = pad_mm;
    }
    // as the chains read them: fmaxf skips a NaN near distance, fminf a NaN far one
    const float Tnear = std::isnan(T) ? -INFINITY : T, Tfar = std::isnan(T) ? INFINITY : T;
    const float Pn = std::isnan(Tn) ? -INFINITY : Tn, Pf = std::isnan(Tf) ? INFINITY : Tf;
    if (!(Pn <= Tnear) || !(Pf >= Tfar)) bad = true;
    if (bad) {
        if (t.violations == 0) { t.worst[0] = q; t.worst[1] = s; t.worst[2] = org; t.worst[3] = o; t.worst[4] = d; t.worst[5] = W; }
        t.violations++;
    }
}

// one world (extent L mm from origin wo, 16-bit quantum ws), one node axis in it
struct World {
    float wo, ws, W, top;
    void make(double L, double wo_) {
        wo = (float)wo_;
        ws = (float)(L / 65535.0);
        W = chr::slab_world_bound(wo, wo, wo, ws);
        top = std::fmaf(65535.0f, ws, wo);
    }
    float coord(uint32_t q16) const { return std::fmaf((float)q16, ws, wo); }   // the reference's decode
};

float ray_origin(Rng &r, const World &w, int mode, float plane) {
    const double L = (double)w.top - (double)w.wo;
    switch (mode) {
    case 0: return (float)((double)w.wo + r.uni() * L);                          // inside
    case 1: return r.below(2) ? w.wo : w.top;                                    // on a face
    case 2: return (float)((double)w.wo - r.uni() * 10.0 * L);                   // outside, below
    case 3: return (float)((double)w.top + r.uni() * 10.0 * L);                  // outside, above
    default: return nudge(plane, (int)r.below(9) - 4);                           // cancellation: org * inv ~ -noid
    }
}

float direction(Rng &r, int cat) {
    float d = cat < NDIRS ? DIRS[cat] : (float)(0.1 + 0.9 * r.uni());
    if (cat == NDIRS + 1) d = 1.0f;
    return r.below(2) ? -d : d;
}

// the fmaxf/fminf rule the walk relies on for wild axes (slab_plane.h): NaN ignored
int nan_rule_ok() {
    const float n = NAN, i = INFINITY;
    const float tmin = std::fmax(std::fmax(std::fmax(n, -i), n), 0.0f);
    const float tmax = std::fmin(std::fmin(i, n), n);
    const float tmax3 = std::fmin(std::fmin(n, n), n);
    return tmin == 0.0f && tmax == i && std::isnan(tmax3) && !(tmin > tmax3) && std::fmax(n, 3.0f) == 3.0f &&
           std::fmin(n, 3.0f) == 3.0f;
}

}  // namespace

int main(int argc, char **argv) {
    const uint64_t ndraws = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 10000000ull;
    Rng r{argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1ull};
    Tally t;
    World w;
    // random draws
    for (uint64_t i = 0; i < ndraws; ++i) {
        const double L = std::pow(10.0, 6.0 * r.uni());   // 1 mm .. 10^6 mm
        w.make(L, r.below(4) == 0 ? -r.uni() * 3.0 * L + L : -0.5 * L * (0.5 + r.uni()));
        uint32_t qa = r.below(65536), qb = r.below(65536);
        if (qa > qb) { const uint32_t x = qa; qa = qb; qb = x; }
        if (r.below(8) == 0) { qb = qa + r.below(300); qb = qb > 65535u ? 65535u : qb; }   // small node
        if (r.below(16) == 0) qb = qa;                                                      // flat node
        if (qb < qa) qb = qa;
        const float lo = w.coord(qa), hi = w.coord(qb);
        const int bump = r.below(16) == 0 ? 1 + (int)r.below(2) : 0;
        const float s = node_quantum(lo, hi, bump, w.W);
        const float q = (float)(r.below(4) == 0 ? (r.below(2) ? 0u : 255u) : r.below(256));
        const float plane = std::fmaf(q, s, lo);
        const float o = ray_origin(r, w, (int)r.below(5), plane);
        const float d = direction(r, (int)r.below(NDIRS + 2));
        check_plane(t, q, s, lo, o, d, w.W);
    }
    const uint64_t random_planes = t.planes;
    // adversarial grid
    const double extents[] = {1.0, 10.0, 1.0e3, 4.6e4, 1.0e6};
    const uint32_t q16s[] = {0u, 1u, 255u, 32767u, 32768u, 65279u, 65534u, 65535u};
    const float qs[] = {0.0f, 1.0f, 127.0f, 128.0f, 254.0f, 255.0f};
    for (double L : extents)
        for (int centred = 0; centred < 3; ++centred) {
            w.make(L, centred == 0 ? -0.5 * L : (centred == 1 ? 0.0 : -1.0 * L));
            for (uint32_t qa : q16s)
                for (uint32_t qb : q16s) {
                    if (qb < qa) continue;
                    const float lo = w.coord(qa), hi = w.coord(qb);
                    for (int bump = 0; bump < 3; ++bump) {
                        const float s = node_quantum(lo, hi, bump, w.W);
                        for (float q : qs) {
                            const float plane = std::fmaf(q, s, lo);
                            const float os[] = {w.wo, w.top, lo, hi, plane, nudge(plane, 1), nudge(plane, -1), 0.0f,
                                                (float)(w.wo - 10.0 * L), (float)(w.top + 10.0 * L),
                                                (float)(w.wo + 0.5 * L), nudge(lo, 3), nudge(lo, -3)};
                            for (float o : os)
                                for (int cat = 0; cat < NDIRS + 2; ++cat)
                                    for (int sign = 0; sign < 2; ++sign) {
                                        float d = cat < NDIRS ? DIRS[cat] : (cat == NDIRS ? 0.1f : 1.0f);
                                        check_plane(t, q, s, lo, o, sign ? -d : d, w.W);
                                        if (cat == NDIRS) check_plane(t, q, s, lo, o, sign ? -0.57735026f : 0.57735026f, w.W);
                                    }
                        }
                    }
                }
        }
    std::printf("random_planes=%llu grid_planes=%llu wild=%llu outside_bound=%llu nonfinite=%llu violations=%llu "
                "max_ratio=%.6f max_pad_mm=%.6g nan_rule=%d first_violation=%a,%a,%a,%a,%a,%a\n",
                (unsigned long long)random_planes, (unsigned long long)(t.planes - random_planes),
                (unsigned long long)t.wild, (unsigned long long)t.outside_bound, (unsigned long long)t.nonfinite,
                (unsigned long long)t.violations, t.max_ratio, t.max_pad_mm, nan_rule_ok(), (double)t.worst[0],
                (double)t.worst[1], (double)t.worst[2], (double)t.worst[3], (double)t.worst[4], (double)t.worst[5]);
    return t.violations == 0 && nan_rule_ok() ? 0 : 1;
}
