// library_host_check.cpp -- the host twins of the photon-library lookup
// (csrc/library_host.cpp: chr_library_expect_host, chr_library_sample_host) and their
// refusals in a stand-alone program: every array is a heap block of exactly the size the
// header states, so a build with -fsanitize=address,undefined sees any word read or
// written beside them.  Built (with library_host.cpp) and run by tests/test_library.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"

std::string &chr::last_error() {
    static thread_local std::string s;
    return s;
}

static long failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            if (!failures) printf("first failure: %s (line %d)\n", #cond, __LINE__); \
            failures++;                                               \
        }                                                             \
    } while (0)

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

int main() {
    const uint32_t ns = 5, nch = 7, tb = 3, nev = 4, nslots = 6;
    uint32_t seed = 1u;
    std::vector<uint64_t> emitted = {100, 0, 1, 1ull << 33, 7};
    std::vector<uint32_t> counts(ns * nch), tmin(ns * nch), thist(ns * nch * tb);
    for (auto &c : counts) c = lcg(seed) % 4 == 0 ? 0u : lcg(seed) % 50u;
    counts[2 * nch] = (1u << 24) + 1u;
    for (auto &k : tmin) k = lcg(seed) % 5 == 0 ? 0xFFFFFFFFu : 0x80000000u ^ (0x41000000u + lcg(seed) % 0x01000000u);
    tmin[3] = 0x3EFFFFFFu;                                        // a negative time
    for (auto &h : thist) h = lcg(seed) % 3 == 0 ? 0u : lcg(seed) % 6u;
    std::vector<uint32_t> offsets = {0, 0, 3, 4, 70};
    std::vector<uint32_t> source(70), nphotons(70);
    std::vector<float> t(70);
    for (uint32_t i = 0; i < 70; ++i) {
        source[i] = lcg(seed) % 7u == 6u ? 0xFFFFFFFFu : lcg(seed) % (ns + 1u);
        nphotons[i] = lcg(seed) % 5u == 0u ? 0u : lcg(seed) % 9000u;
        t[i] = lcg(seed) % 11u == 0u ? NAN : (float)(lcg(seed) % 100u) - 30.0f;
    }
    source[3] = 2u; nphotons[3] = 4000u;                          // m above 2^32 on channel 0
    const chr_library_entries en = {nev, offsets.data(), source.data(), nphotons.data(), t.data()};

    for (int variant = 0; variant < 4; ++variant) {
        const bool has_tmin = variant & 1, has_hist = variant & 2;
        chr_hitmap_desc lib = {ns, (int32_t)nch, has_hist ? tb : 0u, -4.0f, has_hist ? 0.25f : 0.0f, emitted.data(),
                               counts.data(), has_tmin ? tmin.data() : nullptr, has_hist ? thist.data() : nullptr,
                               nullptr, nullptr};
        std::vector<float> mu(nev * nch, -1.0f), tfirst(nev * nch, -1.0f), ts(nev * nch, -1.0f);
        std::vector<uint32_t> n(nev * nch, 77u), rng(6 * nslots);
        for (auto &w : rng) w = lcg(seed);
        const std::vector<uint32_t> rng0 = rng;
        uint64_t skipped = 0;
        CHECK(chr_library_expect_host(&lib, &en, mu.data(), has_tmin ? tfirst.data() : nullptr, &skipped) == CHR_OK);
        CHECK(skipped > 0);
        for (uint32_t c = 0; c < nch; ++c) CHECK(mu[c] == 0.0f && (!has_tmin || std::isinf(tfirst[c])));   // event 0: no entries
        bool lit = false;
        for (float m : mu) { CHECK(m >= 0.0f); lit |= m > 0.0f; }
        CHECK(lit);
        const uint64_t once = skipped;
        CHECK(chr_library_sample_host(&lib, &en, rng.data(), nslots, n.data(), ts.data(), &skipped) == CHR_OK);
        CHECK(skipped == 2 * once);
        CHECK(rng != rng0);
        for (uint32_t k = 0; k < nev * nch; ++k) CHECK((n[k] == 0u) == (ts[k] == 1e9f));
        // more slots than pairs: the states beyond the pairs stay
        std::vector<uint32_t> big(6 * 40);
        for (auto &w : big) w = lcg(seed);
        const std::vector<uint32_t> big0 = big;
        CHECK(chr_library_sample_host(&lib, &en, big.data(), 40, n.data(), ts.data(), &skipped) == CHR_OK);
        for (uint32_t w = 0; w < 6; ++w)
            for (uint32_t s = nev * nch; s < 40; ++s) CHECK(big[w * 40 + s] == big0[w * 40 + s]);

        // the refusals, each from the accepted call above
        chr_hitmap_desc bad = lib;
        bad.nchannels = 0;
        CHECK(chr_library_expect_host(&bad, &en, mu.data(), tfirst.data(), &skipped) == CHR_ERR_INVALID);
        bad = lib; bad.nsources = 0;
        CHECK(chr_library_sample_host(&bad, &en, rng.data(), nslots, n.data(), ts.data(), &skipped) == CHR_ERR_INVALID);
        bad = lib; bad.d_counts = nullptr;
        CHECK(chr_library_expect_host(&bad, &en, mu.data(), tfirst.data(), &skipped) == CHR_ERR_INVALID);
        bad = lib; bad.ntbins = has_hist ? 0u : 2u;
        CHECK(chr_library_expect_host(&bad, &en, mu.data(), tfirst.data(), &skipped) == CHR_ERR_INVALID);
        CHECK(chr_library_expect_host(&lib, &en, nullptr, tfirst.data(), &skipped) == CHR_ERR_INVALID);
        CHECK(chr_library_expect_host(&lib, &en, mu.data(), tfirst.data(), nullptr) == CHR_ERR_INVALID);
        CHECK(chr_library_sample_host(&lib, &en, rng.data(), 0, n.data(), ts.data(), &skipped) == CHR_ERR_INVALID);
        CHECK(chr_library_sample_host(&lib, &en, nullptr, nslots, n.data(), ts.data(), &skipped) == CHR_ERR_INVALID);
        CHECK(chr_library_sample_host(&lib, nullptr, rng.data(), nslots, n.data(), ts.data(), &skipped) == CHR_ERR_INVALID);
        std::vector<uint32_t> down = offsets;
        down[2] = 5;                                              // 0, 0, 5, 4, 70
        const chr_library_entries en_down = {nev, down.data(), source.data(), nphotons.data(), t.data()};
        CHECK(chr_library_expect_host(&lib, &en_down, mu.data(), tfirst.data(), &skipped) == CHR_ERR_INVALID);
        CHECK(chr::last_error().find("ascending") != std::string::npos);
        const chr_library_entries none = {0, nullptr, nullptr, nullptr, nullptr};
        CHECK(chr_library_expect_host(&lib, &none, mu.data(), tfirst.data(), &skipped) == CHR_OK);
        CHECK(skipped == 3 * once);
    }
    printf("variants=4 failures=%ld\n", failures);
    return failures ? 1 : 0;
}
