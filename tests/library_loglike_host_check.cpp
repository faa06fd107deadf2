// library_loglike_host_check.cpp -- the host twin of the photon-library log-likelihood
// (csrc/library_host.cpp: chr_library_loglike_host) and its refusals in a stand-alone
// program: every array is a heap block of exactly the size the header states, so a build
// with -fsanitize=address,undefined sees any word read or written beside them.  Built
// (with library_host.cpp) and run by tests/test_library_loglike.py.
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
    const uint32_t ns = 5, nch = 7, tb = 3, nhyp = 5;
    uint32_t seed = 1u;
    std::vector<uint64_t> emitted = {100, 0, 1, 1ull << 33, 7};
    std::vector<uint32_t> counts(ns * nch), thist(ns * nch * tb);
    for (auto &c : counts) c = lcg(seed) % 4 == 0 ? 0u : lcg(seed) % 50u;
    counts[2 * nch] = (1u << 24) + 1u;
    for (auto &h : thist) h = lcg(seed) % 3 == 0 ? 0u : lcg(seed) % 6u;
    std::vector<uint32_t> offsets = {0, 0, 3, 4, 70, 70};           // the first and the last hypothesis hold nothing
    std::vector<uint32_t> source(70), nphotons(70);
    std::vector<float> t(70);
    for (uint32_t i = 0; i < 70; ++i) {
        source[i] = lcg(seed) % 7u == 6u ? 0xFFFFFFFFu : lcg(seed) % (ns + 1u);
        nphotons[i] = lcg(seed) % 5u == 0u ? 0u : lcg(seed) % 9000u;
        t[i] = lcg(seed) % 11u == 0u ? NAN : (float)(lcg(seed) % 100u) - 30.0f;
    }
    source[3] = 2u; nphotons[3] = 4000u;                          // m above 2^32 on channel 0
    const chr_library_entries en = {nhyp, offsets.data(), source.data(), nphotons.data(), t.data()};
    // the histogram covers [-4, 8): the last bin, its upper edge, NaN, both infinities among the times
    std::vector<uint32_t> nobs = {(1u << 24) + 1u, 0u, 3u, 1u, 1u, 2u, 1u};
    std::vector<float> tobs = {-40.0f, 0.0f, 60.0f, NAN, INFINITY, -INFINITY, 7.5f};

    for (int variant = 0; variant < 4; ++variant) {
        const bool has_hist = variant & 1;
        const uint32_t mode = variant >> 1;
        chr_hitmap_desc lib = {ns, (int32_t)nch, has_hist ? tb : 0u, -4.0f, has_hist ? 0.25f : 0.0f, emitted.data(),
                               counts.data(), nullptr, has_hist ? thist.data() : nullptr, nullptr, nullptr};
        const chr_library_observed obs = {nobs.data(), has_hist ? tobs.data() : nullptr, mode, 1e-3f, 1e-4f};
        std::vector<int64_t> ll(nhyp, -12345), again(nhyp, 777);
        std::vector<uint32_t> bad(nhyp, 99u), bad_again(nhyp, 5u);
        uint64_t skipped = 0;
        CHECK(chr_library_loglike_host(&lib, &en, &obs, ll.data(), bad.data(), &skipped) == CHR_OK);
        CHECK(skipped > 0);
        const uint64_t once = skipped;
        CHECK(ll[0] == ll[4]);                                    // two hypotheses without entries: the floor alone
        CHECK(ll[0] != -12345 && ll[2] != ll[0] && ll[3] != ll[0]);
        for (uint32_t h = 0; h < nhyp; ++h) {
            CHECK(bad[h] == 0u);
            CHECK(ll[h] <= (int64_t)nch << 43 && ll[h] >= -((int64_t)nch << 43));
        }
        // written, not added to: other garbage, the same words; skipped is added to
        CHECK(chr_library_loglike_host(&lib, &en, &obs, again.data(), bad_again.data(), &skipped) == CHR_OK);
        CHECK(again == ll && bad_again == bad && skipped == 2 * once);
        // zero floors: m == 0 meets n > 0; an infinite floor makes the Poisson term a NaN
        chr_library_observed edge = obs;
        edge.floor = 0.0f; edge.tfloor = 0.0f;
        CHECK(chr_library_loglike_host(&lib, &en, &edge, again.data(), bad_again.data(), &skipped) == CHR_OK);
        CHECK(again[0] == -((int64_t)6 << 43));                   // six channels saw light where none is expected
        edge.floor = INFINITY;
        CHECK(chr_library_loglike_host(&lib, &en, &edge, again.data(), bad_again.data(), &skipped) == CHR_OK);
        CHECK(bad_again[0] == (mode == 0u ? 6u : 0u));

        // the refusals, each from the accepted call above, the outputs untouched
        const std::vector<int64_t> ll0 = again;
        const uint64_t skipped0 = skipped;
        chr_hitmap_desc off = lib;
        off.nchannels = 0;
        CHECK(chr_library_loglike_host(&off, &en, &obs, again.data(), bad_again.data(), &skipped) == CHR_ERR_INVALID);
        off = lib; off.nchannels = (1 << 20) + 1;
        CHECK(chr_library_loglike_host(&off, &en, &obs, again.data(), bad_again.data(), &skipped) == CHR_ERR_INVALID);
        off = lib; off.d_counts = nullptr;
        CHECK(chr_library_loglike_host(&off, &en, &obs, again.data(), bad_again.data(), &skipped) == CHR_ERR_INVALID);
        off = lib; off.ntbins = has_hist ? 0u : 2u;
        CHECK(chr_library_loglike_host(&off, &en, &obs, again.data(), bad_again.data(), &skipped) == CHR_ERR_INVALID);
        CHECK(chr_library_loglike_host(&lib, &en, nullptr, again.data(), bad_again.data(), &skipped) == CHR_ERR_INVALID);
        CHECK(chr_library_loglike_host(&lib, &en, &obs, nullptr, bad_again.data(), &skipped) == CHR_ERR_INVALID);
        CHECK(chr_library_loglike_host(&lib, &en, &obs, again.data(), nullptr, &skipped) == CHR_ERR_INVALID);
        CHECK(chr_library_loglike_host(&lib, &en, &obs, again.data(), bad_again.data(), nullptr) == CHR_ERR_INVALID);
        CHECK(chr_library_loglike_host(&lib, nullptr, &obs, again.data(), bad_again.data(), &skipped) == CHR_ERR_INVALID);
        chr_library_observed wrong = obs;
        wrong.nobs = nullptr;
        CHECK(chr_library_loglike_host(&lib, &en, &wrong, again.data(), bad_again.data(), &skipped) == CHR_ERR_INVALID);
        wrong = obs; wrong.mode = 2u;
        CHECK(chr_library_loglike_host(&lib, &en, &wrong, again.data(), bad_again.data(), &skipped) == CHR_ERR_INVALID);
        wrong = obs; wrong.floor = -1.0f;
        CHECK(chr_library_loglike_host(&lib, &en, &wrong, again.data(), bad_again.data(), &skipped) == CHR_ERR_INVALID);
        wrong = obs; wrong.tfloor = NAN;
        CHECK(chr_library_loglike_host(&lib, &en, &wrong, again.data(), bad_again.data(), &skipped) == CHR_ERR_INVALID);
        if (!has_hist) {
            wrong = obs; wrong.tobs = tobs.data();                // times, but no histogram to look them up in
            CHECK(chr_library_loglike_host(&lib, &en, &wrong, again.data(), bad_again.data(), &skipped) == CHR_ERR_INVALID);
        }
        std::vector<uint32_t> down = offsets;
        down[2] = 5;                                              // 0, 0, 5, 4, 70, 70
        const chr_library_entries en_down = {nhyp, down.data(), source.data(), nphotons.data(), t.data()};
        CHECK(chr_library_loglike_host(&lib, &en_down, &obs, again.data(), bad_again.data(), &skipped) == CHR_ERR_INVALID);
        CHECK(chr::last_error().find("ascending") != std::string::npos);
        const chr_library_entries none = {0, nullptr, nullptr, nullptr, nullptr};
        CHECK(chr_library_loglike_host(&lib, &none, &obs, again.data(), bad_again.data(), &skipped) == CHR_OK);
        CHECK(again == ll0 && skipped == skipped0);
    }
    printf("variants=4 failures=%ld\n", failures);
    return failures ? 1 : 0;
}
