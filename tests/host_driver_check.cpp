// host_driver_check.cpp -- the propagate drivers' buffer layout (csrc/prop_layout.h) and
// grow-on-demand buffers (csrc/grow_buffer.h), checked on the host: the two headers are the
// text propagate.hip compiles.  Built and run by tests/test_host_driver.py.
//
// Layout: for every input, each region is inside the allocation, aligned as its user casts
// it, at least as large as its user touches, and disjoint from every other region.
// Buffer: a failed grow reports its error and leaves no size behind.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "grow_buffer.h"
#include "prop_layout.h"

using namespace chr;

static long violations = 0;
static std::string first_violation = "none";

static void fail(const std::string &what) {
    if (!violations) first_violation = what;
    violations++;
}

struct Region {
    const char *name;
    size_t off, size, align;
};

static std::string describe(const char *what, const Region &r, uint32_t n, uint64_t cap, bool fused, bool masks,
                            size_t temp, uint32_t n_layout, uint32_t n_step) {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s:%s:n=%u:cap=%llu:fused=%d:masks=%d:temp=%zu:n_layout=%u:n_step=%u", what, r.name, n,
             (unsigned long long)cap, (int)fused, (int)masks, temp, n_layout, n_step);
    return buf;
}

// one propagate of n photons; a step over n_step queued photons whose hits array holds n_layout
static void check_layout(uint32_t n, uint64_t cap, bool fused, bool masks, size_t temp, uint32_t n_layout,
                         uint32_t n_step) {
    const PropLayout l = prop_layout(n, cap, fused, masks, temp);
    const StepLayout s = step_layout(l, n_layout, n_step);
    const size_t N = n;
    // the scratch words a launch over m positions touches: counters, masks, offsets, block prefixes
    const uint32_t m = fused ? n : (uint32_t)std::min<uint64_t>(cap, n);
    const size_t mw = ((size_t)m + 63) / 64;
    const size_t scratch_need = (16 + 2 * mw + mw + (mw + 255) / 256 + 2) * 4;
    std::vector<Region> r;
    r.push_back({"q0", l.q[0], (N + 1) * 4, 4});
    r.push_back({"q1", l.q[1], (N + 1) * 4, 4});
    r.push_back({"scratch", l.scratch, scratch_need, 16});
    r.push_back({"mask_words", l.scratch + 16 * 4, 2 * mw * 4, 8});
    if (fused) {
        r.push_back({"hits", l.hits, (size_t)n_layout * 8, 16});
        r.push_back({"next", s.next, 16 * 4, 4});
        r.push_back({"keys", s.keys, (size_t)n_step * 4, 4});
        r.push_back({"order", s.order, (size_t)n_step * 4, 4});
        r.push_back({"walk_hist", s.walk_hist, 64 * 4, 4});
        r.push_back({"keys_out", s.keys_out, (size_t)n_step * 4, 256});
        r.push_back({"vals_out", s.vals_out, (size_t)n_step * 4, 4});
        r.push_back({"temp", s.temp, temp, 256});
        r.push_back({"rays", l.rays, 2 * N * 16, 256});
        r.push_back({"rays_walk", l.rays_walk, 2 * N * 16, 16});
        r.push_back({"live0", l.live[0], LAYOUT_LIVE_QUADS * N * 16, 256});
        r.push_back({"live1", l.live[1], LAYOUT_LIVE_QUADS * N * 16, 16});
    }
    if (masks) r.push_back({"tail_masks", l.tail_masks, (N + 63) / 64 * 8, 256});
    if (l.scratch_words * 4 < scratch_need) fail(describe("scratch_words", r[2], n, cap, fused, masks, temp, n_layout, n_step));
    // the whole hits region as the kernels of a full step use it: n hits, then 16 + 2n + 64 words
    if (fused && l.hits + N * 8 + (16 + 2 * N + 64) * 4 > l.sort_space)
        fail(describe("hits_region", r[4], n, cap, fused, masks, temp, n_layout, n_step));
    for (size_t i = 0; i < r.size(); ++i) {
        if (r[i].off % r[i].align) fail(describe("align", r[i], n, cap, fused, masks, temp, n_layout, n_step));
        if (r[i].off + r[i].size > l.total) fail(describe("bounds", r[i], n, cap, fused, masks, temp, n_layout, n_step));
        for (size_t j = i + 1; j < r.size(); ++j) {
            const bool nested = (i == 2 && j == 3);   // the mask words are part of the scratch
            if (!nested && r[i].size && r[j].size && r[i].off < r[j].off + r[j].size && r[j].off < r[i].off + r[i].size)
                fail(describe("overlap", r[i], n, cap, fused, masks, temp, n_layout, n_step) + "/" + r[j].name);
        }
    }
}

// an allocator that counts and fails on demand
static int allocs = 0, releases = 0;
static bool alloc_fails = false, release_fails = false;
static int fake_alloc(void **p, size_t n) {
    if (alloc_fails) return 7;
    allocs++;
    *p = malloc(n ? n : 1);
    return *p ? 0 : 7;
}
static int fake_release(void *p) {
    releases++;
    free(p);
    return release_fails ? 9 : 0;
}

static void expect(bool ok, const char *what) {
    if (!ok) fail(std::string("pool:") + what);
}

static void check_pool() {
    GrowBuffer x;
    expect(grow_buffer(x, 100, fake_alloc, fake_release) == 0 && x.ptr && x.bytes == 100 && allocs == 1, "first grow");
    void *p = x.ptr;
    expect(grow_buffer(x, 50, fake_alloc, fake_release) == 0 && x.ptr == p && allocs == 1 && releases == 0,
           "a request that fits allocates nothing");
    expect(grow_buffer(x, 100, fake_alloc, fake_release) == 0 && x.ptr == p && allocs == 1, "an equal request fits");
    alloc_fails = true;
    expect(grow_buffer(x, 200, fake_alloc, fake_release) == 7, "a failed grow returns the allocator's error");
    expect(x.ptr == nullptr && x.bytes == 0 && releases == 1, "a failed grow leaves the buffer empty");
    const int rc = grow_buffer(x, 50, fake_alloc, fake_release);
    expect(!(rc == 0 && x.ptr == nullptr), "a smaller request after a failed grow: success with a null pointer");
    expect(rc == 7 && x.bytes == 0, "a smaller request after a failed grow asks the allocator again");
    alloc_fails = false;
    expect(grow_buffer(x, 50, fake_alloc, fake_release) == 0 && x.ptr && x.bytes == 50 && allocs == 2, "grow after recovery");
    release_fails = true;
    expect(grow_buffer(x, 60, fake_alloc, fake_release) == 9 && x.ptr == nullptr && x.bytes == 0 && allocs == 2,
           "a failed release returns its error and leaves the buffer empty");
    release_fails = false;
    expect(grow_buffer(x, 10, fake_alloc, fake_release) == 0 && x.ptr && x.bytes == 10, "grow after a failed release");
    free(x.ptr);
}

int main() {
    const uint32_t counts[] = {1, 63, 64, 65, 4095, 4096, 4097, (1u << 20) - 1, 1u << 20, (1u << 20) + 1, 10000000};
    struct { uint64_t cap; bool fused; } shapes[] = {
        {64 * 64, true}, {100 * 41, false}, {512 * 1024, true},
        {64 * 64, false},   // a fused shape with one launch per chunk (CHR_STEP_LAUNCH=0)
    };
    const size_t temps[] = {0, 1, (size_t)1 << 26};
    long layouts = 0;
    for (uint32_t n : counts)
        for (const auto &sh : shapes)
            for (size_t temp : temps)
                for (int masks = 0; masks < 2; ++masks) {
                    // the step's queue: all photons, about half, one; placed by the propagate's count
                    // (device-driven slots) or by its own (host steps)
                    const uint32_t steps[] = {n, n / 2 + 1, 1};
                    for (uint32_t ns : steps) {
                        check_layout(n, sh.cap, sh.fused, masks != 0, temp, n, ns);
                        check_layout(n, sh.cap, sh.fused, masks != 0, temp, ns, ns);
                        layouts += 2;
                    }
                }
    check_pool();
    printf("layouts=%ld violations=%ld first_violation=%s\n", layouts, violations, first_violation.c_str());
    return violations ? 1 : 0;
}
