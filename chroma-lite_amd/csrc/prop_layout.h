// prop_layout.h -- where the regions of one propagate's device allocation lie (propagate.hip's
// prop_bufs and launch_step).  Host-only and without a HIP include: byte offsets from the
// allocation's base, which is 256-aligned (hipMalloc), so an offset's alignment is the
// address's.  tests/host_driver_check.cpp checks bounds, overlaps and alignments.
//
//   [q0: n + 1 words][q1: n + 1 words]         queues, each behind its count header
//   [scratch, 16-aligned]                      [0..15] counters | masks (2 words per 64
//                                              positions) | offsets (1 per 64) | block prefixes
//   fused (one launch per step) only:
//   [hits, 16-aligned: one int2 per queued photon][next + pad, 16 words][keys][order]
//   [walk hist, 64 words]                      placed by the step's photon count (step_layout)
//   [sort_space, 256-aligned: keys out | values out][temp, 256-aligned]
//   [rays, 256-aligned: 2 quads per photon][rays_walk: 2 quads per photon]
//   [live[0], 256-aligned: LIVE_QUADS quads per photon][live[1]]
//   tail_masks only:
//   [tail_masks, 256-aligned: one u64 per 64 photons]
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace chr {

constexpr uint32_t LAYOUT_SCAN_WORDS = 256;   // mask words per scan block (SCAN_WORDS)
constexpr uint32_t LAYOUT_LIVE_QUADS = 4;     // 16-byte quads of a live record (LIVE_QUADS)

// u32 words of masks + offsets + block prefixes for n positions
inline uint64_t mask_scan_words(uint64_t n) {
    const uint64_t nwords = (n + 63) / 64;
    return 2 * nwords + nwords + ((uint32_t)nwords + LAYOUT_SCAN_WORDS - 1) / LAYOUT_SCAN_WORDS + 2;
}
// u32 words of a chunk launch's scratch (chr_propagate_scratch_words)
inline uint64_t chunk_scratch_words(uint32_t nthreads) { return 16 + mask_scan_words(nthreads) + 64; }

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }

struct PropLayout {
    bool fused = false;      // hits .. live[] exist
    bool has_tail_masks = false;
    uint64_t scratch_words = 0;
    size_t q[2] = {0, 0};    // the count headers; entries from + 4
    size_t scratch = 0;
    size_t hits = 0, sort_space = 0, rays = 0, rays_walk = 0, live[2] = {0, 0};
    size_t tail_masks = 0;
    size_t total = 0;
};

// nphotons sizes every region; cap = slots of one chunk; sort_temp = the binning sort's
// temporary bytes for nphotons keys
inline PropLayout prop_layout(uint32_t nphotons, uint64_t cap, bool fused, bool tail_masks, size_t sort_temp) {
    PropLayout l;
    l.fused = fused;
    l.has_tail_masks = tail_masks;
    const size_t n = nphotons;
    const uint32_t chunk_cap = (uint32_t)std::min<uint64_t>(cap, nphotons);
    l.scratch_words = chunk_scratch_words(chunk_cap);
    if (fused) l.scratch_words = std::max<uint64_t>(l.scratch_words, 16 + mask_scan_words(nphotons) + 16);
    const size_t qbytes = (n + 1) * 4;
    // hits, ray counter, binning keys / order / histogram, the sort's two arrays and temporary
    const size_t hbytes = fused ? n * 24 + 128 + 256 + 512 + sort_temp : 0;
    const size_t rbytes = fused ? n * 64 + 512 : 0;    // ray records, queue order + walk order
    const size_t lbytes = fused ? n * 128 + 512 : 0;   // live records, two buffers of 64 B per photon
    const size_t base_bytes = 2 * qbytes + l.scratch_words * 4 + 64 + hbytes + rbytes + lbytes;
    const size_t mbytes = tail_masks ? (n + 63) / 64 * 8 + 512 : 0;
    l.q[0] = 0;
    l.q[1] = qbytes;
    l.scratch = align_up(2 * qbytes, 16);
    if (fused) {
        l.hits = align_up(l.scratch + l.scratch_words * 4, 16);
        l.sort_space = align_up(l.hits + n * 8 + (16 + 2 * n + 64) * 4, 256);
        l.rays = align_up(2 * qbytes + l.scratch_words * 4 + 64 + hbytes, 256);
        l.rays_walk = l.rays + 2 * n * 16;
        l.live[0] = align_up(l.rays_walk + 2 * n * 16, 256);
        l.live[1] = l.live[0] + LAYOUT_LIVE_QUADS * n * 16;
    }
    if (tail_masks) l.tail_masks = align_up(base_bytes, 256);
    l.total = base_bytes + mbytes;
    return l;
}

// The regions one step of a fused propagate places by its photon counts: n_layout photons
// in the hits array ahead of them (a device-driven slot: the propagate's; a host step: its
// own queue length), n keys, values and sorted pairs (the step's queue length, <= n_layout).
struct StepLayout {
    size_t next, keys, order, walk_hist;   // after the hits
    size_t keys_out, vals_out, temp;       // in the sort space
};
inline StepLayout step_layout(const PropLayout &l, uint32_t n_layout, uint32_t n) {
    StepLayout s;
    s.next = l.hits + (size_t)n_layout * 8;
    s.keys = s.next + 16 * 4;
    s.order = s.keys + (size_t)n * 4;
    s.walk_hist = s.next + (16 + 2 * (size_t)n_layout) * 4;
    s.keys_out = l.sort_space;
    s.vals_out = s.keys_out + (size_t)n * 4;
    s.temp = align_up(s.vals_out + (size_t)n * 4, 256);
    return s;
}

}  // namespace chr
