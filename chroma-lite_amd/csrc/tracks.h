// tracks.h -- photon tracks recorded on the device (chr_propagate_tracked): the
// handle, and the launches of tracks.hip that the host driver in propagate.hip
// queues between its steps.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/chroma_amd.h"

// Track record, CHR_TRACK_WORDS u32 words, 64-byte aligned (the layout idea of
// the live record): [0] photon id, [1] history, [2..4] pos,
// [5..7] dir, [8..10] pol, [11] wavelength, [12] t, [13] weight, [14] last-hit
// triangle, [15] entry index k (0: the input state, k: the state after k steps).
struct chr_tracks {
    uint32_t nphotons = 0;            // photons of the propagate (ids are below it)
    uint64_t nrecords = 0;
    std::vector<uint64_t> counts;     // records of every entry (its queue length)
    int device = 0;
    uint64_t capacity = 0;            // records d_step holds (grown geometrically)
    uint4 *d_step = nullptr;          // step-major: entry 0's records, entry 1's, ... each in queue order
    uint64_t *d_step_offsets = nullptr;   // nentries + 1
    uint4 *d_flat = nullptr;          // photon-major: photon 0's records by entry, photon 1's, ...
    uint64_t *d_flat_offsets = nullptr;   // nphotons + 1
    ~chr_tracks();
};

namespace chr {

// entry k of the tracks: one record per position of `queue` (n ids), written to
// records[0 .. n), and track_len[id] = k + 1; a queue word >= nphotons is
// counted in *bad and not followed
int tracks_record(const chr_photons *ph, const uint32_t *queue, uint32_t n, uint32_t nphotons, uint32_t k,
                  uint4 *records, uint32_t *track_len, uint32_t *bad, hipStream_t stream);
// offsets[0 .. nphotons] = exclusive scan of track_len[0 .. nphotons] (track_len[nphotons] must be 0)
int tracks_offsets(const uint32_t *track_len, uint32_t nphotons, uint64_t *offsets, hipStream_t stream);
// record r of the step-major buffer -> position offsets[id] + k of the photon-major one
int tracks_transpose(const uint4 *step, uint64_t nrecords, const uint64_t *offsets, uint32_t nphotons, uint4 *flat,
                     uint32_t *bad, hipStream_t stream);

}  // namespace chr
