// tracks.hip -- photon tracks recorded on the device (gfx950).
//
// replaces: the per-step gather and download of GPUPhotons.propagate(track=True)
// (chroma/gpu/photon.py:252-293: copy_queue of the nine arrays, nine .get() and the
// queue's .get() after every step) and the per-record Python of Simulation's track
// building (chroma/sim.py:77-93).  The host driver, chr_propagate_tracked, is in
// propagate.hip next to chr_propagate; it queues track_record_kernel once per entry.
// After the last step an exclusive scan of the track lengths gives every photon's
// offset and track_transpose_kernel writes the photon-major copy.  No kernel here has
// a loop, reads device data as a bound, or uses LDS.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <cstdint>
#include <cstring>
#include <new>

#include "common.h"
#include "tracks.h"

namespace chr {

constexpr int TRACK_BLOCK = 256;

struct TrackPhotons {
    const float *pos, *dir, *pol, *wl, *t, *weights;
    const uint32_t *flags;
    const int32_t *last_hit;
};

// One work-item per queue position: the id (coalesced), the nine arrays gathered at
// it, the record as four 16-byte stores (a wave writes 4 KB contiguous), and the
// photon's track length so far.  An id is in a step's queue at most once and the
// entries are ordered on the stream: track_len needs no atomic.
__global__ __launch_bounds__(TRACK_BLOCK) void track_record_kernel(TrackPhotons ph, const uint32_t *__restrict__ queue,
                                                                   uint32_t n, uint32_t nphotons, uint32_t k,
                                                                   uint4 *__restrict__ records,
                                                                   uint32_t *__restrict__ track_len,
                                                                   uint32_t *__restrict__ bad) {
    const uint32_t i = blockIdx.x * TRACK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = queue[i];
    if (id >= nphotons) {   // not a photon of this propagate: nothing is read at it
        atomicAdd(bad, 1u);
        return;
    }
    const size_t v = 3 * (size_t)id;
    uint4 w0, w1, w2, w3;
    w0.x = id;
    w0.y = ph.flags[id];
    w0.z = __float_as_uint(ph.pos[v]);
    w0.w = __float_as_uint(ph.pos[v + 1]);
    w1.x = __float_as_uint(ph.pos[v + 2]);
    w1.y = __float_as_uint(ph.dir[v]);
    w1.z = __float_as_uint(ph.dir[v + 1]);
    w1.w = __float_as_uint(ph.dir[v + 2]);
    w2.x = __float_as_uint(ph.pol[v]);
    w2.y = __float_as_uint(ph.pol[v + 1]);
    w2.z = __float_as_uint(ph.pol[v + 2]);
    w2.w = __float_as_uint(ph.wl[id]);
    w3.x = __float_as_uint(ph.t[id]);
    w3.y = __float_as_uint(ph.weights[id]);
    w3.z = (uint32_t)ph.last_hit[id];
    w3.w = k;
    uint4 *r = records + 4 * (size_t)i;
    r[0] = w0;
    r[1] = w1;
    r[2] = w2;
    r[3] = w3;
    track_len[id] = k + 1u;
}

// Four work-items per record, one 16-byte quarter each: the step-major buffer is read
// at the work-item's own index (coalesced), the record's id and entry index come from
// the first and last quarter by wave shuffles, and the four lanes write one aligned
// 64-byte record at offsets[id] + k.  A photon queued at step k was queued at every
// earlier step, so its rank in its own track is k.
__global__ __launch_bounds__(TRACK_BLOCK) void track_transpose_kernel(const uint4 *__restrict__ step, uint64_t nquads,
                                                                      const uint64_t *__restrict__ offsets,
                                                                      uint32_t nphotons, uint4 *__restrict__ flat,
                                                                      uint32_t *__restrict__ bad) {
    const uint64_t q = (uint64_t)blockIdx.x * TRACK_BLOCK + threadIdx.x;
    const bool in = q < nquads;   // nquads is a multiple of 4: the four lanes of a record agree
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (in) w = step[q];
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t id = (uint32_t)__shfl((int)w.x, lane & ~3);
    const uint32_t k = (uint32_t)__shfl((int)w.w, lane | 3);
    if (!in) return;
    if (id >= nphotons) {
        if ((lane & 3) == 0) atomicAdd(bad, 1u);
        return;
    }
    const uint64_t lo = offsets[id], hi = offsets[id + 1];
    if (hi < lo || k >= hi - lo || 4 * hi > nquads) {   // beyond the photon's track or the buffer: never written
        if ((lane & 3) == 0) atomicAdd(bad, 1u);
        return;
    }
    flat[4 * (lo + k) + (uint64_t)(lane & 3)] = w;
}

struct WidenLen {
    __host__ __device__ uint64_t operator()(uint32_t x) const { return (uint64_t)x; }
};

int tracks_record(const chr_photons *ph, const uint32_t *queue, uint32_t n, uint32_t nphotons, uint32_t k,
                  uint4 *records, uint32_t *track_len, uint32_t *bad, hipStream_t stream) {
    if (n == 0) return CHR_OK;
    const TrackPhotons tp{ph->d_pos, ph->d_dir, ph->d_pol, ph->d_wavelengths, ph->d_t, ph->d_weights, ph->d_flags,
                          ph->d_last_hit_triangles};
    const unsigned blocks = (unsigned)(((uint64_t)n + TRACK_BLOCK - 1) / TRACK_BLOCK);
    hipLaunchKernelGGL(track_record_kernel, dim3(blocks), dim3(TRACK_BLOCK), 0, stream, tp, queue, n, nphotons, k,
                       records, track_len, bad);
    CHR_HIP_CHECK(hipGetLastError());
    return CHR_OK;
}

int tracks_offsets(const uint32_t *track_len, uint32_t nphotons, uint64_t *offsets, hipStream_t stream) {
    auto in = rocprim::make_transform_iterator(track_len, WidenLen());
    const size_t n = (size_t)nphotons + 1;
    size_t temp_bytes = 0;
    CHR_HIP_CHECK(rocprim::exclusive_scan(nullptr, temp_bytes, in, offsets, (uint64_t)0, n, rocprim::plus<uint64_t>(),
                                          stream));
    void *temp = nullptr;
    CHR_HIP_CHECK(hipMalloc(&temp, temp_bytes ? temp_bytes : 16));
    const hipError_t e = rocprim::exclusive_scan(temp, temp_bytes, in, offsets, (uint64_t)0, n,
                                                 rocprim::plus<uint64_t>(), stream);
    const hipError_t f = hipFree(temp);   // waits for the scan
    CHR_HIP_CHECK(e);
    CHR_HIP_CHECK(f);
    return CHR_OK;
}

int tracks_transpose(const uint4 *step, uint64_t nrecords, const uint64_t *offsets, uint32_t nphotons, uint4 *flat,
                     uint32_t *bad, hipStream_t stream) {
    if (nrecords == 0) return CHR_OK;
    const uint64_t nquads = 4 * nrecords;
    const uint64_t blocks = (nquads + TRACK_BLOCK - 1) / TRACK_BLOCK;
    if (blocks > 0x7FFFFFFFull) return chr::fail(CHR_ERR_INVALID, "tracks_transpose: %llu records are too many",
                                                 (unsigned long long)nrecords);
    hipLaunchKernelGGL(track_transpose_kernel, dim3((unsigned)blocks), dim3(TRACK_BLOCK), 0, stream, step, nquads,
                       offsets, nphotons, flat, bad);
    CHR_HIP_CHECK(hipGetLastError());
    return CHR_OK;
}

}  // namespace chr

// ---------------------------------------------------------------- the handle
chr_tracks::~chr_tracks() {
    // a handle may be freed on another thread than made it, never on another device's memory
    int dev = 0;
    const bool have = d_step || d_step_offsets || d_flat || d_flat_offsets;
    if (have && hipGetDevice(&dev) == hipSuccess && dev != device) (void)hipSetDevice(device);
    if (d_step) (void)hipFree(d_step);
    if (d_step_offsets) (void)hipFree(d_step_offsets);
    if (d_flat) (void)hipFree(d_flat);
    if (d_flat_offsets) (void)hipFree(d_flat_offsets);
    if (have && dev != device) (void)hipSetDevice(dev);
}

// replaces: len(step_photon_ids) and the lengths of its arrays (photon.py:252-293)
extern "C" int chr_tracks_info(const chr_tracks *t, uint32_t *nentries, uint64_t *nrecords, uint32_t *nphotons) {
    if (!t) return chr::fail(CHR_ERR_INVALID, "chr_tracks_info: null handle");
    if (nentries) *nentries = (uint32_t)t->counts.size();
    if (nrecords) *nrecords = t->nrecords;
    if (nphotons) *nphotons = t->nphotons;
    return CHR_OK;
}

// replaces: [len(ids) for ids in step_photon_ids] (photon.py:252-293)
extern "C" int chr_tracks_entry_counts(const chr_tracks *t, uint64_t *h_counts) {
    if (!t) return chr::fail(CHR_ERR_INVALID, "chr_tracks_entry_counts: null handle");
    if (!h_counts) return chr::fail(CHR_ERR_INVALID, "chr_tracks_entry_counts: null argument");
    if (!t->counts.empty()) std::memcpy(h_counts, t->counts.data(), t->counts.size() * sizeof(uint64_t));
    return CHR_OK;
}

static int tracks_order(const char *fn, const chr_tracks *t, int32_t order) {
    if (!t) return chr::fail(CHR_ERR_INVALID, "%s: null handle", fn);
    if (order != 0 && order != 1)
        return chr::fail(CHR_ERR_INVALID, "%s: order must be 0 (step-major) or 1 (photon-major), got %d", fn, order);
    return CHR_OK;
}

// replaces: nothing in the reference (photon.py:252-293 keeps no device copy): the
// records and offsets where they are, for device-side consumers.  The pointers are
// NULL for an empty buffer and live as long as the handle.
extern "C" int chr_tracks_device(const chr_tracks *t, int32_t order, const uint32_t **d_records,
                                 const uint64_t **d_offsets) {
    CHR_TRY(tracks_order("chr_tracks_device", t, order));
    if (d_records) *d_records = (const uint32_t *)(order ? t->d_flat : t->d_step);
    if (d_offsets) *d_offsets = order ? t->d_flat_offsets : t->d_step_offsets;
    return CHR_OK;
}

// replaces: the per-step downloads of photon.py:252-293 (step_photon_ids.append(...get()),
// step_photons.append(...get())) with one download of all records
extern "C" int chr_tracks_copy(const chr_tracks *t, int32_t order, uint32_t *h_records, uint64_t *h_offsets) {
    CHR_TRY(tracks_order("chr_tracks_copy", t, order));
    const uint4 *rec = order ? t->d_flat : t->d_step;
    const uint64_t *off = order ? t->d_flat_offsets : t->d_step_offsets;
    const size_t noff = (order ? (size_t)t->nphotons : t->counts.size()) + 1;
    if (h_records && t->nrecords) {
        if (!rec) return chr::fail(CHR_ERR_INTERNAL, "chr_tracks_copy: the handle holds no records");
        CHR_HIP_CHECK(hipMemcpy(h_records, rec, (size_t)t->nrecords * CHR_TRACK_WORDS * 4, hipMemcpyDeviceToHost));
    }
    if (h_offsets) {
        if (off) CHR_HIP_CHECK(hipMemcpy(h_offsets, off, noff * 8, hipMemcpyDeviceToHost));
        else std::memset(h_offsets, 0, noff * 8);   // an empty handle: every offset is 0
    }
    return CHR_OK;
}

extern "C" int chr_tracks_free(chr_tracks *t) {
    delete t;
    return CHR_OK;
}
