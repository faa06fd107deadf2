// grow_buffer.h -- the grow step of the buffers the drivers keep per thread, device and
// context and enlarge on demand (propagate.hip's pool_get).  Host-only and without a HIP
// include: allocate and free are passed in, so tests/host_driver_check.cpp drives it with an
// allocator that fails.
#pragma once

#include <cstddef>

namespace chr {

struct GrowBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;   // never more than ptr holds: 0 from the moment the old block is given up
};

// x.ptr holds at least `bytes` on return 0; no call of alloc or release when it already does.
// alloc(void **, size_t) and release(void *) return 0 or an error code, which is returned:
// the buffer is then empty (bytes 0), so no later, smaller request takes it for a fit.
template <class Alloc, class Release>
int grow_buffer(GrowBuffer &x, size_t bytes, Alloc alloc, Release release) {
    if (x.bytes >= bytes) return 0;
    x.bytes = 0;
    if (x.ptr) {
        void *old = x.ptr;
        x.ptr = nullptr;
        if (int rc = release(old)) return rc;
    }
    void *p = nullptr;
    if (int rc = alloc(&p, bytes)) return rc;
    x.ptr = p;
    x.bytes = bytes;
    return 0;
}

}  // namespace chr
