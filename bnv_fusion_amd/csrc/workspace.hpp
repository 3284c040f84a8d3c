// Caller-provided workspaces: every entry point lays its scratch arrays into one buffer the caller allocated, as a
// sequence of typed pieces that each start on a 256-byte boundary.  The carver below is the one place that walks such
// a buffer; a layout function is a list of take<T>() calls in the order the pieces sit.  No HIP call, no allocation:
// usable on the host and inside kernels (the mesh SDF workspace is re-derived from its header on the device).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace bnv {

// size of a workspace piece: every piece starts on a 256-byte boundary
__host__ __device__ constexpr size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// Walks a workspace from `base` (256-byte aligned; may be null).  A null base yields null pieces and the same byte
// count: the size query and the binding of a layout are the same code.
struct Carver {
  char* base;
  size_t off = 0;
  __host__ __device__ explicit Carver(const void* b) : base((char*)b) {}
  // the next piece: room for `count` elements of T
  template <class T>
  __host__ __device__ T* take(size_t count) {
    T* p = base ? (T*)(base + off) : nullptr;   // (pointer arithmetic, not integers: kernels keep global loads)
    off += align256(count * sizeof(T));
    return p;
  }
  __host__ __device__ size_t bytes() const { return off; }
};

}  // namespace bnv
