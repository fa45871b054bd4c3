// Owners of the library's device and pinned host memory (host-only, internal).  Move-only; the destructor and reset() free and ignore
// the error; alloc() frees any block held first, and on failure the object is empty -- never dangling, never the old block.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stddef.h>
#include <string.h>

namespace se3tn {

template <class T>
class DeviceBuf {   // hipMalloc memory
 public:
  DeviceBuf() = default;
  DeviceBuf(DeviceBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DeviceBuf& operator=(DeviceBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  ~DeviceBuf() { reset(); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr; n_ = 0;
  }
  hipError_t alloc(size_t count, bool zero = false) {
    reset();
    hipError_t e = hipMalloc((void**)&p_, count * sizeof(T));
    if (e != hipSuccess) { p_ = nullptr; return e; }
    n_ = count;
    if (zero && (e = hipMemset(p_, 0, count * sizeof(T))) != hipSuccess) reset();
    return e;
  }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  size_t count() const { return n_; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

template <class T>
class PinnedBuf {   // hipHostMalloc memory: default, or mapped (then dev() is the address the device reaches it by)
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_), d_(o.d_), n_(o.n_) { o.p_ = o.d_ = nullptr; o.n_ = 0; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; d_ = o.d_; n_ = o.n_; o.p_ = o.d_ = nullptr; o.n_ = 0; }
    return *this;
  }
  ~PinnedBuf() { reset(); }
  void reset() {
    if (p_) (void)hipHostFree(p_);
    p_ = d_ = nullptr; n_ = 0;
  }
  hipError_t alloc(size_t count, bool zero = false, bool mapped = false) {
    reset();
    hipError_t e = hipHostMalloc((void**)&p_, count * sizeof(T), mapped ? hipHostMallocMapped : hipHostMallocDefault);
    if (e != hipSuccess) { p_ = nullptr; return e; }
    n_ = count;
    if (zero) memset(p_, 0, count * sizeof(T));
    if (mapped && (e = hipHostGetDevicePointer((void**)&d_, p_, 0)) != hipSuccess) reset();
    return e;
  }
  T* get() const { return p_; }
  T* dev() const { return d_; }
  explicit operator bool() const { return p_ != nullptr; }
  size_t count() const { return n_; }

 private:
  T *p_ = nullptr, *d_ = nullptr;
  size_t n_ = 0;
};

// The rasteriser's scratch for `instances` instances of meshes of up to V vertices / F triangles: clip positions and snapped window
// coordinates per vertex, the queues of large triangles and of triangles that cross the frustum (raster_vertex_kernel, raster_queue_kernel)
struct RasterScratch {
  DeviceBuf<float4> vpost;
  DeviceBuf<int4> vsnap;
  DeviceBuf<int> big, clipq;   // [1 + F] each
  hipError_t alloc(int V, int F, int instances) {
    hipError_t e = vpost.alloc((size_t)V * instances);
    if (e == hipSuccess) e = vsnap.alloc((size_t)V * instances);
    if (e == hipSuccess) e = big.alloc((size_t)(1 + F) * instances);
    if (e == hipSuccess) e = clipq.alloc((size_t)(1 + F) * instances);
    return e;
  }
};

}  // namespace se3tn
