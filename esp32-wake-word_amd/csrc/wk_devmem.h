// wk_devmem.h -- owners of device memory and of pinned, mapped host memory
// (internal).  A handle struct holds these instead of raw pointers, so its
// destructor is the one list of what to free: `delete` the handle with its
// device current (inside on_device) and after whatever may still use the
// memory has been waited for.  Errors stay hipError_t; each entry point maps
// them to wk_status by its own rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <memory>
#include <vector>

namespace wk {

// A hipMalloc block.  Move-only; freed on reset() and on destruction.
class DevMem {
 public:
  hipError_t alloc_bytes(size_t bytes) {
    void* p = nullptr;
    p_.reset();
    const hipError_t e = hipMalloc(&p, bytes);
    p_.reset(p);
    return e;
  }
  void reset() { p_.reset(); }

 protected:
  struct Free {
    void operator()(void* p) const { (void)hipFree(p); }
  };
  std::unique_ptr<void, Free> p_;
};

// ... of n elements of T; reads as the T* wherever one is expected.
template <typename T>
class DevBuf : public DevMem {
 public:
  hipError_t alloc(size_t n) { return alloc_bytes(sizeof(T) * n); }
  // Allocate, then copy host to device.  An empty table still gets one element, so it has an address.
  hipError_t upload(const T* host, size_t n) {
    const hipError_t e = alloc(n ? n : 1);
    if (e != hipSuccess || n == 0) return e;
    return hipMemcpy(get(), host, sizeof(T) * n, hipMemcpyHostToDevice);
  }
  hipError_t upload(const std::vector<T>& host) { return upload(host.data(), host.size()); }
  T* get() const { return static_cast<T*>(p_.get()); }
  operator T*() const { return get(); }
};

// A pinned, mapped, coherent host block with its device alias: the host writes
// or reads host(), kernels dev().  Move-only.
template <typename T>
class PinnedBuf {
 public:
  // *failed_call (when given) names the runtime call that returned the error.
  hipError_t alloc(size_t n, const char** failed_call = nullptr) {
    T* p = nullptr;
    h_.reset();
    const char* call = "hipHostMalloc";
    hipError_t e = hipHostMalloc(&p, sizeof(T) * n, hipHostMallocMapped | hipHostMallocCoherent);
    h_.reset(p);
    if (e == hipSuccess) {
      call = "hipHostGetDevicePointer";
      e = hipHostGetDevicePointer((void**)&d_, p, 0);
    }
    if (e != hipSuccess && failed_call) *failed_call = call;
    return e;
  }
  T* host() const { return h_.get(); }
  T* dev() const { return h_ ? d_ : nullptr; }   // (null again once moved from)

 private:
  struct Free {
    void operator()(T* p) const { (void)hipHostFree(p); }
  };
  std::unique_ptr<T, Free> h_;
  T* d_ = nullptr;
};

}  // namespace wk
