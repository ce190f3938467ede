// host_prologue.hpp -- what the entry points of the handle-free and handle-owning units (k_lmfit.hip, k_tmatch.hip, k_contfit.hip,
// mlp_api.hip, k_sedfit.hip) do before they launch: select the device for a scope, leave a message for payne_last_error(NULL), check
// a pointer for 16-byte loads; and what a handle's create and destroy do: keep its device allocations in a bag and free them.
// Internal: not installed, no new export.  (payne_hip.hip's DeviceScope also synchronises and ctx_on_device is sticky by
// contract: neither is this.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "ctx_api.hpp"

namespace payne {
namespace host {

// the create string = msg; returns `code`
PAYNE_LOCAL inline int fail(int code, const std::string& msg) {
  set_create_error(msg);
  return code;
}

// Selects `device` for its scope and puts the caller's device back on the way out.
class PAYNE_LOCAL OnDevice {
 public:
  explicit OnDevice(int device) {
    (void)hipGetDevice(&prev_);
    ok_ = hipSetDevice(device) == hipSuccess;
  }
  ~OnDevice() { (void)hipSetDevice(prev_); }
  OnDevice(const OnDevice&) = delete;
  OnDevice& operator=(const OnDevice&) = delete;
  bool ok() const { return ok_; }

 private:
  int prev_ = 0;
  bool ok_ = false;
};

PAYNE_LOCAL inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The device allocations of a handle, made on the selected device; after the first failure `ok` is false and nothing more is tried.
struct PAYNE_LOCAL DeviceBag {
  std::vector<void*> owned;
  bool ok = true;

  void* alloc(size_t bytes) {
    void* p = nullptr;
    if (!ok || hipMalloc(&p, bytes) != hipSuccess) {
      ok = false;
      return nullptr;
    }
    owned.push_back(p);
    return p;
  }
  void* zeros(size_t bytes) {
    void* p = alloc(bytes);
    if (p && hipMemset(p, 0, bytes) != hipSuccess) ok = false;
    return p;
  }
  void* upload(const void* src, size_t bytes) {
    void* p = alloc(bytes);
    put(p, src, bytes);
    return p;
  }
  void put(void* dst, const void* src, size_t bytes) {
    if (ok && hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess) ok = false;
  }
  template <class V>
  const V* upload(const std::vector<V>& v) { return static_cast<const V*>(upload(v.data(), v.size() * sizeof(V))); }
  float* floats(size_t n) { return static_cast<float*>(zeros(n * sizeof(float))); }
  void put_floats(float* dst, const float* src, size_t n) { put(dst, src, n * sizeof(float)); }
};

// Frees a handle's allocations on its device, behind the device's pending work where `synchronise` says so, and the handle.
template <class Handle>
PAYNE_LOCAL inline void destroy(Handle* h, bool synchronise) {
  if (!h) return;
  {
    OnDevice on(h->device);
    if (on.ok()) {
      if (synchronise) (void)hipDeviceSynchronize();
      for (void* p : h->bag.owned) (void)hipFree(p);
    }
  }
  delete h;
}

}  // namespace host
}  // namespace payne
