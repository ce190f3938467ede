// host_prologue.hpp -- what the entry points of the handle-free and handle-owning units (k_lmfit.hip, k_tmatch.hip, k_contfit.hip,
// mlp_api.hip) do before they launch: select the device for a scope, leave a message for payne_last_error(NULL), check a pointer
// for 16-byte loads.  Internal: not installed, no new export.  (payne_hip.hip's DeviceScope also synchronises and ctx_on_device is
// sticky by contract: neither is this.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

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

}  // namespace host
}  // namespace payne
