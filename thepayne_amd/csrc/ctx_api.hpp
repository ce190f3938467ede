// ctx_api.hpp -- what another unit of libpayne_hip.so may ask of a context.  `struct payne_ctx` is private to payne_hip.hip, which
// defines everything declared here; the other units (sampler_api.hip, mlp_api.hip) come through these functions.  Internal: not
// installed, no new export.
#pragma once
#include <string>

#include "../../include/payne_hip.h"

#define PAYNE_LOCAL __attribute__((visibility("hidden")))   // linked between the library's units, not exported from it

struct WalkTail;    // sampler_core.hpp
struct WalkState;

namespace payne {

// the message payne_last_error(NULL) returns: set by every entry point that fails before it has a context
void set_create_error(const std::string& msg);

// c->err = msg (no context: the create string); returns `code`
PAYNE_LOCAL int ctx_fail(payne_ctx* c, int code, const std::string& msg);

// The calls of an entry point go to the context's device.  Sticky: the caller's device is NOT put back.
PAYNE_LOCAL int ctx_on_device(payne_ctx* c);

struct CtxView { int device, ncols, b_max; };
PAYNE_LOCAL CtxView ctx_view(const payne_ctx* c);

// A walk's next step asked of the likelihood batch's post kernel (its tail).  dev: the walk as the kernel reads it; done: set when
// the launch took it; spec: the walk (host copy) when proposals can be made ahead.
struct TailReq { const WalkTail* dev; int step, propose; bool done; const WalkState* spec; };

// payne_lnlike_batch, with the tail of a walk (null: none)
PAYNE_LOCAL int ctx_lnlike(payne_ctx* c, const double* theta, int B, double* lnl, void* stream, TailReq* tail);

}  // namespace payne
