// api_error.hpp -- the message payne_last_error(NULL) returns: the one string of payne_hip.hip, set by every entry point that
// fails before it has a context (payne_ctx_create and the create calls of mlp_api.hip).
#pragma once
#include <string>

namespace payne {

void set_create_error(const std::string& msg);

}  // namespace payne
