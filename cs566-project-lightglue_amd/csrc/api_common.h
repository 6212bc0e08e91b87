// What every C-ABI translation unit of this library shares: error reporting through
// lg_last_error(), the HIP-call check, and the <family>_weight_count/name/numel accessors.
#pragma once

#include <string>

#include "../../include/lightglue_mi355x.h"
#include "weight_schema.h"

namespace lg {
// stores the message lg_last_error() returns on this thread (lightglue_api.cpp); returns code
int api_fail(int code, const char* msg);

inline int weight_count(const WeightSchema& s) { return s.size(); }
inline const char* weight_name(const WeightSchema& s, int i) {
  return (i >= 0 && i < s.size()) ? s.name(i).c_str() : nullptr;
}
inline int64_t weight_numel(const WeightSchema& s, int i) { return (i >= 0 && i < s.size()) ? s.numel(i) : -1; }
}  // namespace lg

inline int fail(int code, const std::string& msg) { return lg::api_fail(code, msg.c_str()); }

#define LG_HIP(expr)                                                                                \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess) return fail(LG_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)
