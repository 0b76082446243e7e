// Thread-local error message + status helpers for the C-ABI.
#pragma once
#include <string>

#include "../../include/cfm.h"

namespace cfm {
cfm_status set_error(cfm_status s, const std::string& msg);
int calc_length(int T);
}  // namespace cfm

// a launcher's int result (0, or a hipError_t) -> the C-ABI status of the calling function (HIP translation units)
#define KCHK(x)                                                                               \
  do {                                                                                        \
    int _e = (x);                                                                             \
    if (_e) return set_error(CFM_ERR_RUNTIME, std::string(#x ": ") + hipGetErrorString((hipError_t)_e)); \
  } while (0)
