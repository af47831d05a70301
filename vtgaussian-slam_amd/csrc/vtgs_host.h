// vtgs_host.h -- how every entry point of libvtgs.so reports a failed HIP call: VTGS_ERR_HIP, with the message that
// vtgs_last_hip_error() returns (include/vtgs.h).  Host code only; included by every translation unit that has entry points.
#pragma once
#include "../../include/vtgs.h"

#include <hip/hip_runtime.h>
#include <stdio.h>

namespace vtgs {

inline thread_local char g_hip_err[256] = "";             // (C++17 inline variable: one per library and thread, not per file)

inline int hip_fail(hipError_t e, const char* what) {
  snprintf(g_hip_err, sizeof(g_hip_err), "%s: %s", what, hipGetErrorString(e));
  return VTGS_ERR_HIP;
}
#define VTGS_HIP(call)                                        \
  do {                                                        \
    hipError_t e__ = (call);                                  \
    if (e__ != hipSuccess) return hip_fail(e__, #call);       \
  } while (0)

// the last line of an entry point that launched kernels: `return launch_status(__func__);`
inline int launch_status(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VTGS_OK : hip_fail(e, what);
}

}  // namespace vtgs
