// hip_rc.h -- the C ABI's return code for a HIP error (include/smap_hip.h: 0 = success, -(1000 + hipError_t) otherwise); host side, internal.
#pragma once
#include <hip/hip_runtime.h>

static inline int hip_rc(hipError_t e) { return e == hipSuccess ? 0 : -(1000 + (int)e); }
