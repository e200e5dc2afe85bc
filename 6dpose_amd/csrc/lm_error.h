// The error plumbing every host unit shares (not part of the C ABI): lm_set_error (detector.cpp) records the message that
// lm_last_error returns, HIP_TRY returns it from the enclosing function when a HIP call fails.  lm_open_device (detector.cpp) is how a
// context's create selects its device: LM_ERR_NO_DEVICE without one, LM_ERR_INVALID for an index out of range, else hipSetDevice.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/amd_linemod.h"

int lm_set_error(int code, const char* fmt, ...);
int lm_open_device(int device);

#define HIP_TRY(expr)                                                                                         \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess) return lm_set_error(LM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                                  __FILE__, __LINE__);                                        \
    } while (0)
