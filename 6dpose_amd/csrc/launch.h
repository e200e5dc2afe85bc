// The one way a kernel is launched (DESIGN.md "Kernel launches"): only .hip units include this header, every launch_* function they
// define returns [[nodiscard]] hipError_t, and every host caller checks it (HIP_TRY names the launcher in its message).
#pragma once
#include <hip/hip_runtime.h>

namespace lm {

template <typename T>
struct launch_param { using type = T; };      // (keeps the arguments out of template deduction: the kernel alone decides the parameter types)

// kernel<<<grid, block, lds, s>>>(p...) with the launch's own status as the result.  The arguments bind to the kernel's parameter types as
// in a call — an int for a uint32_t or a double for a float is converted into a temporary that lives until the launch returns, an object
// of the parameter's own type (the by-value structs: FeStage is 4 KB) is taken where it is, uncopied — and hipLaunchKernel, which copies
// them into the kernel's argument buffer, is the only runtime call made.  hipGetLastError() after a launch would instead report the
// thread's last error of ANY call, e.g. the hipErrorNotReady of an event query.
template <typename... P>
[[nodiscard]] inline hipError_t lm_launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, const typename launch_param<P>::type&... p) {
    void* ptrs[sizeof...(P) + 1] = {const_cast<void*>(static_cast<const void*>(&p))..., nullptr};
    return hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, ptrs, lds, s);
}

}  // namespace lm

// Inside a launcher with several launches: the first failure is returned and nothing is launched after it.
#define LAUNCH_TRY(expr)                        \
    do {                                        \
        const hipError_t e_ = (expr);           \
        if (e_ != hipSuccess) return e_;        \
    } while (0)
