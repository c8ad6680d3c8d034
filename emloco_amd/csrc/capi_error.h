// capi_error.h -- internal, host only: the one error channel of the C ABI.  Every *_capi.hip unit refuses through capi_fail, which
// keeps the text for emloco_last_error() (sim_capi.hip) and prints nothing.  The text is per thread (one instance per thread for the
// whole library: an inline variable) and describes the last call that failed on that thread.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "../../include/emloco_sim.h"      // EMLOCO_E_*

namespace emloco {

inline thread_local std::string capi_error;

// stores "text[: hip text]", returns `code`
inline int capi_fail(int code, const char *text, hipError_t e = hipSuccess) {
    std::string msg(text);
    if (e != hipSuccess) msg.append(": ").append(hipGetErrorString(e));
    capi_error.swap(msg);
    return code;
}

// stores "who: why[: hip text]"
inline int capi_fail(int code, const char *who, const char *why, hipError_t e = hipSuccess) {
    return capi_fail(code, (std::string(who) + ": " + why).c_str(), e);
}

}  // namespace emloco

// a failed HIP call ends the entry point (or the helper) it stands in, named in the text: "emloco_sim_prepare: hipMalloc(...): out of memory"
#define EMLOCO_HIPCHK(expr)                                                                             \
    do {                                                                                                \
        const hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return emloco::capi_fail(EMLOCO_E_HIP, __func__, #expr, e_);              \
    } while (0)
