// crowd_capi.hip -- C ABI (include/emloco_task.h) over the crowd-aware terrain sensor's kernels.
#include <hip/hip_runtime.h>
#include "crowd_kernels.hip"
#include "capi_error.h"

using emloco::capi_fail;

namespace {
constexpr int kCrowdMaxGrid = 4096;
unsigned crowd_grid(int jobs) { return (unsigned)(jobs < kCrowdMaxGrid ? jobs : kCrowdMaxGrid); }
}  // namespace

extern "C" {

int emloco_task_crowd_sensor(const EmlocoCrowdBufs *bufs, const int32_t *dev_env_ids, int n, void *stream) {
    const char *who = "emloco_task_crowd_sensor";
    if (const char *why = emloco::crowd_refusal(bufs, n)) return capi_fail(EMLOCO_E_ARG, who, why);
    hipStream_t st = (hipStream_t)stream;
    const int rows = dev_env_ids ? n : bufs->n_env;
    if (rows == 0) return 0;
    if (bufs->stamps) {
        hipLaunchKernelGGL(emloco::crowd_stamp_kernel, dim3(crowd_grid(bufs->n_env)), dim3(emloco::kCrowdThreads), 0, st, *bufs);
        EMLOCO_HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(emloco::crowd_gather_kernel, dim3(crowd_grid(rows)), dim3(emloco::kCrowdThreads), 0, st, *bufs, dev_env_ids, rows);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
