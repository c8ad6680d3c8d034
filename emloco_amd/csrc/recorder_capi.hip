// recorder_capi.hip -- C ABI (include/emloco_task.h) over the flight recorder's kernels.
#include <hip/hip_runtime.h>
#include "recorder_kernels.hip"
#include "capi_error.h"

using emloco::capi_fail;

namespace {
constexpr int kRecMaxGrid = 1024;

// the refusal both entry points share: the text names the argument, or NULL when the structure is complete
const char *recorder_refusal(const EmlocoRecorderBufs *r, int t) {
    if (!r) return "null structure";
    if (r->n_env <= 0) return "n_env <= 0";
    if (r->depth < 1) return "depth < 1";
    if (r->n_slots < 1) return "n_slots < 1";
    if (r->t0 < 0 || t < r->t0) return "t before t0 (or t0 negative)";
    if (r->grid < 0) return "negative grid";
    if (r->drive_mode < 0 || r->drive_mode > 1) return "drive_mode 0 | 1 required";
    if (!(r->speed2_limit >= 0.0f)) return "speed2_limit negative or NaN";
    if (!(r->ang_speed2_limit >= 0.0f)) return "ang_speed2_limit negative or NaN";
    if (!r->root_state) return "null root_state";
    if (!r->dof_state) return "null dof_state";
    if (!r->warm_start) return "null warm_start";
    if (!r->drive) return "null drive";
    if (!r->rb_state) return "null rb_state";
    if (!r->contact_force) return "null contact_force";
    if (!r->dof_force) return "null dof_force";
    if (!r->progress_buf) return "null progress_buf";
    if (!r->reset_buf) return "null reset_buf";
    if (!r->terminate_buf) return "null terminate_buf";
    if (!r->ring) return "null ring";
    if (!r->slots) return "null slots";
    if (!r->counters) return "null counters";
    if (!r->last_capture_step) return "null last_capture_step";
    if (!r->cause_ws) return "null cause_ws";
    if (((uintptr_t)r->ring | (uintptr_t)r->slots) & 15u) return "ring / slots not 16-byte aligned";
    return nullptr;
}

unsigned recorder_grid(const EmlocoRecorderBufs *r, int jobs) {
    const int g = r->grid > 0 ? r->grid : jobs;
    return (unsigned)(g < kRecMaxGrid ? g : kRecMaxGrid);
}
}  // namespace

extern "C" {

int emloco_recorder_record(const EmlocoRecorderBufs *r, int t, void *stream) {
    const char *who = "emloco_recorder_record";
    if (const char *why = recorder_refusal(r, t)) return capi_fail(EMLOCO_E_ARG, who, why);
    hipLaunchKernelGGL(emloco::recorder_record_kernel, dim3(recorder_grid(r, r->n_env)), dim3(emloco::kRecThreads), 0, (hipStream_t)stream, *r, t);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_recorder_check(const EmlocoRecorderBufs *r, int t, void *stream) {
    const char *who = "emloco_recorder_check";
    if (const char *why = recorder_refusal(r, t)) return capi_fail(EMLOCO_E_ARG, who, why);
    hipStream_t st = (hipStream_t)stream;
    const int cause_jobs = (r->n_env + emloco::kRecCauseWaves - 1) / emloco::kRecCauseWaves;
    hipLaunchKernelGGL(emloco::recorder_cause_kernel, dim3(recorder_grid(r, cause_jobs)), dim3(64 * emloco::kRecCauseWaves), 0, st, *r, t);
    EMLOCO_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(emloco::recorder_claim_kernel, dim3(1), dim3(emloco::kRecClaimThreads), 0, st, *r, t);
    EMLOCO_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(emloco::recorder_copy_kernel, dim3(recorder_grid(r, r->n_slots)), dim3(emloco::kRecCopyThreads), 0, st, *r, t);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
