// motion_capi.hip -- C ABI (include/emloco_task.h) over the motion library's clip build.
#include <hip/hip_runtime.h>
#include "motion_kernels.hip"
#include "../../include/emloco_task.h"
#include "capi_error.h"

using emloco::capi_fail;

extern "C" int emloco_motion_build(int n_clips, int n_skel, int64_t n_frames_total, const float *dev_quat_global,
                                   const float *dev_root_trans, const int64_t *dev_frame_start, const int32_t *dev_n_frames,
                                   const float *dev_fps, const int32_t *dev_skel_id, const int64_t *host_frame_start,
                                   const int32_t *host_n_frames, const int32_t *host_skel_id, const float *dev_local_translation,
                                   const int32_t *host_parent, const float *host_taps, float *dev_gts, float *dev_grs, float *dev_lrs,
                                   float *dev_gvs, float *dev_gavs, float *dev_dvs, int grid, void *stream) {
    static_assert(EMLOCO_MOTION_TAPS == emloco::MOTION_TAPS && EMLOCO_MOTION_BODIES == emloco::MOTION_NB,
                  "include/emloco_task.h and motion_kernels.hip disagree");
    static_assert(sizeof(long long) == sizeof(int64_t), "frame_start is read as 64-bit");
    if (!dev_quat_global || !dev_root_trans || !dev_frame_start || !dev_n_frames || !dev_fps || !dev_skel_id || !dev_local_translation ||
        !dev_gts || !dev_grs || !dev_lrs || !dev_gvs || !dev_gavs || !dev_dvs)
        return capi_fail(EMLOCO_E_ARG, "emloco_motion_build", "null device array");
    if (grid < 0) return capi_fail(EMLOCO_E_ARG, "emloco_motion_build", "negative grid");
    emloco::MotionArgs a;
    const char *why = emloco::motion_pack(n_clips, n_skel, (long long)n_frames_total, (const long long *)host_frame_start, host_n_frames,
                                          host_skel_id, host_parent, host_taps, &a);
    if (why) return capi_fail(EMLOCO_E_ARG, "emloco_motion_build", why);
    const unsigned g = grid > 0 ? (unsigned)grid : emloco::motion_default_grid(a);
    hipLaunchKernelGGL(emloco::motion_build_kernel, dim3(g), dim3(emloco::MOTION_THREADS), 0, (hipStream_t)stream, a, dev_quat_global,
                       dev_root_trans, (const long long *)dev_frame_start, dev_n_frames, dev_fps, dev_skel_id, dev_local_translation,
                       dev_gts, dev_grs, dev_lrs, dev_gvs, dev_gavs, dev_dvs);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}
