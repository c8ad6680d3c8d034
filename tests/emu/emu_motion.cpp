// TEST INFRASTRUCTURE ONLY: motion_build_kernel on the CPU with the arguments of emloco_motion_build (include/emloco_task.h), all
// arrays on the host; validation and packing are the product's own (emloco::motion_pack), the launch is the emulator's.  Built into
// its own library by tests/emu_motion.py together with emu_runtime.cpp.
#include "hip/hip_runtime.h"
#include "../../emloco_amd/csrc/motion_kernels.hip"

static const char *g_motion_why = "";

extern "C" const char *emu_motion_build_error(void) { return g_motion_why; }

extern "C" int emu_motion_build(int n_clips, int n_skel, int64_t n_frames_total, const float *quat_global, const float *root_trans,
                                const int64_t *frame_start, const int32_t *n_frames, const float *fps, const int32_t *skel_id,
                                const float *local_translation, const int32_t *parent, const float *taps, float *gts, float *grs,
                                float *lrs, float *gvs, float *gavs, float *dvs, int grid) {
    g_motion_why = "";
    if (!quat_global || !root_trans || !frame_start || !n_frames || !fps || !skel_id || !local_translation || !gts || !grs || !lrs ||
        !gvs || !gavs || !dvs) { g_motion_why = "null array"; return -1; }
    if (grid < 0) { g_motion_why = "negative grid"; return -1; }
    emloco::MotionArgs a;
    const char *why = emloco::motion_pack(n_clips, n_skel, (long long)n_frames_total, (const long long *)frame_start, n_frames, skel_id,
                                          parent, taps, &a);
    if (why) { g_motion_why = why; return -1; }
    const unsigned g = grid > 0 ? (unsigned)grid : emloco::motion_default_grid(a);
    emu::launch(g, emloco::MOTION_THREADS, [&] {
        emloco::motion_build_kernel(a, quat_global, root_trans, (const long long *)frame_start, n_frames, fps, skel_id, local_translation,
                                    gts, grs, lrs, gvs, gavs, dvs);
    });
    blockIdx.x = 0;
    return 0;
}
