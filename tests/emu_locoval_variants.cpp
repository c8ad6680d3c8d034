// TEST INFRASTRUCTURE ONLY: runs the LocoVal kernels of emloco_amd/csrc/predictor_kernels.hip + locoval_variants.h on the CPU through
// tests/emu/hip/ (tests/test_locoval_variants_cpu.py compiles it with emu/emu_runtime.cpp).  The variant entry points go through the
// product's own dispatch (emloco::locoval_variant_fwd / _bwd) with a launcher that runs the kernel on the emulator; the emu_locoval_old_*
// entry points launch the full network's kernels as emloco_locoval_fwd_rows / _bwd / _bwd_rows do (predictor_capi.hip).
#include <stdint.h>
#include "hip/hip_runtime.h"
#include "../emloco_amd/csrc/predictor_kernels.hip"

using namespace emloco;

namespace {
struct EmuLaunch {
    template <class K, class... A> void operator()(K kernel, unsigned grid, unsigned block, A... args) const {
        emu::launch(grid, block, [&] { kernel(args...); });
        blockIdx.x = 0;
    }
};
}  // namespace

extern "C" int emu_locoval_variant_dims(int variant, int32_t *dims4) {
    LocoValDims d;
    if (!locoval_dims(variant, &d)) return -1;
    dims4[0] = d.in; dims4[1] = d.h1; dims4[2] = d.h2; dims4[3] = d.n_param;
    return 0;
}

extern "C" int emu_locoval_variant_fwd_rows(int variant, int B, const float *traj, int ts, const float *pose, const float *vel, const float *w1,
                                            const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, float *value,
                                            float *x, float *h1, float *h2, float *angle, float *pose_rot, const float *row_weight) {
    const LocoValFwd a{B, traj, ts, pose, vel, w1, b1, w2, b2, w3, b3, value, x, h1, h2, angle, pose_rot, row_weight};
    locoval_variant_fwd(EmuLaunch{}, variant, a);
    return 0;
}

// slot / count NULL: the dense backward (emloco_locoval_variant_bwd)
extern "C" int emu_locoval_variant_bwd_rows(int variant, int B, const float *traj, int ts, const float *pose, const float *vel, const float *w1,
                                            const float *w2, const float *w3, const float *value, const float *x, const float *h1,
                                            const float *h2, const float *angle, const float *dvalue, const int32_t *slot, const float *count,
                                            float *dparams, float *dtraj, float *ws) {
    const LocoValBwd a{B, traj, ts, pose, vel, w1, w2, w3, value, x, h1, h2, angle, dvalue, ws, dparams, dtraj, slot, count};
    locoval_variant_bwd(EmuLaunch{}, variant, a);
    return 0;
}

extern "C" int emu_locoval_old_fwd_rows(int B, const float *traj, int ts, const float *pose, const float *vel, const float *w1, const float *b1,
                                        const float *w2, const float *b2, const float *w3, const float *b3, float *value, float *x100, float *h1,
                                        float *h2, float *angle, const float *row_weight) {
    emu::launch((unsigned)B, 64, [&] { locoval_fwd_kernel(B, traj, ts, pose, vel, w1, b1, w2, b2, w3, b3, value, x100, h1, h2, angle, row_weight); });
    blockIdx.x = 0;
    return 0;
}

extern "C" int emu_locoval_old_bwd_rows(int B, const float *traj, int ts, const float *pose, const float *vel, const float *w1, const float *w2,
                                        const float *w3, const float *value, const float *x100, const float *h1, const float *h2,
                                        const float *angle, const float *dvalue, const int32_t *slot, const float *count, float *dparams,
                                        float *dtraj, float *ws) {
    emu::launch((unsigned)B, 64, [&] { locoval_bwd_kernel(B, traj, ts, pose, vel, w1, w2, w3, value, x100, h1, h2, angle, dvalue, ws, dtraj, slot); });
    emu::launch((unsigned)((LV_NPARAM + 255) / 256), 256, [&] { locoval_reduce_kernel(B, ws, dparams, count); });
    blockIdx.x = 0;
    return 0;
}

extern "C" int emu_locoval_fit_grad_rows(int n, const float *value, const float *target, const float *weight, float *dvalue, float *tail,
                                         int32_t *slot) {
    emu::launch(1, 1024, [&] { locoval_fit_grad_kernel(n, value, target, weight, dvalue, tail, slot); });
    return 0;
}
