// TEST INFRASTRUCTURE ONLY: the crowd policy's convolution trunk (emloco_amd/csrc/cnn_kernels.hip) on the CPU with the launch shape of
// cnn_capi.hip, all arrays on the host.  Built into its own library by tests/emu_cnn.py together with emu_runtime.cpp.
#include "hip/hip_runtime.h"
#include "../../emloco_amd/csrc/cnn_kernels.hip"

static const char *g_cnn_why = "";

extern "C" const char *emu_cnn_error(void) { return g_cnn_why; }

// the argument list of emloco_cnn_trunk with `grid` in the stream's place: > 0 makes that many workgroups stride over the rows
extern "C" int emu_cnn_trunk(int rows, int res, int channels, int layers, int f0, int f1, int f2, int f3, const float *x, int ldx,
                             const float *mean, const float *var, float eps, float clip, int normalize, const float *params, float *out,
                             int ldo, int out_off, int grid) {
    emloco::CnnTrunk a;
    a.rows = rows, a.res = res, a.channels = channels, a.layers = layers;
    a.filters[0] = f0, a.filters[1] = f1, a.filters[2] = f2, a.filters[3] = f3;
    a.ldx = ldx, a.ldo = ldo, a.out_off = out_off, a.normalize = normalize ? 1 : 0;
    a.eps = eps, a.clip = clip;
    a.x = x, a.mean = mean, a.var = var, a.params = params, a.out = out;
    const char *why = emloco::cnn_refusal(a);
    g_cnn_why = why ? why : "";
    if (why) return -1;
    emu::launch((unsigned)(grid > 0 && grid < rows ? grid : rows), emloco::kCnnThreads,
                [&] { emloco::cnn_trunk_kernel(a, x, mean, var, params, out); });
    blockIdx.x = 0;
    return 0;
}
