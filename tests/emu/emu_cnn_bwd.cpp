// TEST INFRASTRUCTURE ONLY: the backward of the crowd policy's convolution trunk (emloco_amd/csrc/cnn_backward_kernels.hip) on the CPU with
// the launch shape of cnn_capi.hip, all arrays on the host.  Built into its own library by tests/emu_cnn_bwd.py together with
// emu_runtime.cpp.
#include "hip/hip_runtime.h"
#include "../../emloco_amd/csrc/cnn_backward_kernels.hip"

static const char *g_cnn_bwd_why = "";

extern "C" const char *emu_cnn_bwd_error(void) { return g_cnn_bwd_why; }

// the grid the C ABI takes for `rows` (tests take the row limit of one workgroup from the workspace query, this is for the emulator's own use)
extern "C" int emu_cnn_bwd_grid(int rows) { return emloco::cnn_bwd_grid(rows); }

// the argument list of emloco_cnn_trunk_backward with `grid` in the stream's place: 0 = the ABI's own choice, > 0 makes that many
// workgroups stride over the rows
extern "C" int emu_cnn_trunk_backward(int rows, int res, int channels, int layers, int f0, int f1, int f2, int f3, const float *x, int ldx,
                                      const float *mean, const float *var, float eps, float clip, int normalize, const float *params,
                                      const float *dout, int lddo, int dout_off, float *dparams, float *workspace, int64_t workspace_floats,
                                      int grid) {
    emloco::CnnTrunkBwd b = {};
    emloco::CnnTrunk &a = b.t;
    a.rows = rows, a.res = res, a.channels = channels, a.layers = layers;
    a.filters[0] = f0, a.filters[1] = f1, a.filters[2] = f2, a.filters[3] = f3;
    a.ldx = ldx, a.normalize = normalize ? 1 : 0;
    a.eps = eps, a.clip = clip;
    a.x = x, a.mean = mean, a.var = var, a.params = params;
    b.dout = dout, b.lddo = lddo, b.dout_off = dout_off, b.dparams = dparams, b.workspace = workspace, b.workspace_floats = workspace_floats;
    const char *why = emloco::cnn_bwd_refusal(b, true);
    g_cnn_bwd_why = why ? why : "";
    if (why) return -1;
    const int g = grid > 0 && grid < emloco::cnn_bwd_grid(rows) ? grid : emloco::cnn_bwd_grid(rows);      // (the workspace is sized by the ABI's)
    const int count = emloco::cnn_param_count(channels, layers, a.filters);
    emu::launch((unsigned)g, emloco::kCnnBwdThreads,
                [&] { emloco::cnn_trunk_backward_kernel(a, x, mean, var, params, dout, lddo, dout_off, workspace); });
    emu::launch((unsigned)((count + 255) / 256), 256, [&] { emloco::cnn_grad_reduce_kernel(workspace, g, count, dparams); });
    blockIdx.x = 0;
    return 0;
}
