// cnn_capi.hip -- C ABI (include/emloco_predictor.h) over the crowd policy's convolution trunk.
#include <hip/hip_runtime.h>
#include "cnn_kernels.hip"
#include "cnn_backward_kernels.hip"
#include "capi_error.h"

using emloco::capi_fail;

namespace {
constexpr int kCnnMaxGrid = 4096;
}  // namespace

extern "C" {

int emloco_cnn_trunk(int rows, int res, int channels, int layers, int f0, int f1, int f2, int f3, const float *x, int ldx,
                     const float *mean, const float *var, float eps, float clip, int normalize, const float *params, float *out, int ldo,
                     int out_off, void *stream) {
    emloco::CnnTrunk a;
    a.rows = rows, a.res = res, a.channels = channels, a.layers = layers;
    a.filters[0] = f0, a.filters[1] = f1, a.filters[2] = f2, a.filters[3] = f3;
    a.ldx = ldx, a.ldo = ldo, a.out_off = out_off, a.normalize = normalize ? 1 : 0;
    a.eps = eps, a.clip = clip;
    a.x = x, a.mean = mean, a.var = var, a.params = params, a.out = out;
    if (const char *why = emloco::cnn_refusal(a)) return capi_fail(EMLOCO_E_ARG, "emloco_cnn_trunk", why);
    hipLaunchKernelGGL(emloco::cnn_trunk_kernel, dim3((unsigned)(rows < kCnnMaxGrid ? rows : kCnnMaxGrid)), dim3(emloco::kCnnThreads), 0,
                       (hipStream_t)stream, a, x, mean, var, params, out);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int64_t emloco_cnn_trunk_backward_workspace(int rows, int res, int channels, int layers, int f0, int f1, int f2, int f3) {
    emloco::CnnTrunkBwd b = {};
    b.t.rows = rows, b.t.res = res, b.t.channels = channels, b.t.layers = layers;
    b.t.filters[0] = f0, b.t.filters[1] = f1, b.t.filters[2] = f2, b.t.filters[3] = f3;
    if (const char *why = emloco::cnn_bwd_refusal(b, false)) return capi_fail(EMLOCO_E_ARG, "emloco_cnn_trunk_backward_workspace", why);
    return (int64_t)emloco::cnn_bwd_grid(rows) * emloco::cnn_param_count(channels, layers, b.t.filters);
}

int emloco_cnn_trunk_backward(int rows, int res, int channels, int layers, int f0, int f1, int f2, int f3, const float *x, int ldx,
                              const float *mean, const float *var, float eps, float clip, int normalize, const float *params,
                              const float *dout, int lddo, int dout_off, float *dparams, float *workspace, int64_t workspace_floats,
                              void *stream) {
    emloco::CnnTrunkBwd b = {};
    emloco::CnnTrunk &a = b.t;
    a.rows = rows, a.res = res, a.channels = channels, a.layers = layers;
    a.filters[0] = f0, a.filters[1] = f1, a.filters[2] = f2, a.filters[3] = f3;
    a.ldx = ldx, a.normalize = normalize ? 1 : 0;
    a.eps = eps, a.clip = clip;
    a.x = x, a.mean = mean, a.var = var, a.params = params;
    b.dout = dout, b.lddo = lddo, b.dout_off = dout_off, b.dparams = dparams, b.workspace = workspace, b.workspace_floats = workspace_floats;
    if (const char *why = emloco::cnn_bwd_refusal(b, true)) return capi_fail(EMLOCO_E_ARG, "emloco_cnn_trunk_backward", why);
    const int grid = emloco::cnn_bwd_grid(rows), count = emloco::cnn_param_count(channels, layers, a.filters);
    hipLaunchKernelGGL(emloco::cnn_trunk_backward_kernel, dim3((unsigned)grid), dim3(emloco::kCnnBwdThreads), 0, (hipStream_t)stream, a, x,
                       mean, var, params, dout, lddo, dout_off, workspace);
    EMLOCO_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(emloco::cnn_grad_reduce_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, workspace,
                       grid, count, dparams);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
