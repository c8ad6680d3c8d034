// locoval_multi.h -- several LocoVal networks on the same rows in one launch: the forward of the evaluation that compares networks on
// the same games (`run.py --test --compare_valuenet`, include/emloco_predictor.h: emloco_locoval_eval_fwd_multi).
//
// One wave per row, as the full and the pose kernels; rows whose mask is 0 leave at once and keep their values.  The staged inputs are
// read and yaw-normalised ONCE (locoval_input: the full network's 100-vector, of which every variant's input is a part -- [0, 26) the
// trajectory, [26, 98) the pose, [98, 100) the velocity), then the networks of the table run one after another on that vector in LDS
// through the pieces the single-network forwards are made of (locoval_unit, locoval_head, row_sum / wave_sum), in their order of
// operations: network k's value is bit for bit what emloco_locoval_variant_fwd_rows writes for it alone.  That is also why this kernel
// is compiled here, in the predictor's unit beside those forwards, and not in the evaluation's (eval_kernels.hip is built without
// multiply-add contraction, the forwards with it).  The narrow variants sum their output layer over the 16-lane row, as their kernel
// does; nothing is written but the value planes -- the inputs are const, no network sees what another one left.
#pragma once

namespace emloco {

template <int IN, int H1, int H2, bool ROW16>
__device__ __forceinline__ void locoval_multi_net(int lane, int i, const EmlocoLocoValNet &n, const float *x, float *h1, float *h2) {
    if (lane < H1) h1[lane] = locoval_unit<IN>(n.b1[lane], n.w1 + lane * IN, 1, x);
    __syncthreads();
    if (lane < H2) h2[lane] = locoval_unit<H1>(n.b2[lane], n.w2 + lane * H1, 1, h1);
    __syncthreads();
    float p = lane < H2 ? n.w3[lane] * h2[lane] : 0.0f;
    p = ROW16 ? row_sum(p) : wave_sum(p);
    if (lane == 0) n.value[i] = locoval_head(p, n.b3[0]);
}

__global__ void __launch_bounds__(64)
locoval_eval_fwd_multi_kernel(int B, const float *traj13, const float *pose, const float *vel, const float *row_mask, EmlocoLocoValNets t) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= B || row_mask[i] == 0.0f) return;
    __shared__ float x[LV_IN], xv[28], h1[LV_H1], h2[LV_H2];
    locoval_input(lane, traj13 + (long)i * 39, 3, pose + (long)i * 72, vel + (long)i * 2, x, nullptr);
    __syncthreads();
    if (lane < 28) xv[lane] = x[lane < 26 ? lane : lane + 72];        // the velocity-only input [traj 26 | vel 2]
    __syncthreads();
    for (int k = 0; k < t.n_nets; ++k) {
        const EmlocoLocoValNet &n = t.net[k];
        switch (n.variant) {
        case EMLOCO_LOCOVAL_FULL: locoval_multi_net<LV_IN, LV_H1, LV_H2, false>(lane, i, n, x, h1, h2); break;
        case EMLOCO_LOCOVAL_POSE: locoval_multi_net<LVP_IN, LVP_H1, LVP_H2, false>(lane, i, n, x, h1, h2); break;
        case EMLOCO_LOCOVAL_VEL: locoval_multi_net<LocoValRow<1>::IN, LocoValRow<1>::H1, LocoValRow<1>::H2, true>(lane, i, n, xv, h1, h2); break;
        default: locoval_multi_net<LocoValRow<0>::IN, LocoValRow<0>::H1, LocoValRow<0>::H2, true>(lane, i, n, xv, h1, h2); break;
        }
        __syncthreads();            // the next network writes h1 / h2
    }
}

}  // namespace emloco
