// locoval_variants.h -- the reduced-input LocoVal networks (value_pose_net.py:22-50: use_pose / use_vel) beside the full one.
//
// variant = (use_pose << 1) | use_vel (EMLOCO_LOCOVAL_* of include/emloco_predictor.h); sizes as value_pose_net.py:43-52:
//     3 full   100 / 49 / 24   locoval_fwd_kernel / locoval_bwd_kernel / locoval_reduce_kernel (predictor_kernels.hip), untouched
//     2 pose    98 / 48 / 24   one wave per sample like the full kernels, without the velocity rows
//     1 vel     28 / 13 /  6   FOUR samples per wave, one per 16-lane DPP row (h1 <= 13 and the 13 waypoints fit a row):
//     0 traj    26 / 12 /  6   a 256-thread workgroup serves 16 samples and holds the ~1.8 KB of weights in LDS once
// Included at the end of predictor_kernels.hip; the dispatch (`locoval_variant_fwd / _bwd`) is shared by the C ABI
// (predictor_capi.hip) and the CPU emulation's glue (tests/emu/emu_predictor.cpp) through a launcher object, as fold_rows is.
#pragma once

namespace emloco {

struct LocoValDims { int in, h1, h2, n_param; };
inline bool locoval_dims(int variant, LocoValDims *d) {
    if (variant < 0 || variant > 3) return false;
    d->in = 26 + ((variant & 2) ? 72 : 0) + ((variant & 1) ? 2 : 0);
    d->h1 = d->in / 2 - 1;                      // value_pose_net.py:51
    d->h2 = d->h1 / 2;                          // :52
    d->n_param = d->h1 * d->in + d->h1 + d->h2 * d->h1 + d->h2 + d->h2 + 1;
    return true;
}

struct LocoValFwd {
    int B;
    const float *traj; int ts;
    const float *pose, *vel, *w1, *b1, *w2, *b2, *w3, *b3;
    float *value, *x, *h1, *h2, *angle /* or NULL */, *pose_rot /* or NULL; variants without the pose only */;
    const float *row_weight /* or NULL: every row */;
};
struct LocoValBwd {
    int B;
    const float *traj; int ts;
    const float *pose, *vel, *w1, *w2, *w3, *value, *x, *h1, *h2, *angle, *dvalue;
    float *ws, *dparams, *dtraj;
    const int32_t *slot /* or NULL: dense */;
    const float *count /* with slot: the number of slots in use */;
};

// (the yaw itself, locoval_yaw, stands with the other shared pieces of the forwards in predictor_kernels.hip)
// d angle / d waypoint 1 times dth, added to that waypoint's gradient (ox, oy); the guarded x carries no gradient
__device__ __forceinline__ void locoval_yaw_bwd(const float *traj, int ts, float dth, float &ox, float &oy) {
    float xv = traj[ts], yv = traj[ts + 1];
    const bool guarded = fabsf(xv) < 1e-10f;
    if (guarded) xv = 1e-10f;
    const float r2 = xv * xv + yv * yv;
    if (!guarded) ox += dth * (-yv / r2);
    oy += dth * (xv / r2);
}

// ------------------------------------------------------------------ pose variant 98 / 48 / 24 (one wave per sample)
#define LVP_IN 98
#define LVP_H1 48
#define LVP_H2 24
#define LVP_NPARAM (LVP_H1 * LVP_IN + LVP_H1 + LVP_H2 * LVP_H1 + LVP_H2 + LVP_H2 + 1)

// value_pose_net.py:73-103 + :116-127 forward_pose
__global__ void __launch_bounds__(64)
locoval_pose_fwd_kernel(LocoValFwd a) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= a.B) return;
    if (a.row_weight && a.row_weight[i] == 0.0f) return;
    __shared__ float x[LVP_IN], h1[LVP_H1], h2[LVP_H2];
    const float *tr = a.traj + (long)i * 13 * a.ts, *po = a.pose + (long)i * 72;
    const float ang = locoval_yaw(tr, a.ts);
    const float c = cosf(ang), s = sinf(ang);
    if (lane == 0 && a.angle) a.angle[i] = ang;
    if (lane < 13) locoval_norm_traj(lane, tr, a.ts, c, s, x);
    if (lane < 24) locoval_norm_pose(lane, po, c, s, x + 26);
    __syncthreads();
    for (int k = lane; k < LVP_IN; k += 64) a.x[(long)i * LVP_IN + k] = x[k];
    if (lane < LVP_H1) {
        const float acc = locoval_unit<LVP_IN>(a.b1[lane], a.w1 + lane * LVP_IN, 1, x);
        h1[lane] = acc; a.h1[(long)i * LVP_H1 + lane] = acc;
    }
    __syncthreads();
    if (lane < LVP_H2) {
        const float acc = locoval_unit<LVP_H1>(a.b2[lane], a.w2 + lane * LVP_H1, 1, h1);
        h2[lane] = acc; a.h2[(long)i * LVP_H2 + lane] = acc;
    }
    __syncthreads();
    float p = lane < LVP_H2 ? a.w3[lane] * h2[lane] : 0.0f;
    p = wave_sum(p);
    if (lane == 0) a.value[i] = locoval_head(p, a.b3[0]);
}

// this sample's parameter-gradient share to ws[row][5953] and d traj (locoval_bwd_kernel without the velocity terms)
__global__ void __launch_bounds__(64)
locoval_pose_bwd_kernel(LocoValBwd a) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= a.B) return;
    const int row = a.slot ? a.slot[i] : i;
    if (row < 0) return;
    __shared__ float x[LVP_IN], d1[LVP_H1], d2[LVP_H2], dx[LVP_IN];
    for (int k = lane; k < LVP_IN; k += 64) x[k] = a.x[(long)i * LVP_IN + k];
    const float v = a.value[i];
    const float dz3 = a.dvalue[i] * v * (1.0f - v);
    float *g = a.ws + (long)row * LVP_NPARAM;
    float *gw1 = g, *gb1 = g + LVP_H1 * LVP_IN, *gw2 = gb1 + LVP_H1, *gb2 = gw2 + LVP_H2 * LVP_H1, *gw3 = gb2 + LVP_H2, *gb3 = gw3 + LVP_H2;
    if (lane < LVP_H2) {
        const float hv = a.h2[(long)i * LVP_H2 + lane];
        gw3[lane] = dz3 * hv;
        const float dd = hv > 0.0f ? dz3 * a.w3[lane] : 0.0f;
        d2[lane] = dd; gb2[lane] = dd;
    }
    if (lane == 0) gb3[0] = dz3;
    __syncthreads();
    if (lane < LVP_H1) {
        const float hv = a.h1[(long)i * LVP_H1 + lane];
        float acc = 0.0f;
        for (int j = 0; j < LVP_H2; ++j) acc += a.w2[j * LVP_H1 + lane] * d2[j];
        const float dd = hv > 0.0f ? acc : 0.0f;
        d1[lane] = dd; gb1[lane] = dd;
        for (int j = 0; j < LVP_H2; ++j) gw2[j * LVP_H1 + lane] = d2[j] * hv;
    }
    __syncthreads();
    for (int e = lane; e < LVP_H1 * LVP_IN; e += 64) { const int j = e / LVP_IN, k = e - j * LVP_IN; gw1[e] = d1[j] * x[k]; }
    for (int k = lane; k < LVP_IN; k += 64) {
        float acc = 0.0f;
        for (int j = 0; j < LVP_H1; ++j) acc += a.w1[j * LVP_IN + k] * d1[j];
        dx[k] = acc;
    }
    __syncthreads();
    // back through the yaw normalisation to the trajectory (the pose carries no gradient in the loss)
    const float *tr = a.traj + (long)i * 13 * a.ts, *po = a.pose + (long)i * 72;
    float *dt = a.dtraj + (long)i * 13 * a.ts;
    const float ang = a.angle[i];
    const float c = cosf(ang), s = sinf(ang);
    float dth = 0.0f, ox = 0.0f, oy = 0.0f;
    if (lane < 13) {
        const float px = tr[lane * a.ts], py = tr[lane * a.ts + 1], gx = dx[2 * lane], gy = dx[2 * lane + 1];
        ox = gx * c - gy * s;
        oy = gx * s + gy * c;
        dth += gx * (-px * s + py * c) + gy * (-px * c - py * s);
    }
    if (lane < 24) {
        const bool hidden = lane == 4 || lane == 8 || lane == 9 || lane == 10 || lane == 11;
        if (!hidden) {
            const float px = po[lane * 3], py = po[lane * 3 + 1], gx = dx[26 + lane * 3], gy = dx[26 + lane * 3 + 1];
            dth += gx * (-px * s + py * c) + gy * (-px * c - py * s);
        }
    }
    dth = wave_sum(dth);
    if (lane == 1) locoval_yaw_bwd(tr, a.ts, dth, ox, oy);  // the angle is a function of waypoint 1, whose lane adds that path
    if (lane < 13) {
        dt[lane * a.ts] = ox;
        dt[lane * a.ts + 1] = oy;
        for (int k = 2; k < a.ts; ++k) dt[lane * a.ts + k] = 0.0f;
    }
}

// ------------------------------------------------------------------ narrow variants 28 / 13 / 6 and 26 / 12 / 6
// Four samples per wave, one per 16-lane DPP row; workgroup = 4 waves = LVR_SAMPLES samples.  Lane l of a row is waypoint l in the
// normalisation, unit l of a layer in the MLP.  Rows without work (beyond B, weight 0, no slot) keep walking through the barriers and
// the row sums with their stores masked.  LDS: weights once per workgroup (w1 k-major in the forward, so the 16 lanes of a row read
// 16 consecutive words and the rows of a wave the same ones: no bank conflicts; as stored in the backward, whose lanes run over k),
// activations per sample (two samples of a 32-lane half sit IN words apart: distinct banks).
#define LVR_SAMPLES 16
template <int VEL> struct LocoValRow {
    static constexpr int IN = 26 + 2 * VEL, H1 = IN / 2 - 1, H2 = H1 / 2;
    static constexpr int NPARAM = H1 * IN + H1 + H2 * H1 + H2 + H2 + 1;
    static_assert(H1 <= 16 && H2 <= 8, "one layer unit per lane of a 16-lane row");
};

// value_pose_net.py:73-103 + :110-114 forward_traj / :129-135 forward_vel.  pose_rot (optional): the caller's pose rotated by the
// sample's yaw (:96-97 runs for every variant); it is not an input here and no joint is zeroed.
template <int VEL> __global__ void __launch_bounds__(256)
locoval_row_fwd_kernel(LocoValFwd a) {
    typedef LocoValRow<VEL> D;
    constexpr int IN = D::IN, H1 = D::H1, H2 = D::H2;
    __shared__ float w1t[IN * 16], b1s[16], w2s[H2 * H1], b2s[8], w3s[8], b3s[1];
    __shared__ float xs[LVR_SAMPLES][IN], h1s[LVR_SAMPLES][16], h2s[LVR_SAMPLES][8];
    const int tid = threadIdx.x, l = tid & 15, sm = tid >> 4;
    const int i = blockIdx.x * LVR_SAMPLES + sm;
    for (int e = tid; e < H1 * IN; e += 256) { const int j = e / IN, k = e - j * IN; w1t[k * 16 + j] = a.w1[e]; }
    for (int e = tid; e < H2 * H1; e += 256) w2s[e] = a.w2[e];
    if (tid < H1) b1s[tid] = a.b1[tid];
    if (tid < H2) { b2s[tid] = a.b2[tid]; w3s[tid] = a.w3[tid]; }
    if (tid == 0) b3s[0] = a.b3[0];
    const bool act = i < a.B && (!a.row_weight || a.row_weight[i] != 0.0f);
    if (act) {
        const float *tr = a.traj + (long)i * 13 * a.ts;
        const float ang = locoval_yaw(tr, a.ts);
        const float c = cosf(ang), s = sinf(ang);
        if (l == 0 && a.angle) a.angle[i] = ang;
        if (l < 13) locoval_norm_traj(l, tr, a.ts, c, s, xs[sm]);
        if (VEL && l == 13) locoval_norm_vel(a.vel + (long)i * 2, c, s, xs[sm] + IN - 2);
        if (a.pose_rot)
            for (int j = l; j < 24; j += 16) {
                const float *po = a.pose + (long)i * 72 + j * 3;
                float *pr = a.pose_rot + (long)i * 72 + j * 3;
                const float px = po[0], py = po[1];
                pr[0] = px * c + py * s;
                pr[1] = -px * s + py * c;
                pr[2] = po[2];
            }
    }
    __syncthreads();
    if (act) {
        for (int k = l; k < IN; k += 16) a.x[(long)i * IN + k] = xs[sm][k];
        if (l < H1) {
            const float acc = locoval_unit<IN>(b1s[l], w1t + l, 16, xs[sm]);
            h1s[sm][l] = acc; a.h1[(long)i * H1 + l] = acc;
        }
    }
    __syncthreads();
    if (act && l < H2) {
        const float acc = locoval_unit<H1>(b2s[l], w2s + l * H1, 1, h1s[sm]);
        h2s[sm][l] = acc; a.h2[(long)i * H2 + l] = acc;
    }
    __syncthreads();
    float p = (act && l < H2) ? w3s[l] * h2s[sm][l] : 0.0f;
    p = row_sum(p);
    if (act && l == 0) a.value[i] = locoval_head(p, b3s[0]);
}

template <int VEL> __global__ void __launch_bounds__(256)
locoval_row_bwd_kernel(LocoValBwd a) {
    typedef LocoValRow<VEL> D;
    constexpr int IN = D::IN, H1 = D::H1, H2 = D::H2;
    __shared__ float w1s[H1 * IN], w2s[H2 * H1], w3s[8];
    __shared__ float xs[LVR_SAMPLES][IN], d1s[LVR_SAMPLES][16], d2s[LVR_SAMPLES][8], dxs[LVR_SAMPLES][IN];
    const int tid = threadIdx.x, l = tid & 15, sm = tid >> 4;
    const int i = blockIdx.x * LVR_SAMPLES + sm;
    for (int e = tid; e < H1 * IN; e += 256) w1s[e] = a.w1[e];
    for (int e = tid; e < H2 * H1; e += 256) w2s[e] = a.w2[e];
    if (tid < H2) w3s[tid] = a.w3[tid];
    // sparse mode (slot != NULL): only the rows with a slot contribute, row i's parameter-gradient share goes to ws[slot[i]]
    const int row = i < a.B ? (a.slot ? a.slot[i] : i) : -1;
    const bool act = row >= 0;
    float *g = a.ws + (long)(act ? row : 0) * D::NPARAM;
    float *gw1 = g, *gb1 = g + H1 * IN, *gw2 = gb1 + H1, *gb2 = gw2 + H2 * H1, *gw3 = gb2 + H2, *gb3 = gw3 + H2;
    __syncthreads();
    if (act) {
        for (int k = l; k < IN; k += 16) xs[sm][k] = a.x[(long)i * IN + k];
        const float v = a.value[i];
        const float dz3 = a.dvalue[i] * v * (1.0f - v);
        if (l < H2) {
            const float hv = a.h2[(long)i * H2 + l];
            gw3[l] = dz3 * hv;
            const float dd = hv > 0.0f ? dz3 * w3s[l] : 0.0f;
            d2s[sm][l] = dd; gb2[l] = dd;
        }
        if (l == 0) gb3[0] = dz3;
    }
    __syncthreads();
    if (act && l < H1) {
        const float hv = a.h1[(long)i * H1 + l];
        float acc = 0.0f;
        for (int j = 0; j < H2; ++j) acc += w2s[j * H1 + l] * d2s[sm][j];
        const float dd = hv > 0.0f ? acc : 0.0f;
        d1s[sm][l] = dd; gb1[l] = dd;
        for (int j = 0; j < H2; ++j) gw2[j * H1 + l] = d2s[sm][j] * hv;
    }
    __syncthreads();
    if (act) {
        for (int e = l; e < H1 * IN; e += 16) { const int j = e / IN, k = e - j * IN; gw1[e] = d1s[sm][j] * xs[sm][k]; }
        for (int k = l; k < IN; k += 16) {
            float acc = 0.0f;
            for (int j = 0; j < H1; ++j) acc += w1s[j * IN + k] * d1s[sm][j];
            dxs[sm][k] = acc;
        }
    }
    __syncthreads();
    // back through the yaw normalisation to the trajectory (the velocity carries no gradient in the loss)
    const float *tr = a.traj + (long)(act ? i : 0) * 13 * a.ts;
    float dth = 0.0f, ox = 0.0f, oy = 0.0f;
    if (act) {
        const float ang = a.angle[i];
        const float c = cosf(ang), s = sinf(ang);
        if (l < 13) {
            const float px = tr[l * a.ts], py = tr[l * a.ts + 1], gx = dxs[sm][2 * l], gy = dxs[sm][2 * l + 1];
            ox = gx * c - gy * s;
            oy = gx * s + gy * c;
            dth += gx * (-px * s + py * c) + gy * (-px * c - py * s);
        }
        if (VEL && l == 0) {
            const float *ve = a.vel + (long)i * 2;
            dth += dxs[sm][IN - 2] * (-ve[0] * s + ve[1] * c) + dxs[sm][IN - 1] * (-ve[0] * c - ve[1] * s);
        }
    }
    dth = row_sum(dth);
    if (act && l < 13) {
        if (l == 1) locoval_yaw_bwd(tr, a.ts, dth, ox, oy);
        float *dt = a.dtraj + (long)i * 13 * a.ts;
        dt[l * a.ts] = ox;
        dt[l * a.ts + 1] = oy;
        for (int k = 2; k < a.ts; ++k) dt[l * a.ts + k] = 0.0f;
    }
}

// locoval_reduce_kernel for a row of n_param floats: the same fixed order, eight rows requested at once
__global__ void locoval_reduce_n_kernel(int B, int n_param, const float *ws, float *dparams, const float *count) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_param) return;
    const int rows = count ? (int)count[0] : B;
    float s = 0.0f;
    int i = 0;
    for (; i + 8 <= rows; i += 8) {
        float v[8];
        for (int u = 0; u < 8; ++u) v[u] = ws[(long)(i + u) * n_param + p];
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; i < rows; ++i) s += ws[(long)i * n_param + p];
    dparams[p] = s;
}

// ------------------------------------------------------------------ dispatch: launch(kernel, grid, block, kernel arguments...)
template <class LAUNCH> inline void locoval_variant_fwd(LAUNCH launch, int variant, const LocoValFwd &a) {
    const unsigned B = (unsigned)a.B, groups = (B + LVR_SAMPLES - 1) / LVR_SAMPLES;
    if (variant == 3)
        launch(locoval_fwd_kernel, B, 64u, a.B, a.traj, a.ts, a.pose, a.vel, a.w1, a.b1, a.w2, a.b2, a.w3, a.b3, a.value, a.x, a.h1, a.h2, a.angle,
               a.row_weight);
    else if (variant == 2) launch(locoval_pose_fwd_kernel, B, 64u, a);
    else if (variant == 1) launch(locoval_row_fwd_kernel<1>, groups, 256u, a);
    else launch(locoval_row_fwd_kernel<0>, groups, 256u, a);
}

template <class LAUNCH> inline void locoval_variant_bwd(LAUNCH launch, int variant, const LocoValBwd &a) {
    const unsigned B = (unsigned)a.B, groups = (B + LVR_SAMPLES - 1) / LVR_SAMPLES;
    if (variant == 3) {
        launch(locoval_bwd_kernel, B, 64u, a.B, a.traj, a.ts, a.pose, a.vel, a.w1, a.w2, a.w3, a.value, a.x, a.h1, a.h2, a.angle, a.dvalue, a.ws,
               a.dtraj, a.slot);
        launch(locoval_reduce_kernel, (unsigned)((LV_NPARAM + 255) / 256), 256u, a.B, (const float *)a.ws, a.dparams, a.count);
        return;
    }
    LocoValDims d;
    locoval_dims(variant, &d);
    if (variant == 2) launch(locoval_pose_bwd_kernel, B, 64u, a);
    else if (variant == 1) launch(locoval_row_bwd_kernel<1>, groups, 256u, a);
    else launch(locoval_row_bwd_kernel<0>, groups, 256u, a);
    launch(locoval_reduce_n_kernel, (unsigned)((d.n_param + 255) / 256), 256u, a.B, d.n_param, (const float *)a.ws, a.dparams, a.count);
}

}  // namespace emloco
