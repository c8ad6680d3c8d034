// locoval_refine.h -- test-time refinement of predicted paths against a LocoVal network: the whole optimisation loop in one launch.
//
// plausibl/test_value_mlp.py:239-274 (class Opt) makes the trajectories a leaf tensor and runs 750 steps of Adam(lr = 1e-4) on
// exp(-V).mean(); V is the network of value_pose_net.py:73-159.  Every trajectory is an independent problem and the loop is
// hundreds of dependent steps on 24 numbers, so here a row keeps its 24 free coordinates, their Adam moments and the activations
// on chip for all the steps, and the weights sit once per workgroup in LDS.  No parameter gradient is formed and no workspace in
// HBM is used beyond the outputs.
//
// Per step, with p the xy of waypoints 1..12 (waypoint 0 and the columns from 2 on are copied through), p0 their input values:
//     L = grad_scale * exp(-V(p)) + anchor_w / 12 * sum_k |p_k - p0_k|^2
//     g = dL/dp through the MLP, the rotation and the yaw angle (locoval_yaw_bwd for waypoint 1, the guarded x without a gradient;
//         the angle's path includes the pose and velocity inputs' terms, as in locoval_bwd_kernel, though both are constants here)
//     m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)    (torch.optim.Adam)
// The objective is the reference's up to the batch mean: exp(-V).mean() over N rows is grad_scale = 1 / N.  The default of the
// callers is 1: Adam cancels the scale except through eps, and a row's result must not depend on which rows share its launch.
//
// Mapping (as the forward / backward kernels of the same variant): the pose-reading variants (3, 2) one trajectory per wave, four to
// a 256-thread workgroup; the narrow ones (1, 0) one per 16-lane DPP row, sixteen to a workgroup.  A trajectory never leaves its
// wave; lane l is waypoint l in the normalisation and the Adam step, unit l of a layer in the MLP.
//
// What is bit-equal to the forward kernels and what is not.  value_before and value_after are computed by `refine_value` from the
// shared pieces (locoval_yaw, locoval_norm_*, locoval_unit, locoval_head) in the forward kernels' statement order: the bits of
// emloco_locoval_variant_fwd on traj and on traj_out.  The steps in between factor the first layer: pose and velocity enter a step
// only through the angle (x = px c + py s, y = -px s + py c), so their share of unit j is C_j + c A_j + s B_j with A, B, C summed
// once per row, and its angle derivative is -s A_j + c B_j.  A step then costs 26 + 2 products per unit instead of `in`, and d x is
// formed for the 26 trajectory inputs only; its sums run in another order than the forward kernels'.
//
// LDS per workgroup: W1's 26 trajectory columns in both layouts (k-major for the forward, whose lanes are units; row-major for
// d x[k] = sum_j W1[j][k] d1[j], whose lanes run over k), W2 in both, b2, w3, b3, and per trajectory p, x, h1, d1, d2, d x:
// 24 192 B for the full network (19 796 B of weights + 4 x 1 096 B), 23 716 B for the pose variant, 10 584 B and 10 040 B for the
// narrow ones (3.3 KB of weights + 16 trajectories) -- six workgroups of the full network fit a CU's 160 KB; its 120 registers
// allow four.
// Included by predictor_capi.hip after predictor_kernels.hip (not part of the CPU emulation's sources).
#pragma once

namespace emloco {

struct LocoValRefine {
    int B;
    const float *traj; int ts;
    const float *pose, *vel, *w1, *b1, *w2, *b2, *w3, *b3;
    const uint8_t *row_mask /* or NULL: every row */;
    int n_steps;
    float lr, beta1, beta2, eps, grad_scale, anchor_g /* anchor_w * 2 / 12: the anchor's gradient per coordinate of p - p0 */;
    float *traj_out, *value_before, *value_after, *grad0 /* or NULL */;
};

template <int V> struct LocoValRefineDims {
    static constexpr bool POSE = (V & 2) != 0, VEL = (V & 1) != 0;
    static constexpr int IN = 26 + (POSE ? 72 : 0) + (VEL ? 2 : 0), H1 = IN / 2 - 1, H2 = H1 / 2;
    static constexpr int LANES = POSE ? 64 : 16, ROWS = 256 / LANES;      // lanes per trajectory, trajectories per workgroup
    static_assert(H1 <= LANES && H2 <= LANES && 13 <= LANES, "one layer unit / one waypoint per lane");
};

template <int LANES> __device__ __forceinline__ float refine_group_sum(float v) { return LANES == 64 ? wave_sum(v) : row_sum(v); }

// The value of the trajectory in p (13 waypoints, stride 2) as the variant's forward kernel computes it, in every lane of the group.
template <int V> __device__ __forceinline__ float
refine_value(const LocoValRefine &a, bool act, int l, const float *p, const float *po, const float *ve, float *x, float *h1) {
    typedef LocoValRefineDims<V> D;
    if (act) {
        const float ang = locoval_yaw(p, 2);
        const float c = cosf(ang), s = sinf(ang);
        if (l < 13) locoval_norm_traj(l, p, 2, c, s, x);
        if (D::POSE && l < 24) locoval_norm_pose(l, po, c, s, x + 26);
        if (D::VEL && l == (D::POSE ? 0 : 13)) locoval_norm_vel(ve, c, s, x + D::IN - 2);
    }
    __syncthreads();
    if (act && l < D::H1) h1[l] = locoval_unit<D::IN>(a.b1[l], a.w1 + l * D::IN, 1, x);
    __syncthreads();
    float h2 = 0.0f;
    if (act && l < D::H2) h2 = locoval_unit<D::H1>(a.b2[l], a.w2 + l * D::H1, 1, h1);
    float q = (act && l < D::H2) ? a.w3[l] * h2 : 0.0f;
    q = refine_group_sum<D::LANES>(q);
    return locoval_head(q, a.b3[0]);
}

template <int V> __global__ void __launch_bounds__(256)
locoval_refine_kernel(LocoValRefine a) {
    typedef LocoValRefineDims<V> D;
    constexpr int IN = D::IN, H1 = D::H1, H2 = D::H2, LANES = D::LANES, ROWS = D::ROWS;
    __shared__ float w1t[26 * H1], w1r[H1 * 26], w2t[H1 * H2], w2r[H2 * H1], b2s[H2], w3s[H2], b3s[1];
    __shared__ float ps[ROWS][26], xs[ROWS][IN], h1s[ROWS][H1], d1s[ROWS][H1], d2s[ROWS][H2], dxs[ROWS][26];
    const int tid = threadIdx.x, l = tid % LANES, sm = tid / LANES;
    const int i = blockIdx.x * ROWS + sm;
    const bool inr = i < a.B, act = inr && (!a.row_mask || a.row_mask[i] != 0);
    for (int e = tid; e < H1 * 26; e += 256) {
        const int j = e / 26, k = e - j * 26;
        const float w = a.w1[j * IN + k];
        w1r[e] = w; w1t[k * H1 + j] = w;
    }
    for (int e = tid; e < H2 * H1; e += 256) {
        const int j = e / H1, k = e - j * H1;
        const float w = a.w2[e];
        w2r[e] = w; w2t[k * H2 + j] = w;
    }
    if (tid < H2) { b2s[tid] = a.b2[tid]; w3s[tid] = a.w3[tid]; }
    if (tid == 0) b3s[0] = a.b3[0];
    const long row = inr ? i : 0;
    const float *tr = a.traj + row * 13 * a.ts;
    const float *po = D::POSE ? a.pose + row * 72 : nullptr, *ve = D::VEL ? a.vel + row * 2 : nullptr;
    float *out = a.traj_out + row * 13 * a.ts;
    if (inr && !act && l < 13)                               // a masked row: the trajectory as it came, the value entries untouched
        for (int k = 0; k < a.ts; ++k) out[l * a.ts + k] = tr[l * a.ts + k];
    float px = 0.0f, py = 0.0f;                             // this lane's waypoint
    if (act && l < 13) { px = tr[l * a.ts]; py = tr[l * a.ts + 1]; ps[sm][2 * l] = px; ps[sm][2 * l + 1] = py; }
    const float p0x = px, p0y = py;
    __syncthreads();
    const float v0 = refine_value<V>(a, act, l, ps[sm], po, ve, xs[sm], h1s[sm]);
    if (act && l == 0) { a.value_before[i] = v0; if (a.n_steps == 0) a.value_after[i] = v0; }
    if (a.n_steps > 0) {
        // the constant inputs' share of unit l: C + c A + s B
        float A = 0.0f, Bq = 0.0f, Cq = 0.0f;
        if (act && l < H1) {
            const float *w = a.w1 + l * IN;
            Cq = a.b1[l];
            if (D::POSE)
                for (int j = 0; j < 24; ++j) {
                    if (j == 4 || j == 8 || j == 9 || j == 10 || j == 11) continue;
                    const float wx = w[26 + j * 3], wy = w[26 + j * 3 + 1], wz = w[26 + j * 3 + 2];
                    const float qx = po[j * 3], qy = po[j * 3 + 1], qz = po[j * 3 + 2];
                    A += wx * qx + wy * qy;
                    Bq += wx * qy - wy * qx;
                    Cq += wz * qz;
                }
            if (D::VEL) {
                const float wx = w[IN - 2], wy = w[IN - 1];
                A += wx * ve[0] + wy * ve[1];
                Bq += wx * ve[1] - wy * ve[0];
            }
        }
        float mx = 0.0f, my = 0.0f, vx = 0.0f, vy = 0.0f;
        double b1t = 1.0, b2t = 1.0;
        for (int t = 1; t <= a.n_steps; ++t) {
            b1t *= (double)a.beta1; b2t *= (double)a.beta2;
            __syncthreads();                                 // p of the last step is in ps
            float c = 1.0f, s = 0.0f;
            if (act) {
                const float ang = locoval_yaw(ps[sm], 2);
                c = cosf(ang); s = sinf(ang);
                if (l < 13) { xs[sm][2 * l] = px * c + py * s; xs[sm][2 * l + 1] = -px * s + py * c; }
            }
            __syncthreads();
            float h1v = 0.0f;
            if (act && l < H1) {
                float z = Cq + c * A + s * Bq;
                for (int k = 0; k < 26; ++k) z += w1t[k * H1 + l] * xs[sm][k];
                h1v = z > 0.0f ? z : 0.0f;
                h1s[sm][l] = h1v;
            }
            __syncthreads();
            float h2v = 0.0f;
            if (act && l < H2) {
                float z = b2s[l];
                for (int k = 0; k < H1; ++k) z += w2t[k * H2 + l] * h1s[sm][k];
                h2v = z > 0.0f ? z : 0.0f;
            }
            const float val = locoval_head(refine_group_sum<LANES>((act && l < H2) ? w3s[l] * h2v : 0.0f), b3s[0]);
            const float dz3 = -a.grad_scale * expf(-val) * val * (1.0f - val);
            if (act && l < H2) d2s[sm][l] = h2v > 0.0f ? dz3 * w3s[l] : 0.0f;
            __syncthreads();
            float dth = 0.0f;                                // d L / d angle, this lane's share
            if (act && l < H1) {
                float acc = 0.0f;
                for (int j = 0; j < H2; ++j) acc += w2r[j * H1 + l] * d2s[sm][j];
                const float dd = h1v > 0.0f ? acc : 0.0f;
                d1s[sm][l] = dd;
                dth = dd * (c * Bq - s * A);
            }
            __syncthreads();
            if (act)
                for (int k = l; k < 26; k += LANES) {
                    float acc = 0.0f;
                    for (int j = 0; j < H1; ++j) acc += w1r[j * 26 + k] * d1s[sm][j];
                    dxs[sm][k] = acc;
                }
            __syncthreads();
            float ox = 0.0f, oy = 0.0f;
            if (act && l < 13) {
                const float gx = dxs[sm][2 * l], gy = dxs[sm][2 * l + 1];
                ox = gx * c - gy * s;
                oy = gx * s + gy * c;
                dth += gx * (-px * s + py * c) + gy * (-px * c - py * s);
            }
            dth = refine_group_sum<LANES>(dth);
            if (act && l >= 1 && l < 13) {
                if (l == 1) locoval_yaw_bwd(ps[sm], 2, dth, ox, oy);
                ox += a.anchor_g * (px - p0x);
                oy += a.anchor_g * (py - p0y);
                if (t == 1 && a.grad0) { a.grad0[((long)i * 12 + (l - 1)) * 2] = ox; a.grad0[((long)i * 12 + (l - 1)) * 2 + 1] = oy; }
                const float step = (float)((double)a.lr / (1.0 - b1t)), bc2 = (float)sqrt(1.0 - b2t);
                mx = a.beta1 * mx + (1.0f - a.beta1) * ox; my = a.beta1 * my + (1.0f - a.beta1) * oy;
                vx = a.beta2 * vx + (1.0f - a.beta2) * ox * ox; vy = a.beta2 * vy + (1.0f - a.beta2) * oy * oy;
                px -= step * mx / (sqrtf(vx) / bc2 + a.eps);
                py -= step * my / (sqrtf(vy) / bc2 + a.eps);
                ps[sm][2 * l] = px; ps[sm][2 * l + 1] = py;
            }
        }
        __syncthreads();
        const float v1 = refine_value<V>(a, act, l, ps[sm], po, ve, xs[sm], h1s[sm]);
        if (act && l == 0) a.value_after[i] = v1;
    }
    if (act && l < 13) {
        out[l * a.ts] = px; out[l * a.ts + 1] = py;
        for (int k = 2; k < a.ts; ++k) out[l * a.ts + k] = tr[l * a.ts + k];
    }
}

template <class LAUNCH> inline void locoval_refine(LAUNCH launch, int variant, const LocoValRefine &a) {
    const unsigned B = (unsigned)a.B;
    if (variant == 3) launch(locoval_refine_kernel<3>, (B + 3) / 4, 256u, a);
    else if (variant == 2) launch(locoval_refine_kernel<2>, (B + 3) / 4, 256u, a);
    else if (variant == 1) launch(locoval_refine_kernel<1>, (B + 15) / 16, 256u, a);
    else launch(locoval_refine_kernel<0>, (B + 15) / 16, 256u, a);
}

}  // namespace emloco
