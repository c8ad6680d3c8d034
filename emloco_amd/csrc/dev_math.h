// dev_math.h -- device-side vector / quaternion helpers shared by the gfx950 kernels.
// Quaternions are xyzw.  Two groups:
//   (1) plain geometry used by the rigid-body step (Hamilton product, rotation matrix, rotation vector);
//   (2) the reference task code's helpers restated term by term so fp32 observations track it:
//       /root/reference/pacer/pacer/utils/torch_utils.py (my_quat_rotate :14-24, quat_to_tan_norm :66-79,
//       exp_map_to_quat :88-111, calc_heading* :137-175) and
//       /root/reference/isaacgym/python/isaacgym/torch_utils.py (quat_mul :19-41, quat_apply :49-56,
//       quat_from_angle_axis :96-101).
#pragma once
#include <hip/hip_runtime.h>

namespace emloco {

// Closest points of two segments P0P1, Q0Q1 (clamped parametrisation, Ericson RTCD 5.1.9).  Plain + - * / and compares in
// a fixed order (the CPU checker restates the same sequence).
__device__ __forceinline__ float sc_clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }
__device__ __forceinline__ void seg_seg_closest(const float *p0, const float *p1, const float *q0, const float *q1, float *c1, float *c2) {
    const float EPS = 1e-12f;
    float d1[3], d2[3], r[3];
    for (int k = 0; k < 3; ++k) { d1[k] = p1[k] - p0[k]; d2[k] = q1[k] - q0[k]; r[k] = p0[k] - q0[k]; }
    const float a = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2];
    const float e = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
    const float f = d2[0] * r[0] + d2[1] * r[1] + d2[2] * r[2];
    float s = 0.0f, t = 0.0f;
    if (a <= EPS && e <= EPS) { s = 0.0f; t = 0.0f; }
    else if (a <= EPS) { s = 0.0f; t = sc_clamp01(f / e); }
    else {
        const float c = d1[0] * r[0] + d1[1] * r[1] + d1[2] * r[2];
        if (e <= EPS) { t = 0.0f; s = sc_clamp01(-c / a); }
        else {
            const float b = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
            const float den = a * e - b * b;
            s = den > EPS ? sc_clamp01((b * f - c * e) / den) : 0.0f;
            t = (b * s + f) / e;
            if (t < 0.0f) { t = 0.0f; s = sc_clamp01(-c / a); }
            else if (t > 1.0f) { t = 1.0f; s = sc_clamp01((b - c) / a); }
        }
    }
    for (int k = 0; k < 3; ++k) { c1[k] = p0[k] + d1[k] * s; c2[k] = q0[k] + d2[k] * t; }
}

__device__ __forceinline__ void cross3(const float *a, const float *b, float *o) {
    float x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
    o[0] = x; o[1] = y; o[2] = z;
}
__device__ __forceinline__ float dot3(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// Fused sum-of-products forms for the articulated-body factorisation / solves (phases 3, 4, 7): one rounding per term,
// ascending k.  The library is built with -ffp-contract=off, so a fused multiply-add exists only where it is written; the
// CPU checker spells the same chains.
__device__ __forceinline__ float fdot6(const float *a, const float *b) {
    return fmaf(a[5], b[5], fmaf(a[4], b[4], fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])))));
}
#define SOP2(a0, b0, a1, b1) fmaf((a1), (b1), (a0) * (b0))
#define SOP3(a0, b0, a1, b1, a2, b2) fmaf((a2), (b2), fmaf((a1), (b1), (a0) * (b0)))
#define ADD_SOP3(c, a0, b0, a1, b1, a2, b2) fmaf((a2), (b2), fmaf((a1), (b1), fmaf((a0), (b0), (c))))
#define SUB_SOP3(c, a0, b0, a1, b1, a2, b2) fmaf(-(a2), (b2), fmaf(-(a1), (b1), fmaf(-(a0), (b0), (c))))
__device__ __forceinline__ float dot6(const float *a, const float *b) {
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5];
}
__device__ __forceinline__ void qmul(const float *a, const float *b, float *o) {
    float x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    float y = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    float z = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    float w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}
__device__ __forceinline__ void qnormalize(float *q) {
    float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    float s = 1.0f / n;
    q[0] *= s; q[1] *= s; q[2] *= s; q[3] *= s;
}
__device__ __forceinline__ void q2mat(const float *q, float *R) {
    float x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.0f - 2.0f * (y * y + z * z); R[1] = 2.0f * (x * y - z * w); R[2] = 2.0f * (x * z + y * w);
    R[3] = 2.0f * (x * y + z * w); R[4] = 1.0f - 2.0f * (x * x + z * z); R[5] = 2.0f * (y * z - x * w);
    R[6] = 2.0f * (x * z - y * w); R[7] = 2.0f * (y * z + x * w); R[8] = 1.0f - 2.0f * (x * x + y * y);
}
__device__ __forceinline__ void matvec3(const float *R, const float *v, float *o) {
    float x = R[0] * v[0] + R[1] * v[1] + R[2] * v[2];
    float y = R[3] * v[0] + R[4] * v[1] + R[5] * v[2];
    float z = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
    o[0] = x; o[1] = y; o[2] = z;
}
// Deterministic sin/cos/atan from +,-,*,/ and sqrt only (correctly rounded in IEEE fp32): with
// -ffp-contract=off the rigid-body step reproduces the CPU oracle bit for bit.
__device__ __forceinline__ void det_sincos(float x, float *sn, float *cs) {
    const float inv_pi = 0.318309886f, pi_hi = 3.140625f, pi_lo = 9.67653589793e-4f;
    const float kf = floorf(x * inv_pi + 0.5f);
    const float y = (x - kf * pi_hi) - kf * pi_lo;
    const float y2 = y * y;
    const float ps = 1.0f + y2 * (-1.0f / 6.0f + y2 * (1.0f / 120.0f + y2 * (-1.0f / 5040.0f + y2 * (1.0f / 362880.0f +
                     y2 * (-1.0f / 39916800.0f + y2 * (1.0f / 6227020800.0f))))));
    const float pc = 1.0f + y2 * (-0.5f + y2 * (1.0f / 24.0f + y2 * (-1.0f / 720.0f + y2 * (1.0f / 40320.0f +
                     y2 * (-1.0f / 3628800.0f + y2 * (1.0f / 479001600.0f + y2 * (-1.0f / 87178291200.0f)))))));
    const float sgn = (((long)kf) & 1) ? -1.0f : 1.0f;
    *sn = sgn * (y * ps);
    *cs = sgn * pc;
}
__device__ __forceinline__ float det_atan01(float t) {
    const float u = t / (1.0f + sqrtf(1.0f + t * t));
    const float u2 = u * u;
    const float p = 1.0f + u2 * (-1.0f / 3.0f + u2 * (1.0f / 5.0f + u2 * (-1.0f / 7.0f + u2 * (1.0f / 9.0f + u2 * (-1.0f / 11.0f +
                    u2 * (1.0f / 13.0f + u2 * (-1.0f / 15.0f + u2 * (1.0f / 17.0f))))))));
    return 2.0f * (u * p);
}
__device__ __forceinline__ float det_atan2_pos(float s, float w) {
    if (s <= w) return w > 0.0f ? det_atan01(s / w) : 0.0f;
    return 1.57079637f - det_atan01(w / s);
}
__device__ __forceinline__ void rotvec2quat(const float *e, float *q) {
    float th2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
    float th = sqrtf(th2);
    float k, c;
    if (th < 1e-4f) { k = 0.5f - th2 * (1.0f / 48.0f); c = 1.0f - th2 * 0.125f; }
    else { float sn; det_sincos(0.5f * th, &sn, &c); k = sn / th; }
    q[0] = e[0] * k; q[1] = e[1] * k; q[2] = e[2] * k; q[3] = c;
}
__device__ __forceinline__ void quat2rotvec(const float *qin, float *e) {
    float q[4] = {qin[0], qin[1], qin[2], qin[3]};
    if (q[3] < 0.0f) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    float s = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    float k;
    if (s < 1e-6f) k = 2.0f;
    else k = 2.0f * det_atan2_pos(s, q[3]) / s;
    e[0] = q[0] * k; e[1] = q[1] * k; e[2] = q[2] * k;
}

// Transcendentals of the reference task code (atan2 / sin / cos / acos of torch's CPU path): evaluated in double precision and
// rounded once, i.e. correctly rounded fp32 results -- the same on the device, in the emulator and in the oracle
// (the CPU restatement used by the tests does the same), and the best available stand-in for torch's own last bit (its CPU sin / cos go
// through MKL's closed VML, ~5 % of values differ from the correctly rounded one by 1 ulp).  The heading quaternion behind
// the terrain probes comes from these, so the map indices (p / 0.1).long() are identical across the three.
__device__ __forceinline__ float cr_sinf(float x) { return (float)sin((double)x); }
__device__ __forceinline__ float cr_cosf(float x) { return (float)cos((double)x); }
// both at once (one argument reduction): the double results are the ones sin() / cos() give, rounded the same way
__device__ __forceinline__ void cr_sincosf(float x, float *s, float *c) {
    double ds, dc;
    sincos((double)x, &ds, &dc);
    *s = (float)ds; *c = (float)dc;
}
__device__ __forceinline__ float cr_atan2f(float y, float x) { return (float)atan2((double)y, (double)x); }
__device__ __forceinline__ float cr_acosf(float x) { return (float)acos((double)x); }

// ---- reference task-code helpers (group 2) -------------------------------------------------
__device__ __forceinline__ void ref_quat_rotate(const float *q, const float *v, float *o) {
    float w = q[3];
    float s = 2.0f * (w * w) - 1.0f;
    float cx = q[1] * v[2] - q[2] * v[1];
    float cy = q[2] * v[0] - q[0] * v[2];
    float cz = q[0] * v[1] - q[1] * v[0];
    float d = q[0] * v[0] + q[1] * v[1] + q[2] * v[2];
    o[0] = (v[0] * s + cx * w * 2.0f) + q[0] * d * 2.0f;
    o[1] = (v[1] * s + cy * w * 2.0f) + q[1] * d * 2.0f;
    o[2] = (v[2] * s + cz * w * 2.0f) + q[2] * d * 2.0f;
}
__device__ __forceinline__ void ref_quat_mul(const float *a, const float *b, float *o) {
    float x1 = a[0], y1 = a[1], z1 = a[2], w1 = a[3];
    float x2 = b[0], y2 = b[1], z2 = b[2], w2 = b[3];
    float ww = (z1 + x1) * (x2 + y2);
    float yy = (w1 - y1) * (w2 + z2);
    float zz = (w1 + y1) * (w2 - z2);
    float xx = ww + yy + zz;
    float qq = 0.5f * (xx + (z1 - x1) * (x2 - y2));
    o[3] = qq - ww + (z1 - y1) * (y2 - z2);
    o[0] = qq - xx + (x1 + w1) * (x2 + w2);
    o[1] = qq - yy + (w1 - x1) * (y2 + z2);
    o[2] = qq - zz + (z1 + y1) * (w2 - x2);
}
__device__ __forceinline__ void ref_quat_apply(const float *a, const float *b, float *o) {
    float tx = (a[1] * b[2] - a[2] * b[1]) * 2.0f;
    float ty = (a[2] * b[0] - a[0] * b[2]) * 2.0f;
    float tz = (a[0] * b[1] - a[1] * b[0]) * 2.0f;
    float ux = a[1] * tz - a[2] * ty;
    float uy = a[2] * tx - a[0] * tz;
    float uz = a[0] * ty - a[1] * tx;
    o[0] = (b[0] + a[3] * tx) + ux;
    o[1] = (b[1] + a[3] * ty) + uy;
    o[2] = (b[2] + a[3] * tz) + uz;
}
// quat_from_angle_axis about +z: normalize(axis) = z, then the quaternion is re-normalised
__device__ __forceinline__ void ref_quat_about_z(float angle, float *o) {
    float th = angle / 2.0f;
    float s, c;
    cr_sincosf(th, &s, &c);
    float n = sqrtf(s * s + c * c);
    if (n < 1e-9f) n = 1e-9f;
    o[0] = 0.0f / n; o[1] = 0.0f / n; o[2] = s / n; o[3] = c / n;
}
__device__ __forceinline__ float ref_calc_heading(const float *q) {
    const float ex[3] = {1.0f, 0.0f, 0.0f};
    float r[3];
    ref_quat_rotate(q, ex, r);
    return cr_atan2f(r[1], r[0]);
}
__device__ __forceinline__ void ref_quat_to_tan_norm(const float *q, float *o6) {
    const float ex[3] = {1.0f, 0.0f, 0.0f}, ez[3] = {0.0f, 0.0f, 1.0f};
    ref_quat_rotate(q, ex, o6);
    ref_quat_rotate(q, ez, o6 + 3);
}
__device__ __forceinline__ void ref_exp_map_to_quat(const float *e, float *o) {
    float angle = sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    float ax[3] = {e[0] / angle, e[1] / angle, e[2] / angle};
    { float sa, ca; cr_sincosf(angle, &sa, &ca); angle = cr_atan2f(sa, ca); }
    if (!(fabsf(angle) > 1e-5f)) { angle = 0.0f; ax[0] = 0.0f; ax[1] = 0.0f; ax[2] = 1.0f; }
    float n = sqrtf(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    if (n < 1e-9f) n = 1e-9f;
    float th = angle / 2.0f;
    float s, c;
    cr_sincosf(th, &s, &c);
    float q[4] = {ax[0] / n * s, ax[1] / n * s, ax[2] / n * s, c};
    float qn = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (qn < 1e-9f) qn = 1e-9f;
    o[0] = q[0] / qn; o[1] = q[1] / qn; o[2] = q[2] / qn; o[3] = q[3] / qn;
}

// Wave-wide sum on the DPP crossbar (no LDS round trips): inside each 16-lane row  v += row_mirror(v);
// v += row_half_mirror(v); v += quad_perm[1,0,3,2](v); v += quad_perm[2,3,0,1](v)  -- every lane of a row then
// holds the row total -- and the four row totals are added as ((r0 + r1) + r2) + r3.  The association order is
// fixed and is the one the CPU oracle uses (oracle_sim.c: wave_sum_order), so Gauss-Seidel residuals agree bit
// for bit.  ~10 VALU-latency steps instead of 6 dependent ds_bpermute round trips.
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float lane_bcast(float v, int src_lane /* wave-uniform */) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}
// The sum of one 16-lane DPP row, left in every lane of that row: the four rows of a wave are summed independently (four samples per
// wave in the narrow LocoVal kernels, locoval_variants.h).  The CPU emulation executes the same four permutations
// (tests/emu/hip/hip_runtime.h: __builtin_amdgcn_update_dpp), so the association order is one source for both.
__device__ __forceinline__ float row_sum(float v) {
    v += dpp_mov<0x140>(v);   // row_mirror
    v += dpp_mov<0x141>(v);   // row_half_mirror
    v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    v = row_sum(v);
    return ((lane_bcast(v, 0) + lane_bcast(v, 16)) + lane_bcast(v, 32)) + lane_bcast(v, 48);   // fixed order r0+r1+r2+r3
}

}  // namespace emloco

namespace emloco {
// pacer/pacer/utils/torch_utils.py:113-135 slerp
__device__ __forceinline__ void ref_slerp(const float *q0, const float *q1in, float t, float *o) {
    float q1[4] = {q1in[0], q1in[1], q1in[2], q1in[3]};
    float c = q0[0] * q1[0] + q0[1] * q1[1] + q0[2] * q1[2] + q0[3] * q1[3];
    if (c < 0.0f) { q1[0] = -q1[0]; q1[1] = -q1[1]; q1[2] = -q1[2]; q1[3] = -q1[3]; }
    c = fabsf(c);
    const float half = cr_acosf(c);
    const float s = sqrtf(1.0f - c * c);
    const float ra = cr_sinf((1.0f - t) * half) / s, rb = cr_sinf(t * half) / s;
    for (int i = 0; i < 4; ++i) {
        float v = ra * q0[i] + rb * q1[i];
        if (fabsf(s) < 0.001f) v = 0.5f * q0[i] + 0.5f * q1[i];
        if (fabsf(c) >= 1.0f) v = q0[i];
        o[i] = v;
    }
}
// pacer/pacer/utils/torch_utils.py:26-64 quat_to_exp_map
__device__ __forceinline__ void ref_quat_to_exp_map(const float *q, float *o) {
    const float sin_theta = sqrtf(1.0f - q[3] * q[3]);
    float angle = 2.0f * cr_acosf(q[3]);
    { float sa, ca; cr_sincosf(angle, &sa, &ca); angle = cr_atan2f(sa, ca); }
    if (fabsf(sin_theta) > 1e-5f) {
        o[0] = angle * (q[0] / sin_theta); o[1] = angle * (q[1] / sin_theta); o[2] = angle * (q[2] / sin_theta);
    } else { o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f; }
}
}  // namespace emloco
