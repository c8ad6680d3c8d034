// traj_kernels.hip -- waypoint tracks to dense path vertices through a natural cubic spline (emloco_traj_densify, include/emloco_task.h).
//
// What scipy.interpolate.CubicSpline(knot_t, way, axis=0, bc_type='natural')(query_t) computes for every track of a batch
// (social-transmotion/load_jta_traj.py:93-95: 13 waypoints at 0.4 s -> the 101 vertices TrajGenerator follows).  The spline is solved for
// its second derivatives M (M = 0 at both end knots): the n - 2 interior ones satisfy
//     h[i-1] M[i-1] + 2 (h[i-1] + h[i]) M[i] + h[i] M[i+1] = 6 (s[i] - s[i-1]),      h[i] = t[i+1] - t[i],  s[i] = (y[i+1] - y[i]) / h[i]
// a tridiagonal system whose matrix depends on the knots only.  On piece i
//     S(x) = y[i] + d (b[i] + d (M[i] / 2 + d (M[i+1] - M[i]) / (6 h[i]))),           d = x - t[i],  b[i] = s[i] - h[i] (2 M[i] + M[i+1]) / 6
// and a query outside the knots takes the nearest end piece, as scipy extrapolates.
//
// One workgroup of 256 lanes serves DENSIFY_TPB = 64 consecutive tracks:
//   1. lane 0 factors the tridiagonal matrix (Thomas: the modified super-diagonal and the pivots) into LDS, lanes 0..n_query-1 find
//      the piece and the offset d of their query -- both once per workgroup, shared by its 192 solves;
//   2. the workgroup's waypoints, contiguous in memory, are read with consecutive lanes on consecutive floats, shifted by the track's
//      first waypoint (x, y) -- the spline is translation-invariant and fp32 at +-100 m world coordinates costs a decimal digit
//      otherwise -- and tested for non-finite values;
//   3. lanes 0..191 each solve one (track, coordinate): a forward and a back substitution of n - 2 steps;
//   4. all lanes evaluate the workgroup's contiguous tracks x n_query x 3 outputs, consecutive lanes writing consecutive floats (the
//      kernel is write-bound: 156 B in, 1 212 B out per track at 13 knots / 101 queries).
// Plain fp32 arithmetic in a fixed order (the unit is built with -ffp-contract=off), no atomics: tests/emu/emu_task.cpp runs
// the same source on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace emloco {

constexpr int DENSIFY_MIN_KNOTS = 4, DENSIFY_MAX_KNOTS = 16, DENSIFY_MAX_QUERY = 128;
constexpr int DENSIFY_TPB = 64, DENSIFY_THREADS = 256;
constexpr int DENSIFY_FLAG_ORIGIN = 1;             // EMLOCO_DENSIFY_ORIGIN

// knots and queries travel by value with the launch: the host validates them, nothing is copied or synchronised
struct DensifyArgs {
    int n_knots, n_query, flags;
    long long n_traj;
    float knot[DENSIFY_MAX_KNOTS];
    float query[DENSIFY_MAX_QUERY];
};

// Fills `a` from the caller's host arrays; nullptr, or what is wrong with them.
inline const char *densify_pack(const float *knot_t, int n_knots, long long n_traj, const float *query_t, int n_query, int flags, DensifyArgs *a) {
    if (!knot_t || !query_t) return "null knots or queries";
    if (n_knots < DENSIFY_MIN_KNOTS || n_knots > DENSIFY_MAX_KNOTS) return "n_knots must be in [4, 16]";
    if (n_query < 1 || n_query > DENSIFY_MAX_QUERY) return "n_query must be in [1, 128]";
    if (n_traj < 0 || n_traj > (long long)DENSIFY_TPB * 0x7fffffffLL) return "bad n_traj";
    if (flags & ~DENSIFY_FLAG_ORIGIN) return "unknown flag";
    for (int i = 0; i < n_knots; ++i) {
        if (!(knot_t[i] - knot_t[i] == 0.0f)) return "knots must be finite";
        if (i > 0 && !(knot_t[i] > knot_t[i - 1])) return "knots must be strictly increasing";
    }
    for (int q = 0; q < n_query; ++q)
        if (!(query_t[q] - query_t[q] == 0.0f)) return "queries must be finite";
    a->n_knots = n_knots; a->n_query = n_query; a->flags = flags; a->n_traj = n_traj;
    for (int i = 0; i < DENSIFY_MAX_KNOTS; ++i) a->knot[i] = i < n_knots ? knot_t[i] : 0.0f;
    for (int q = 0; q < DENSIFY_MAX_QUERY; ++q) a->query[q] = q < n_query ? query_t[q] : 0.0f;
    return nullptr;
}

__device__ __forceinline__ bool densify_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(DENSIFY_THREADS) void traj_densify_kernel(const DensifyArgs a, const float *__restrict__ way, float *__restrict__ out,
                                                                       uint8_t *__restrict__ valid) {
    constexpr int ROW = DENSIFY_MAX_KNOTS * 3;
    __shared__ float sh_h[DENSIFY_MAX_KNOTS], sh_cp[DENSIFY_MAX_KNOTS], sh_den[DENSIFY_MAX_KNOTS], sh_inv6h[DENSIFY_MAX_KNOTS];
    __shared__ float sh_qd[DENSIFY_MAX_QUERY];
    __shared__ int sh_qi[DENSIFY_MAX_QUERY];
    __shared__ float sh_y[DENSIFY_TPB * ROW], sh_b[DENSIFY_TPB * ROW], sh_m[DENSIFY_TPB * ROW];      // [track][knot][coordinate]
    __shared__ float sh_org[DENSIFY_TPB * 2];
    __shared__ int sh_bad[DENSIFY_TPB];

    const int tid = (int)threadIdx.x;
    const int n = a.n_knots, nq = a.n_query;
    const long long t0 = (long long)blockIdx.x * DENSIFY_TPB;
    const long long left = a.n_traj - t0;
    const int nt = left < DENSIFY_TPB ? (int)left : DENSIFY_TPB;            // tracks of this workgroup (>= 1 by the grid size)
    const int row = n * 3;

    // 1. what depends on the knots and the queries only
    if (tid == 0) {
        for (int i = 0; i < n - 1; ++i) {
            const float h = a.knot[i + 1] - a.knot[i];
            sh_h[i] = h;
            sh_inv6h[i] = 1.0f / (6.0f * h);
        }
        sh_cp[0] = 0.0f; sh_den[0] = 1.0f;
        for (int i = 1; i <= n - 2; ++i) {                                   // rows of the interior unknowns M[1..n-2]
            const float diag = 2.0f * (sh_h[i - 1] + sh_h[i]);
            const float den = i == 1 ? diag : diag - sh_h[i - 1] * sh_cp[i - 1];
            sh_den[i] = den;
            sh_cp[i] = sh_h[i] / den;
        }
    }
    if (tid < nq) {
        const float x = a.query[tid];
        int p = 0;
        for (int i = 1; i <= n - 2; ++i) p = x >= a.knot[i] ? i : p;         // piece [t[p], t[p+1]); outside the knots: the end piece
        sh_qi[tid] = p;
        sh_qd[tid] = x - a.knot[p];
    }
    if (tid < DENSIFY_TPB) sh_bad[tid] = 0;
    __syncthreads();

    // 2. the waypoints, origin-shifted
    const float *src = way + t0 * row;
    for (int e = tid; e < nt * row; e += DENSIFY_THREADS) {
        const int t = e / row, r = e - t * row, c = r % 3;
        const float v = src[e];
        float o = 0.0f;
        if (c < 2) {
            o = src[t * row + c];
            if (r < 2) sh_org[t * 2 + c] = v;
        }
        if (densify_nonfinite(v)) sh_bad[t] = 1;                             // (every writer stores the same value)
        sh_y[t * ROW + r] = v - o;
    }
    __syncthreads();

    // 3. one (track, coordinate) per lane
    if (tid < nt * 3) {
        const int t = tid / 3, c = tid - t * 3;
        float *y = sh_y + t * ROW + c, *b = sh_b + t * ROW + c, *m = sh_m + t * ROW + c;
        float s_prev = (y[3] - y[0]) / sh_h[0];
        b[0] = s_prev;
        float dp = 0.0f;
        for (int i = 1; i <= n - 2; ++i) {
            const float s = (y[3 * (i + 1)] - y[3 * i]) / sh_h[i];
            b[3 * i] = s;
            const float rhs = 6.0f * (s - s_prev);
            dp = (i == 1 ? rhs : rhs - sh_h[i - 1] * dp) / sh_den[i];
            m[3 * i] = dp;
            s_prev = s;
        }
        m[0] = 0.0f; m[3 * (n - 1)] = 0.0f;
        for (int i = n - 3; i >= 1; --i) m[3 * i] = m[3 * i] - sh_cp[i] * m[3 * (i + 1)];
        for (int i = 0; i <= n - 2; ++i) b[3 * i] = b[3 * i] - sh_h[i] * (2.0f * m[3 * i] + m[3 * (i + 1)]) / 6.0f;
    }
    __syncthreads();

    // 4. the outputs: element o of the workgroup's nt * nq * 3 consecutive floats belongs to (track t, query r / 3, coordinate r % 3)
    const int per = nq * 3;
    const int total = nt * per;
    float *dst = out + t0 * per;
    const bool keep_origin = !(a.flags & DENSIFY_FLAG_ORIGIN);
    int t = tid / per, r = tid - t * per;
    for (int o = tid; o < total; o += DENSIFY_THREADS) {
        const int q = r / 3, c = r - q * 3;
        const int p = sh_qi[q];
        const float d = sh_qd[q];
        const int k = t * ROW + 3 * p + c;
        const float m0 = sh_m[k], m1 = sh_m[k + 3];
        float v = sh_y[k] + d * (sh_b[k] + d * (0.5f * m0 + d * ((m1 - m0) * sh_inv6h[p])));
        if (keep_origin && c < 2) v = v + sh_org[t * 2 + c];
        dst[o] = sh_bad[t] ? 0.0f : v;
        r += DENSIFY_THREADS;
        while (r >= per) { r -= per; ++t; }
    }
    if (valid && tid < nt) valid[t0 + tid] = sh_bad[tid] ? 0 : 1;
}

}  // namespace emloco
