// motion_kernels.hip -- the motion library's clip cache from raw clip frames (emloco_motion_build, include/emloco_task.h).
//
// What utils/motion_lib_smpl.py `clip_cache` computes per (clip, skeleton) pair on the host in float64, for a batch of pairs in
// float32: from the global body rotations gq [T][24][4] (xyzw) and the root translation [T][3] of a clip
//     grs  = gq, bit for bit
//     lrs  = qnormalize(inv(gq[parent]) * gq)                       (the root's = its gq; real part non-negative)
//     gts  = forward kinematics over the skeleton's local translations: gp[b] = gp[parent] + rotate(gq[parent], lt[b])
//     gvs  = gaussian(np.gradient(gp, axis = time)) / dt            (17 taps, index clamp; central differences, one-sided at the ends)
//     gavs = gaussian(axis * angle / dt of qnormalize(gq[t+1] * inv(gq[t])))     (identity at the last frame)
//     dvs  = axis * angle / dt of qnormalize(inv(lq[t]) * lq[t+1]), bodies 1..23  (the last frame repeats the one before)
// with angle = 2 atan2(|xyz|, w): on a unit quaternion with w >= 0 the host's arccos(2 w^2 - 1), and well conditioned in float32
// near angle 0 where arccos is not.
//
// Work item = (clip, tile of MOTION_TILE frames); a workgroup of 256 lanes walks the items with a stride of the grid size, so the
// result does not depend on the grid.  Per item, with the 9-frame halo (8 filter taps + 1 for the gradient) on both sides:
//   1. one (frame, body) per lane over the tile and its halo: the body's translation by walking its ancestors root first -- the
//      order the host adds them in -- into LDS, and the unfiltered angular velocity into LDS; the lanes of the tile's own frames also
//      write grs, lrs, gts and dvs (consecutive lanes, consecutive floats);
//   2. one (frame, body) per lane over the tile: the two 17-tap filters from LDS, the gradient formed on the way.
// A frame index is clamped to the clip before it is turned into an LDS slot, so any T >= 2 takes the same path.
// Plain fp32 arithmetic in a fixed order (the unit is built with -ffp-contract=off), no atomics, no cross-lane operations:
// tests/emu/emu_motion.cpp runs the same source on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace emloco {

constexpr int MOTION_NB = 24, MOTION_TAPS = 17, MOTION_RADIUS = 8, MOTION_HALO = MOTION_RADIUS + 1;
constexpr int MOTION_TILE = 64, MOTION_WIN = MOTION_TILE + 2 * MOTION_HALO, MOTION_THREADS = 256;
constexpr int MOTION_MAX_GRID = 4096;

// the skeleton's topology and the filter travel by value with the launch: the host validates them, nothing is copied or synchronised
struct MotionArgs {
    int n_clips, n_skel, max_tiles;
    int parent[MOTION_NB];
    float taps[MOTION_TAPS];
};

// Fills `a` from the caller's host arrays; nullptr, or what is wrong with them.  `n_frames`, `skel_id`, `frame_start` are the HOST
// copies of the per-clip arrays: every row a clip writes must lie inside the F rows of the outputs.
inline const char *motion_pack(int n_clips, int n_skel, long long F, const long long *frame_start, const int32_t *n_frames,
                               const int32_t *skel_id, const int32_t *parent, const float *taps, MotionArgs *a) {
    if (!frame_start || !n_frames || !skel_id || !parent || !taps) return "null host array";
    if (n_clips < 1 || n_skel < 1 || F < 2) return "n_clips, n_skel must be at least 1, the frame count at least 2";
    int max_t = 0;
    for (int c = 0; c < n_clips; ++c) {
        if (n_frames[c] < 2) return "a clip needs at least 2 frames";
        if (skel_id[c] < 0 || skel_id[c] >= n_skel) return "skel_id out of range";
        if (frame_start[c] < 0 || frame_start[c] > F - n_frames[c]) return "a clip's frames lie outside the arrays";
        max_t = n_frames[c] > max_t ? n_frames[c] : max_t;
    }
    for (int b = 0; b < MOTION_NB; ++b)
        if (b == 0 ? parent[b] != -1 : (parent[b] < 0 || parent[b] >= b)) return "parent: -1 for body 0, below the child's index otherwise";
    for (int k = 0; k < MOTION_TAPS; ++k)
        if (!(taps[k] - taps[k] == 0.0f)) return "filter taps must be finite";
    a->n_clips = n_clips; a->n_skel = n_skel;
    a->max_tiles = (max_t + MOTION_TILE - 1) / MOTION_TILE;
    if ((long long)a->max_tiles * n_clips > 0x7fffffffLL) return "too many tiles";
    for (int b = 0; b < MOTION_NB; ++b) a->parent[b] = parent[b];
    for (int k = 0; k < MOTION_TAPS; ++k) a->taps[k] = taps[k];
    return nullptr;
}

inline unsigned motion_default_grid(const MotionArgs &a) {
    const long long items = (long long)a.max_tiles * a.n_clips;
    return (unsigned)(items < MOTION_MAX_GRID ? items : MOTION_MAX_GRID);
}

struct MQuat { float x, y, z, w; };

__device__ __forceinline__ MQuat mq_load(const float *p) { return MQuat{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ MQuat mq_mul(const MQuat a, const MQuat b) {          // motion_lib_smpl.py _qmul, term for term
    return MQuat{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
                 a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
__device__ __forceinline__ MQuat mq_inv(const MQuat q) { return MQuat{-q.x, -q.y, -q.z, q.w}; }
__device__ __forceinline__ MQuat mq_normalize(MQuat q) {                         // real part non-negative, unit length
    if (q.w < 0.0f) q = MQuat{-q.x, -q.y, -q.z, -q.w};
    const float n = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-9f);
    return MQuat{q.x / n, q.y / n, q.z / n, q.w / n};
}
// q (v, 0) q^-1
__device__ __forceinline__ void mq_rotate(const MQuat q, const float vx, const float vy, const float vz, float *o) {
    const MQuat r = mq_mul(mq_mul(q, MQuat{vx, vy, vz, 0.0f}), mq_inv(q));
    o[0] = r.x; o[1] = r.y; o[2] = r.z;
}
// axis * angle / dt of a normalised quaternion with a non-negative real part; exactly zero for the identity
__device__ __forceinline__ void mq_rotvec_rate(const MQuat q, const float dt, float *o) {
    const float s = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z);
    const float angle = 2.0f * atan2f(s, q.w);
    const float d = fmaxf(s, 1e-9f);
    o[0] = q.x / d * angle / dt; o[1] = q.y / d * angle / dt; o[2] = q.z / d * angle / dt;
}

__global__ __launch_bounds__(MOTION_THREADS) void motion_build_kernel(
    const MotionArgs a, const float *__restrict__ quat_global, const float *__restrict__ root_trans,
    const long long *__restrict__ frame_start, const int32_t *__restrict__ n_frames, const float *__restrict__ fps,
    const int32_t *__restrict__ skel_id, const float *__restrict__ local_translation, float *__restrict__ gts, float *__restrict__ grs,
    float *__restrict__ lrs, float *__restrict__ gvs, float *__restrict__ gavs, float *__restrict__ dvs) {
    constexpr int NB = MOTION_NB, ROW = NB * 3;
    __shared__ float sh_gp[MOTION_WIN * ROW];                  // slot s = frame t0 - 9 + s
    __shared__ float sh_w[(MOTION_WIN - 2) * ROW];             // slot s = frame t0 - 8 + s: unfiltered angular velocity
    __shared__ float sh_lt[ROW];
    __shared__ unsigned char sh_chain[NB * NB];                // body b: its ancestors and itself below the root, root side first
    __shared__ int sh_depth[NB];

    const int tid = (int)threadIdx.x;
    if (tid < NB) {
        int d = 0;
        for (int x = tid; a.parent[x] >= 0; x = a.parent[x]) ++d;
        sh_depth[tid] = d;
        for (int x = tid, k = d - 1; k >= 0; x = a.parent[x], --k) sh_chain[tid * NB + k] = (unsigned char)x;
    }

    const long long items = (long long)a.n_clips * a.max_tiles;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int c = (int)(item / a.max_tiles);
        const int t0 = (int)(item - (long long)c * a.max_tiles) * MOTION_TILE;
        const int T = n_frames[c];
        if (t0 >= T) continue;                                 // (the whole workgroup: c and t0 are uniform)
        const long long base = frame_start[c];
        const float dt = 1.0f / fps[c];
        const int nt = T - t0 < MOTION_TILE ? T - t0 : MOTION_TILE;
        const float *gq = quat_global + base * (NB * 4);
        const float *lt = local_translation + (long long)skel_id[c] * ROW;

        __syncthreads();                                       // the previous item's filters have read sh_gp / sh_w; sh_chain is written
        if (tid < ROW) sh_lt[tid] = lt[tid];
        __syncthreads();

        // 1. translations and angular velocities of the tile and its halo; the per-frame outputs of the tile's own frames
        for (int e = tid; e < MOTION_WIN * NB; e += MOTION_THREADS) {
            const int s = e / NB, b = e - s * NB;
            const int f = t0 - MOTION_HALO + s;
            if (f < 0 || f >= T) continue;
            const float *qf = gq + (long long)f * (NB * 4);
            float p[3] = {root_trans[(base + f) * 3 + 0], root_trans[(base + f) * 3 + 1], root_trans[(base + f) * 3 + 2]};
            const int depth = sh_depth[b];
            for (int k = 0; k < depth; ++k) {
                const int x = sh_chain[b * NB + k];
                float o[3];
                mq_rotate(mq_load(qf + a.parent[x] * 4), sh_lt[x * 3 + 0], sh_lt[x * 3 + 1], sh_lt[x * 3 + 2], o);
                p[0] = p[0] + o[0]; p[1] = p[1] + o[1]; p[2] = p[2] + o[2];
            }
            sh_gp[s * ROW + b * 3 + 0] = p[0]; sh_gp[s * ROW + b * 3 + 1] = p[1]; sh_gp[s * ROW + b * 3 + 2] = p[2];
            const MQuat q = mq_load(qf + b * 4);
            if (s >= 1 && s < MOTION_WIN - 1) {
                float w[3] = {0.0f, 0.0f, 0.0f};
                if (f < T - 1) mq_rotvec_rate(mq_normalize(mq_mul(mq_load(qf + NB * 4 + b * 4), mq_inv(q))), dt, w);
                float *dst = sh_w + (s - 1) * ROW + b * 3;
                dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2];
            }
            if (f >= t0 && f < t0 + nt) {
                const long long row = base + f;
                float *o4 = grs + (row * NB + b) * 4;
                o4[0] = q.x; o4[1] = q.y; o4[2] = q.z; o4[3] = q.w;
                float *o3 = gts + (row * NB + b) * 3;
                o3[0] = p[0]; o3[1] = p[1]; o3[2] = p[2];
                const int pb = a.parent[b];
                const MQuat lq = pb < 0 ? q : mq_normalize(mq_mul(mq_inv(mq_load(qf + pb * 4)), q));
                o4 = lrs + (row * NB + b) * 4;
                o4[0] = lq.x; o4[1] = lq.y; o4[2] = lq.z; o4[3] = lq.w;
                if (b > 0) {                                   // the joint's velocity between frames f0 and f0 + 1, f0 = min(f, T - 2)
                    const int f0 = f < T - 1 ? f : T - 2;
                    const float *q0 = gq + (long long)f0 * (NB * 4), *q1 = q0 + NB * 4;
                    const MQuat l0 = mq_normalize(mq_mul(mq_inv(mq_load(q0 + pb * 4)), mq_load(q0 + b * 4)));
                    const MQuat l1 = mq_normalize(mq_mul(mq_inv(mq_load(q1 + pb * 4)), mq_load(q1 + b * 4)));
                    float v[3];
                    mq_rotvec_rate(mq_normalize(mq_mul(mq_inv(l0), l1)), dt, v);
                    o3 = dvs + row * (ROW - 3) + (b - 1) * 3;
                    o3[0] = v[0]; o3[1] = v[1]; o3[2] = v[2];
                }
            }
        }
        __syncthreads();

        // 2. the two filters over the tile's frames
        for (int e = tid; e < nt * ROW; e += MOTION_THREADS) {
            const int j = e / ROW, r = e - j * ROW;            // r = body * 3 + coordinate
            const int f = t0 + j;
            float v = 0.0f, w = 0.0f;
            for (int k = 0; k < MOTION_TAPS; ++k) {
                int u = f + k - MOTION_RADIUS;
                u = u < 0 ? 0 : (u > T - 1 ? T - 1 : u);
                const int lo = u > 0 ? u - 1 : 0, hi = u < T - 1 ? u + 1 : T - 1;
                const float d = sh_gp[(hi - t0 + MOTION_HALO) * ROW + r] - sh_gp[(lo - t0 + MOTION_HALO) * ROW + r];
                const float g = hi - lo == 2 ? d / 2.0f : d;
                v = v + a.taps[k] * g;
                w = w + a.taps[k] * sh_w[(u - t0 + MOTION_RADIUS) * ROW + r];
            }
            gvs[(base + f) * ROW + r] = v / dt;
            gavs[(base + f) * ROW + r] = w;
        }
    }
}

}  // namespace emloco
