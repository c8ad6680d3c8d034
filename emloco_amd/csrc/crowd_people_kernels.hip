// crowd_people_kernels.hip -- the group observation (include/emloco_task.h: EmlocoCrowdPeople): the ten selected joints and the root
// velocity of the five nearest members of an env's group, in the env's heading frame.  The reference does this with a
// [groups, gs, gs] distance tensor, a topk and three gathers (humanoid_pedestrain_terrain.py:1613-1666).  Included by crowd_capi.hip,
// which is built without fused-multiply-add contraction: plain fp32 in the order the header states, so the CPU emulation gives the
// same bytes.
//   crowd_people_roots_kernel   one thread per env: the root position to a packed [E][4] array
//   crowd_people_kernel         one wave per listed env: lane l walks members l, l + 64, ... of the group and keeps its five lowest keys
//                               (distance bits << 32 | member) sorted in registers; five wave minima pick the neighbours (the winning
//                               lane drops its head); lane t < 55 then forms triple t, and the 165 + 165 values leave with lanes across
//                               columns (shuffles, no LDS).
// Distances are non-negative, so their bit patterns order as unsigned integers; the member index makes every key unique, so the
// result does not depend on the visiting order.  No atomics, no LDS, no barrier.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_math.h"
#include "../../include/emloco_task.h"

namespace emloco {

constexpr int kPeopleThreads = 256;
constexpr int kPeopleWaves = kPeopleThreads / 64;
constexpr int kPeopleBodies = 24;
constexpr int kPeopleTriples = EMLOCO_PEOPLE_TOPK * (EMLOCO_PEOPLE_JOINTS + 1);
constexpr unsigned long long kPeopleNoKey = ~0ull;
constexpr unsigned kPeopleInfBits = 0x7f800000u;

static_assert(EMLOCO_PEOPLE_TOPK == 5, "the selection keeps five keys per lane in named registers");
static_assert(kPeopleTriples * 3 == EMLOCO_PEOPLE_WIDTH && kPeopleTriples <= 64, "one lane per triple");

__global__ __launch_bounds__(256) void crowd_people_roots_kernel(const EmlocoCrowdPeople p) {
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (e >= p.n_env) return;
    const float *root = p.rb_state + (long)e * kPeopleBodies * 13;
    float *out = p.roots_ws + (long)e * 4;
    out[0] = root[0]; out[1] = root[1]; out[2] = root[2]; out[3] = 0.0f;
}

__device__ __forceinline__ int people_body(int j) {
    constexpr int bodies[EMLOCO_PEOPLE_JOINTS] = EMLOCO_PEOPLE_BODIES;
    int b = bodies[0];
#pragma unroll
    for (int k = 1; k < EMLOCO_PEOPLE_JOINTS; ++k) b = j == k ? bodies[k] : b;
    return b;
}

__device__ __forceinline__ unsigned long long people_min(unsigned long long a, unsigned long long b) { return b < a ? b : a; }

__global__ __launch_bounds__(kPeopleThreads) void crowd_people_kernel(const EmlocoCrowdPeople p, const int32_t *env_ids, int n) {
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int gs = p.group_size;
    for (int row = (int)blockIdx.x * kPeopleWaves + wave; row < n; row += (int)gridDim.x * kPeopleWaves) {
        const int env = __builtin_amdgcn_readfirstlane(env_ids ? env_ids[row] : row);
        if (env < 0 || env >= p.n_env) continue;                   // (wave-uniform) padding entries of a compacted list
        const int g0 = (env / gs) * gs;
        const float *own = p.rb_state + (long)env * kPeopleBodies * 13;
        const float rx = own[0], ry = own[1], rz = own[2];
        // the lane's five lowest keys, ascending
        unsigned long long k0 = kPeopleNoKey, k1 = kPeopleNoKey, k2 = kPeopleNoKey, k3 = kPeopleNoKey, k4 = kPeopleNoKey;
        for (int ml = lane; ml < gs; ml += 64) {
            if (g0 + ml == env) continue;
            const float *mr = p.roots_ws + (long)(g0 + ml) * 4;
            const float dx = mr[0] - rx, dy = mr[1] - ry, dz = mr[2] - rz;
            const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
            unsigned bits = __float_as_uint(dist);
            if (!(dist < __uint_as_float(kPeopleInfBits))) bits = kPeopleInfBits;      // NaN and +inf alike
            unsigned long long x = ((unsigned long long)bits << 32) | (unsigned)ml, t;
            if (x < k0) { t = k0; k0 = x; x = t; }
            if (x < k1) { t = k1; k1 = x; x = t; }
            if (x < k2) { t = k2; k2 = x; x = t; }
            if (x < k3) { t = k3; k3 = x; x = t; }
            if (x < k4) { k4 = x; }
        }
        int sel0 = 0, sel1 = 0, sel2 = 0, sel3 = 0, sel4 = 0;      // env ids of the neighbours
        unsigned far = 0u;                                         // bit k: neighbour k is masked
#pragma unroll
        for (int k = 0; k < EMLOCO_PEOPLE_TOPK; ++k) {
            unsigned long long best = k0;
            for (int off = 32; off > 0; off >>= 1) best = people_min(best, __shfl_xor(best, off));
            if (k0 == best) { k0 = k1; k1 = k2; k2 = k3; k3 = k4; k4 = kPeopleNoKey; }     // (keys are unique: one lane)
            int ml = (int)(unsigned)(best & 0xffffffffull);
            ml = ml < gs ? ml : gs - 1;                            // (group_size >= 6: a real key always wins; never out of the group)
            const int m = g0 + ml;
            if (__uint_as_float((unsigned)(best >> 32)) > EMLOCO_PEOPLE_FAR) far |= 1u << k;
            if (k == 0) sel0 = m; else if (k == 1) sel1 = m; else if (k == 2) sel2 = m; else if (k == 3) sel3 = m; else sel4 = m;
        }
        if (p.neighbours && lane < EMLOCO_PEOPLE_TOPK)
            p.neighbours[(long)env * EMLOCO_PEOPLE_TOPK + lane] = lane == 0 ? sel0 : lane == 1 ? sel1 : lane == 2 ? sel2 : lane == 3 ? sel3 : sel4;
        // lane t < 55: triple t -- t < 50: joint t % 10 of neighbour t / 10; else the root velocity of neighbour t - 50
        float hinv[4];
        ref_quat_about_z(-ref_calc_heading(own + 3), hinv);
        float o[3] = {0.0f, 0.0f, 0.0f};
        if (lane < kPeopleTriples) {
            const bool is_vel = lane >= EMLOCO_PEOPLE_TOPK * EMLOCO_PEOPLE_JOINTS;
            const int k = is_vel ? lane - EMLOCO_PEOPLE_TOPK * EMLOCO_PEOPLE_JOINTS : lane / EMLOCO_PEOPLE_JOINTS;
            const int j = is_vel ? 0 : lane - k * EMLOCO_PEOPLE_JOINTS;
            const int m = k == 0 ? sel0 : k == 1 ? sel1 : k == 2 ? sel2 : k == 3 ? sel3 : sel4;
            if (!((far >> k) & 1u)) {
                const float *src = p.rb_state + ((long)m * kPeopleBodies + people_body(j)) * 13 + (is_vel ? 7 : 0);
                float v[3] = {src[0], src[1], src[2]};
                if (!is_vel) { v[0] = v[0] - rx; v[1] = v[1] - ry; v[2] = v[2] - rz; }
                ref_quat_rotate(hinv, v, o);
            }
        }
        float *obs = p.obs + (long)env * p.obs_stride + p.col, *fobs = p.flip_obs + (long)env * p.obs_stride + p.col;
#pragma unroll
        for (int c0 = 0; c0 < EMLOCO_PEOPLE_WIDTH; c0 += 64) {     // (every lane makes every trip: the shuffles are wave-wide)
            const int c = c0 + lane, t = c / 3, comp = c - t * 3;
            const float a = __shfl(o[0], t), b = __shfl(o[1], t), d = __shfl(o[2], t);
            if (c < EMLOCO_PEOPLE_WIDTH) {
                const float v = comp == 0 ? a : comp == 1 ? b : d;
                obs[c] = v;
                fobs[c] = comp == 1 ? -v : v;
            }
        }
    }
}

// what emloco_task_crowd_people refuses, by name (NULL: complete); host code, shared with the CPU emulation of the launch
inline const char *crowd_people_refusal(const EmlocoCrowdPeople *p, int n) {
    if (!p) return "null structure";
    if (!p->rb_state) return "null rb_state";
    if (!p->roots_ws) return "null roots_ws";
    if (!p->obs) return "null obs";
    if (!p->flip_obs) return "null flip_obs";
    if (p->group_size < EMLOCO_PEOPLE_TOPK + 1) return "group_size < 6";
    if (p->n_env < 1 || p->n_env % p->group_size != 0) return "n_env is not a multiple of group_size";
    if (p->col < 0 || (long)p->col + EMLOCO_PEOPLE_WIDTH > (long)p->obs_stride) return "col + 165 > obs_stride";
    if (n < 0) return "n < 0";
    return nullptr;
}

}  // namespace emloco
