// crowd_spawn_kernels.hip -- the crowd spawn (include/emloco_task.h: EmlocoCrowdSpawn): at a reset every listed member of a group
// goes to a random admissible spot of the group's square, at least min_dist from every member standing at that moment.  Included by
// crowd_capi.hip, which is built without fused-multiply-add contraction: plain fp32 in the order the header states, so the CPU
// emulation and a numpy float32 restatement give the same bytes.
//   crowd_spawn_mark_kernel    one thread per list position: the lowest position of every listed env into mark_ws (integer atomicMin
//                              on the unsigned view, where the resting value -1 is the largest)
//   crowd_spawn_place_kernel   one workgroup per group, one wave per candidate.  The group's root xy is staged once in LDS; a member
//                              that is listed, or whose root is not finite, is staged as NaN, so "standing" is "the squared distance
//                              compares".  The listed members are compacted in ascending order (ballots, wave 0).  Per placed member
//                              wave k evaluates candidate k: admissibility wave-uniform, the minimum over the members with lanes
//                              across members and five shuffles; lane 0 posts it to LDS; ONE barrier; every wave then reads the
//                              tries <= 8 results, comes to the same decision and publishes the new spot to LDS itself (equal values
//                              from every wave), so the next round needs no second barrier.  The result slots alternate between two
//                              sets: a wave two rounds ahead cannot exist, the barrier in between holds it.
// A round is a dependent step: a full first reset of a 512-group is 512 rounds in one workgroup.  No scratch, no float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/emloco_task.h"

namespace emloco {

constexpr int kSpawnMarkThreads = 256;
constexpr unsigned kSpawnInfBits = 0x7f800000u;

__device__ __forceinline__ bool spawn_finite(float v) { return (__float_as_uint(v) & kSpawnInfBits) != kSpawnInfBits; }

__global__ __launch_bounds__(kSpawnMarkThreads) void crowd_spawn_mark_kernel(const EmlocoCrowdSpawn s, const int32_t *env_ids, int rows) {
    const int i = (int)blockIdx.x * kSpawnMarkThreads + (int)threadIdx.x;
    if (i >= rows) return;
    const int e = env_ids ? env_ids[i] : i;
    if (e < 0 || e >= s.n_env) return;
    atomicMin((unsigned *)s.mark_ws + e, (unsigned)i);
}

// min over the staged members other than `self` of (dx dx) + (dy dy) to (cx, cy), the whole wave's; a NaN-staged member never compares
// (`self` is named because a faster wave may already have published its spot when the centre's clearance is taken)
__device__ __forceinline__ float spawn_clearance2(const float *xs, const float *ys, int gs, int lane, int self, float cx, float cy) {
    float best = __uint_as_float(kSpawnInfBits);
    for (int j = lane; j < gs; j += 64) {
        const float dx = xs[j] - cx, dy = ys[j] - cy;
        const float d2 = (dx * dx) + (dy * dy);
        best = (j != self && d2 < best) ? d2 : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(best, off);
        best = o < best ? o : best;
    }
    return best;
}

__device__ __forceinline__ bool spawn_admissible(const EmlocoCrowdSpawn &s, float cx, float cy) {
    if (!(s.min_x <= cx && cx <= s.max_x && s.min_y <= cy && cy <= s.max_y)) return false;
    const float qx = cx / s.hscale, qy = cy / s.hscale;
    // (int)q lies in [0, rows) exactly when -1 < q < rows; tested on the quotient, so no out-of-range conversion is ever made
    if (!(qx > -1.0f && qx < (float)s.rows && qy > -1.0f && qy < (float)s.cols)) return false;
    return s.walkable[(long)(int)qx * s.cols + (int)qy] == 0;
}

__global__ __launch_bounds__(EMLOCO_SPAWN_MAX_TRIES * 64) void crowd_spawn_place_kernel(const EmlocoCrowdSpawn s, const float *u, int rows) {
    __shared__ float xs[EMLOCO_SPAWN_MAX_GROUP], ys[EMLOCO_SPAWN_MAX_GROUP];
    __shared__ int mark[EMLOCO_SPAWN_MAX_GROUP], listed[EMLOCO_SPAWN_MAX_GROUP];
    __shared__ float res_c2[2][EMLOCO_SPAWN_MAX_TRIES], res_x[2][EMLOCO_SPAWN_MAX_TRIES], res_y[2][EMLOCO_SPAWN_MAX_TRIES];
    __shared__ int res_ok[2][EMLOCO_SPAWN_MAX_TRIES];
    __shared__ int n_listed;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int gs = s.group_size, tries = s.tries, g = (int)blockIdx.x, g0 = g * gs;
    const float nan = __uint_as_float(0x7fc00000u);
    for (int m = tid; m < gs; m += tries * 64) {
        const int mk_in = s.mark_ws[g0 + m];
        const int mk = mk_in < rows ? mk_in : -1;                  // (a mark this call did not write names no row of u: not listed)
        const float *root = s.roots + (long)(g0 + m) * s.root_stride;
        const float x = root[0], y = root[1];
        const bool stands = mk < 0 && spawn_finite(x) && spawn_finite(y);
        mark[m] = mk;
        xs[m] = stands ? x : nan;
        ys[m] = stands ? y : nan;
    }
    __syncthreads();
    if (wave == 0) {                                               // the listed members, ascending
        int count = 0;
        for (int base = 0; base < gs; base += 64) {                // (every lane makes every trip: the ballot is wave-wide)
            const int m = base + lane;
            const bool is = m < gs && mark[m] >= 0;
            const unsigned long long b = __ballot(is);
            if (is) listed[count + __popcll(b & ((1ull << lane) - 1ull))] = m;
            count += __popcll(b);
        }
        if (lane == 0) n_listed = count;
    }
    __syncthreads();
    const int count = n_listed;
    if (count == 0) return;
    const float cgx = s.centres[2 * g], cgy = s.centres[2 * g + 1];
    const float md2 = s.min_dist * s.min_dist;
    const float *urow = u + ((long)mark[listed[0]] * tries + wave) * 2;
    float u0 = urow[0], u1 = urow[1];
    for (int r = 0; r < count; ++r) {
        const int m = listed[r], set = r & 1;
        const float tx = 2.0f * u0 - 1.0f, ty = 2.0f * u1 - 1.0f;
        const float ex = s.extent * tx, ey = s.extent * ty;
        const float cx = cgx + ex, cy = cgy + ey;
        if (r + 1 < count) {                                       // the next round's uniforms, ahead of this round's barrier
            urow = u + ((long)mark[listed[r + 1]] * tries + wave) * 2;
            u0 = urow[0]; u1 = urow[1];
        }
        const bool ok = spawn_admissible(s, cx, cy);
        const float c2 = spawn_clearance2(xs, ys, gs, lane, m, cx, cy);
        if (lane == 0) { res_ok[set][wave] = ok; res_c2[set][wave] = c2; res_x[set][wave] = cx; res_y[set][wave] = cy; }
        __syncthreads();
        int pick = -1, fall = -1, flags = 0;
        float fall_c2 = -1.0f;
        for (int k = 0; k < tries; ++k) {
            if (!res_ok[set][k]) continue;
            const float v = res_c2[set][k];
            if (pick < 0 && v >= md2) pick = k;
            if (v > fall_c2) { fall_c2 = v; fall = k; }            // (v >= 0: the first admissible one always enters; ties keep the lower k)
        }
        if (pick < 0 && fall >= 0) { pick = fall; flags = EMLOCO_SPAWN_CROWDED; }
        float px, py, pc2;
        if (pick >= 0) {
            px = res_x[set][pick]; py = res_y[set][pick]; pc2 = res_c2[set][pick];
        } else {                                                   // (workgroup-uniform) no ground: the centre, its clearance by every wave alike
            px = cgx; py = cgy;
            pc2 = spawn_clearance2(xs, ys, gs, lane, m, cgx, cgy);
            flags = EMLOCO_SPAWN_NO_GROUND | (pc2 < md2 ? EMLOCO_SPAWN_CROWDED : 0);
        }
        if (lane == 0) {                                           // the member stands from here on, if its spot is finite
            const bool stands = spawn_finite(px) && spawn_finite(py);
            xs[m] = stands ? px : nan;
            ys[m] = stands ? py : nan;
        }
        if (tid == 0) {
            const int e = g0 + m;
            s.place_xy[2 * (long)e] = px;
            s.place_xy[2 * (long)e + 1] = py;
            EmlocoCrowdSpawnInfo out;
            out.clearance2 = pc2; out.tried = pick; out.flags = flags; out.order = r;
            s.info[e] = out;
            s.mark_ws[e] = -1;
        }
    }
}

// what emloco_task_crowd_spawn refuses, by name (NULL: complete); host code, shared with the CPU emulation of the launch
inline const char *crowd_spawn_refusal(const EmlocoCrowdSpawn *s, const int32_t *env_ids, int n, const float *u) {
    if (!s) return "null structure";
    if (!s->roots) return "null roots";
    if (!s->walkable) return "null walkable";
    if (!s->centres) return "null centres";
    if (!s->mark_ws) return "null mark_ws";
    if (!s->place_xy) return "null place_xy";
    if (!s->info) return "null info";
    if (s->group_size < 1) return "group_size < 1";
    if (s->group_size > EMLOCO_SPAWN_MAX_GROUP) return "group_size > 2048";
    if (s->n_env < 1 || s->n_env % s->group_size != 0) return "n_env is not a positive multiple of group_size";
    if (s->tries < 1 || s->tries > EMLOCO_SPAWN_MAX_TRIES) return "tries outside 1..8";
    if (s->root_stride < 2) return "root_stride < 2";
    if (s->rows < 1) return "rows < 1";
    if (s->cols < 1) return "cols < 1";
    if (!(s->hscale > 0.0f) || !(s->hscale < __builtin_inff())) return "hscale is not positive and finite";
    if (!(s->extent > 0.0f) || !(s->extent < __builtin_inff())) return "extent is not positive and finite";
    if (!(s->min_dist >= 0.0f) || !(s->min_dist < __builtin_inff())) return "min_dist is negative or not finite";
    if (!(s->min_x <= s->max_x)) return "empty box: min_x > max_x";
    if (!(s->min_y <= s->max_y)) return "empty box: min_y > max_y";
    if (n < 0) return "n < 0";
    if (!u && (env_ids ? n : s->n_env) > 0) return "null u";
    return nullptr;
}

}  // namespace emloco
