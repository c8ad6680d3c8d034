// crowd_kernels.hip -- the crowd-aware terrain sensor (include/emloco_task.h: EmlocoCrowdBufs): the members of a group stamp the map
// cells under their root points into the group's owner map, then every env's probes read height (channel 0) and, with three
// channels, the relative velocity of the member standing on the cell.  The reference does this with a Python loop over groups and a
// clone of the whole height field per group (humanoid_pedestrain_terrain.py:1221-1297); here the cost of a step is the stamps and
// the probes, whatever the map's area.  Arithmetic: the ref_* helpers of dev_math.h / task_device.h term by term, -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include "task_device.h"

namespace emloco {

constexpr int kCrowdThreads = 256;
constexpr int kCrowdWaves = kCrowdThreads / 64;
constexpr int kCrowdRootPoints = EMLOCO_CROWD_ROOT_X * EMLOCO_CROWD_ROOT_Y;

// One workgroup per env (grid-stride): thread p < 200 is root point p = 20 i + j (:685-702), rotated by the root's heading and added to
// the root position (:793-796).  atomicMax of (tag | member * 200 + p + 1): the current tag beats every older word, and among the
// words of this call the highest index wins -- the last writer of the reference's serial indexed assignment (:1247,1262).
__global__ __launch_bounds__(kCrowdThreads) void crowd_stamp_kernel(const EmlocoCrowdBufs c) {
    __shared__ float sh_q[4];
    const int tid = (int)threadIdx.x;
    const long cells = (long)c.hf_rows * c.hf_cols;
    for (int env = (int)blockIdx.x; env < c.n_env; env += (int)gridDim.x) {
        const float *root = c.rb_state + (long)env * TNB * 13;
        if (tid == 0) {
            float q[4];
            ref_quat_about_z(ref_calc_heading(root + 3), q);
            for (int k = 0; k < 4; ++k) sh_q[k] = q[k];
        }
        __syncthreads();
        if (tid < kCrowdRootPoints) {
            const int i = tid / EMLOCO_CROWD_ROOT_Y, j = tid - i * EMLOCO_CROWD_ROOT_Y;
            const float pt[3] = {c.root_x[i], c.root_y[j], 0.0f};
            float rr[3];
            ref_quat_apply(sh_q, pt, rr);
            int px, py;
            map_index(c.hf_rows, c.hf_cols, rr[0] + root[0], rr[1] + root[1], c.hscale, &px, &py);     // clamped: NaN -> (0, 0)
            const int group = env / c.group_size, member = env - group * c.group_size;
            const unsigned word = (c.tag << c.tag_shift) | (unsigned)(member * kCrowdRootPoints + tid + 1);
            atomicMax(c.owner + (long)group * cells + (long)px * c.hf_cols + py, word);
        }
        __syncthreads();
    }
}

// One workgroup per listed env (grid-stride), one wave per probe row i, lane = j.  The rows are staged in LDS and leave as
// contiguous runs: row i of the block is res * channels floats in obs and, with j reversed, the same run in flip_obs.
__global__ __launch_bounds__(kCrowdThreads) void crowd_gather_kernel(const EmlocoCrowdBufs c, const int32_t *env_ids, int n) {
    __shared__ float sh_quat[2][4];                // [0] inverse heading of the root, [1] heading of the head
    __shared__ float sh_center[12];
    __shared__ float sh_row[kCrowdWaves][2][EMLOCO_CROWD_MAX_RES * 3];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int res = c.res, C = c.channels;
    const long cells = (long)c.hf_rows * c.hf_cols;
    const unsigned idx_mask = (1u << c.tag_shift) - 1u;
    for (int b = (int)blockIdx.x; b < n; b += (int)gridDim.x) {
        const int env = env_ids ? env_ids[b] : b;
        if (env < 0 || env >= c.n_env) continue;                   // (block-uniform) padding entries of a compacted list
        const float *root = c.rb_state + (long)env * TNB * 13;
        const float *head = root + c.head_body * 13;
        if (tid < 2) {                                             // the two heading quaternions in one pass (post_physics_env does the same)
            const float h = ref_calc_heading((tid == 1 ? head : root) + 3);
            float q[4];
            ref_quat_about_z(tid == 1 ? h : -h, q);
            for (int k = 0; k < 4; ++k) sh_quat[tid][k] = q[k];
        } else if (tid >= 64 && tid < 64 + 9) {                    // centre probes on the unstamped field (:427-429, :732-759)
            float wx, wy;
            center_probe(root, root + 3, tid - 64, &wx, &wy);
            sh_center[tid - 64] = sample_height(c.heightfield, c.hf_rows, c.hf_cols, wx, wy, c.hscale, c.vscale);
        }
        float *obs = c.obs + (long)env * c.dst_width, *fobs = c.flip_obs + (long)env * c.dst_width;
        for (int k = tid; k < c.n_copy; k += kCrowdThreads) {
            obs[k] = c.src_obs[(long)env * c.src_width + k];
            fobs[k] = c.src_flip_obs[(long)env * c.src_width + k];
        }
        __syncthreads();
        const float cmean = mean9(sh_center);
        const float *hinv = sh_quat[0], *hq = sh_quat[1];
        const float own_v[3] = {root[7], root[8], root[9]};
        const int group = env / c.group_size;
        const unsigned *owner = c.stamps ? c.owner + (long)group * cells : nullptr;
        for (int i0 = 0; i0 < res; i0 += kCrowdWaves) {            // (every thread makes every trip: the barriers are block-wide)
            const int i = i0 + wave;
            if (i < res && lane < res) {
                const float pt[3] = {c.probe_xy[i], c.probe_xy[lane], 0.0f};
                float rr[3];
                ref_quat_apply(hq, pt, rr);
                int px, py;
                map_index(c.hf_rows, c.hf_cols, rr[0] + head[0], rr[1] + head[1], c.hscale, &px, &py);
                const long c1 = (long)px * c.hf_cols + py, c2 = c1 + c.hf_cols + 1;
                int16_t h1 = c.heightfield[c1], h2 = c.heightfield[c2];
                float cell_v[3] = {0.0f, 0.0f, 0.0f};
                if (owner) {
                    const unsigned w1 = owner[c1], w2 = owner[c2];
                    if ((w1 >> c.tag_shift) == c.tag) {
                        h1 = (int16_t)(h1 + c.stamp_units);       // torch's int16 addition: wraps
                        if (C == 3) {
                            int member = (int)((w1 & idx_mask) - 1u) / kCrowdRootPoints;
                            member = member < 0 ? 0 : (member >= c.group_size ? c.group_size - 1 : member);
                            const float *ov = c.rb_state + (long)(group * c.group_size + member) * TNB * 13 + 7;
                            cell_v[0] = ov[0]; cell_v[1] = ov[1]; cell_v[2] = ov[2];
                        }
                    }
                    if ((w2 >> c.tag_shift) == c.tag) h2 = (int16_t)(h2 + c.stamp_units);
                }
                const int16_t hm = h1 < h2 ? h1 : h2;
                float out[3];
                out[0] = cmean - (float)hm * c.vscale;
                if (C == 3) {
                    float rel[3], ego[3];
                    if (owner) {                                   // :1267-1274: (map - own), then into the heading frame
                        for (int k = 0; k < 3; ++k) rel[k] = cell_v[k] - own_v[k];
                        ref_quat_rotate(hinv, rel, ego);
                        out[1] = ego[0]; out[2] = ego[1];
                    } else {                                       // :1290-1295: 0 - (own in the heading frame)
                        ref_quat_rotate(hinv, own_v, ego);
                        out[1] = 0.0f - ego[0]; out[2] = 0.0f - ego[1];
                    }
                }
                for (int k = 0; k < C; ++k) {
                    float v = out[k];
                    if (v < -3.0f) v = -3.0f;
                    if (v > 3.0f) v = 3.0f;
                    v *= 5.0f;
                    sh_row[wave][0][lane * C + k] = v;
                    sh_row[wave][1][(res - 1 - lane) * C + k] = v;
                }
            }
            __syncthreads();
            if (i < res) {
                const long at = (long)c.n_copy + (long)i * res * C;
                for (int k = lane; k < res * C; k += 64) { obs[at + k] = sh_row[wave][0][k]; fobs[at + k] = sh_row[wave][1][k]; }
            }
            __syncthreads();
        }
    }
}

// what emloco_task_crowd_sensor refuses, by name (NULL: complete); host code, shared with the CPU emulation of the launch
inline const char *crowd_refusal(const EmlocoCrowdBufs *c, int n) {
    if (!c) return "null structure";
    if (c->n_env <= 0) return "n_env <= 0";
    if (c->group_size < 1 || c->n_env % c->group_size != 0) return "n_env is not a multiple of group_size";
    if (c->res < 1 || c->res > EMLOCO_CROWD_MAX_RES) return "res outside 1 .. 64";
    if (c->channels != 1 && c->channels != 3) return "channels 1 | 3 required";
    if (c->stamps < 0 || c->stamps > 1) return "stamps 0 | 1 required";
    if (c->hf_rows < 2 || c->hf_cols < 2) return "height map smaller than 2 x 2";
    if (c->head_body < 0 || c->head_body >= TNB) return "head_body outside 0 .. 23";
    if (c->n_copy < 0 || c->n_copy > c->src_width) return "n_copy outside 0 .. src_width";
    if ((long)c->dst_width < (long)c->n_copy + (long)c->channels * c->res * c->res) return "dst_width below n_copy + channels * res * res";
    if (n < 0) return "n < 0";
    if (!c->rb_state) return "null rb_state";
    if (!c->heightfield) return "null heightfield";
    if (!c->probe_xy) return "null probe_xy";
    if (!c->obs) return "null obs";
    if (!c->flip_obs) return "null flip_obs";
    if (c->n_copy > 0 && !c->src_obs) return "null src_obs";
    if (c->n_copy > 0 && !c->src_flip_obs) return "null src_flip_obs";
    if (c->stamps) {
        if (!c->root_x) return "null root_x";
        if (!c->root_y) return "null root_y";
        if (!c->owner) return "null owner";
        if (c->tag_shift < 1 || c->tag_shift > 30 || (long)c->group_size * kCrowdRootPoints >= (1l << c->tag_shift))
            return "tag_shift: group_size * 200 < 2^tag_shift <= 2^30 required";
        if (c->tag < 1u || c->tag >= (1u << (32 - c->tag_shift))) return "tag outside 1 .. 2^(32 - tag_shift) - 1";
    }
    return nullptr;
}

}  // namespace emloco
