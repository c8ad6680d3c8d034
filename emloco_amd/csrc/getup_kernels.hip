// getup_kernels.hip -- the get-up task's resets for gfx950 (see include/emloco_task.h for the reference lines).
//
//   getup_split_kernel        one 1024-thread workgroup: frees the listed envs' pool slots, classifies every list entry
//                             (recovery | fall | normal), hands free pool slots to the fall entries in a keyed-permutation order and
//                             compacts the three lists -- ballot-free integer prefix sums (a thread owns a run of consecutive entries,
//                             shuffle scan inside a wave, LDS across the 16 waves, as compact_flags does), so the lists come out in
//                             the input's order whatever the list length
//   getup_copy_kernel         fall list: pool row -> simulator root / dof rows, warm-start impulses zeroed   (one wave per entry)
//   getup_finish_kernel       fall and recovery lists: flag buffers, contact forces, trajectory, LocoVal inputs -- the device
//                             functions of the reset chain (reset_kernels.hip), called, not restated
//   getup_amp_default_kernel  history rows 1..14 = the newest row
//   getup_flags_kernel        recovery counters and the flags they hold back, all envs
#include <hip/hip_runtime.h>
#include "dev_math.h"
#include "emloco_types.h"
#include "../../include/emloco_task.h"
#include "task_device.h"
// The reset chain's device functions come from reset_kernels.hip, which also defines that chain's kernels; they belong to the task unit
// (task_capi.hip).  In this unit they get names of their own, so that the two units link into one library.
#define reset_fill_rnd_kernel getup_unit_reset_fill_rnd_kernel
#define reset_sample_kernel getup_unit_reset_sample_kernel
#define reset_finish_kernel getup_unit_reset_finish_kernel
#define traj_reset_kernel getup_unit_traj_reset_kernel
#define reset_amp_history_kernel getup_unit_reset_amp_history_kernel
#include "reset_kernels.hip"
#undef reset_fill_rnd_kernel
#undef reset_sample_kernel
#undef reset_finish_kernel
#undef traj_reset_kernel
#undef reset_amp_history_kernel

namespace emloco {

#define GETUP_SPLIT_THREADS 1024

// exclusive prefix of `v` over the workgroup's threads in thread order, *total = the sum; sh: 16 ints of LDS.  Two barriers; the
// second one also frees `sh` for the next call.
__device__ __forceinline__ int getup_block_scan(int v, int *sh, int *total) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl(inc, lane - d < 0 ? 0 : lane - d);
        if (lane >= d) inc += up;
    }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    int off = inc - v, sum = 0;
    for (int w = 0; w < GETUP_SPLIT_THREADS / 64; ++w) { const int c = sh[w]; off += w < wave ? c : 0; sum += c; }
    __syncthreads();
    *total = sum;
    return off;
}

struct GetupSplitArgs {
    const int32_t *ids; int n;
    const float *rnd; unsigned seed_lo, seed_hi;
    float recovery_prob, fall_prob; int recovery_steps; unsigned slot_key;
    int32_t *normal, *fall, *recover, *fall_slot;
};

__device__ __forceinline__ bool getup_absent(int id, int n_env) { return id < 0 || id >= n_env; }

enum { GETUP_NORMAL = 0, GETUP_FALL = 1, GETUP_RECOVER = 2 };

// steps 2-4 of emloco_getup_split for list entry i (env = ids[i] >= 0); a fall entry may still turn normal for want of a slot
__device__ __forceinline__ int getup_classify(const EmlocoGetupBufs &g, const GetupSplitArgs &a, int i, int env) {
    const float u0 = a.rnd ? a.rnd[(long)i * 2] : reset_rnd_value(a.seed_lo, a.seed_hi, i, 0);
    const float u1 = a.rnd ? a.rnd[(long)i * 2 + 1] : reset_rnd_value(a.seed_lo, a.seed_hi, i, 1);
    if (u0 < a.recovery_prob && g.terminate_buf[env] == 1) return GETUP_RECOVER;
    return u1 < a.fall_prob ? GETUP_FALL : GETUP_NORMAL;
}

__global__ void __launch_bounds__(GETUP_SPLIT_THREADS)
getup_split_kernel(EmlocoGetupBufs g, GetupSplitArgs a) {
    __shared__ int sh[GETUP_SPLIT_THREADS / 64];
    const int tid = threadIdx.x, n = a.n, P = g.n_pool;
    const int per = (n + GETUP_SPLIT_THREADS - 1) / GETUP_SPLIT_THREADS, i0 = tid * per;             // this thread's run of list entries
    const int perp = (P + GETUP_SPLIT_THREADS - 1) / GETUP_SPLIT_THREADS, k0 = tid * perp;           // ... and of permutation positions

    // the list: the entries in front of the first negative id (an id beyond the env count ends it as well: nothing is indexed with it)
    int neg = 0, total;
    for (int k = 0; k < per; ++k) { const int i = i0 + k; if (i < n && getup_absent(a.ids[i], g.n_env)) ++neg; }
    int neg_before = getup_block_scan(neg, sh, &total);
    int first = 0;                                             // entries of this run that belong to the list: [i0, i0 + first)
    if (neg_before == 0)
        for (int k = 0; k < per; ++k) { const int i = i0 + k; if (i >= n || getup_absent(a.ids[i], g.n_env)) break; ++first; }

    // 1. every listed env gives its slot back
    for (int k = 0; k < first; ++k) {
        const int env = a.ids[i0 + k], s = g.assign[env];
        if (s >= 0 && s < P) g.pool_taken[s] = 0;
        g.assign[env] = -1;
    }
    __syncthreads();

    // the free slots in the order they are handed out: split_ws[r] = the r-th free slot along P_key(0), P_key(1), ...
    int nfree_run = 0, n_free;
    for (int k = 0; k < perp; ++k) { const int p = k0 + k; if (p < P && g.pool_taken[real_pick_perm((unsigned)p, (unsigned)P, a.slot_key)] == 0) ++nfree_run; }
    int r = getup_block_scan(nfree_run, sh, &n_free);
    for (int k = 0; k < perp; ++k) {
        const int p = k0 + k;
        if (p < P) { const int s = (int)real_pick_perm((unsigned)p, (unsigned)P, a.slot_key); if (g.pool_taken[s] == 0) g.split_ws[r++] = s; }
    }
    __syncthreads();

    // 2-5. classes; the j-th fall entry takes the j-th free slot, the surplus turns normal
    int cnt_fall = 0, dummy;
    for (int k = 0; k < first; ++k) cnt_fall += getup_classify(g, a, i0 + k, a.ids[i0 + k]) == GETUP_FALL ? 1 : 0;
    const int j0 = getup_block_scan(cnt_fall, sh, &dummy);
    int c_n = 0, c_f = 0, c_r = 0, j = j0;
    for (int k = 0; k < first; ++k) {
        int c = getup_classify(g, a, i0 + k, a.ids[i0 + k]);
        if (c == GETUP_FALL && j++ >= n_free) c = GETUP_NORMAL;
        c_n += c == GETUP_NORMAL; c_f += c == GETUP_FALL; c_r += c == GETUP_RECOVER;
    }
    int t_n, t_f, t_r;
    int o_n = getup_block_scan(c_n, sh, &t_n), o_f = getup_block_scan(c_f, sh, &t_f), o_r = getup_block_scan(c_r, sh, &t_r);
    j = j0;
    for (int k = 0; k < first; ++k) {
        const int env = a.ids[i0 + k];
        int c = getup_classify(g, a, i0 + k, env), slot = -1;
        if (c == GETUP_FALL) { if (j < n_free) slot = g.split_ws[j]; else c = GETUP_NORMAL; ++j; }
        if (c == GETUP_NORMAL) a.normal[o_n++] = env;
        else if (c == GETUP_RECOVER) a.recover[o_r++] = env;
        else { a.fall[o_f] = env; a.fall_slot[o_f++] = slot; g.pool_taken[slot] = 1; g.assign[env] = slot; }
        g.recovery_counter[env] = c == GETUP_NORMAL ? 0 : a.recovery_steps;           // 6.
    }
    // padding and counts
    for (int i = tid; i < n; i += GETUP_SPLIT_THREADS) {
        if (i >= t_n) a.normal[i] = -1;
        if (i >= t_f) { a.fall[i] = -1; a.fall_slot[i] = -1; }
        if (i >= t_r) a.recover[i] = -1;
    }
    if (tid == 0) {
        a.normal[n] = t_n; a.fall[n] = t_f; a.fall_slot[n] = t_f; a.recover[n] = t_r;
        if (g.stats) { g.stats[EMLOCO_GETUP_STAT_RECOVER] += t_r; g.stats[EMLOCO_GETUP_STAT_FALL] += t_f; g.stats[EMLOCO_GETUP_STAT_NORMAL] += t_n; }
    }
}

// random rows of the two lists of emloco_getup_apply made on the device: workgroups [0, half) the fall list (rows [0, n) of the
// workspace, seed), [half, 2 half) the recovery list (rows [n, 2 n), ~seed)
__global__ void __launch_bounds__(64)
getup_fill_rnd_kernel(const int32_t *fall, const int32_t *recover, int n, int half, unsigned seed_lo, unsigned seed_hi, float *ws) {
    const int which = (int)blockIdx.x >= half ? 1 : 0;
    const int32_t *ids = which ? recover : fall;
    float *rnd = ws + (which ? (long)n * EMLOCO_RESET_RND : 0);
    for (int bi = (int)blockIdx.x - which * half; bi < n; bi += half) {
        if (ids[bi] < 0) break;
        reset_fill_row(which ? ~seed_lo : seed_lo, which ? ~seed_hi : seed_hi, bi, rnd, threadIdx.x, blockDim.x);
    }
}

// _reset_fall_episode :166-168: the pool row of every fall entry into that env's simulator rows; warm-start impulses start from zero
__global__ void __launch_bounds__(64)
getup_copy_kernel(EmlocoGetupBufs g, EmlocoSimDev s, const int32_t *fall, const int32_t *fall_slot, int n) {
    const int lane = threadIdx.x;
    for (int bi = blockIdx.x; bi < n; bi += gridDim.x) {
        const int env = fall[bi], slot = fall_slot[bi];
        if (env < 0) break;
        if (slot < 0 || slot >= g.n_pool) continue;              // (a list that is not emloco_getup_split's: nothing to copy)
        const float *pr = g.pool_root + (long)slot * 13, *pd = g.pool_dof + (long)slot * RNDOF * 2;
        if (lane < 13) s.root_state[(long)env * 13 + lane] = pr[lane];
        for (int i = lane; i < RNDOF * 2; i += 64) s.dof_state[(long)env * RNDOF * 2 + i] = pd[i];
        for (int i = lane; i < EMLOCO_MAXCAND * 3; i += 64) s.lambda_ws[(long)env * EMLOCO_MAXCAND * 3 + i] = 0.0f;
    }
}

// what a reset does to an env whose state is in place (reset_finish_env without the height fix and without the warm-start impulses)
__device__ __forceinline__ void getup_finish_env(const EmlocoResetBufs &t, const EmlocoSimDev &s, int bi, int env, const float *u, int lane, float *sm) {
    if (lane == 0) { t.progress_buf[env] = 0; t.reset_buf[env] = 0; t.terminate_buf[env] = 0; }           // humanoid.py:477-480
    for (int i = lane; i < RNB * 3; i += 64) s.contact_force[(long)env * RNB * 3 + i] = 0.0f;
    const float *rs = s.root_state + (long)env * 13;
    const float ipx = rs[0], ipy = rs[1];
    const float rvx = rs[7], rvy = rs[8];
    reset_traj_to(t, u, bi, lane, ipx, ipy, rvx, rvy, rs[9], t.traj_verts + (long)env * RNV * 3, t.inverted + env,
                  t.waypoint_traj + (long)env * EMLOCO_TRAJ_SAMPLES * 3, sm);
    reset_capture_pose(t, s, env, lane, rvx, rvy);
}

// workgroups [0, half): the fall list, [half, 2 half): the recovery list
__global__ void __launch_bounds__(64)
getup_finish_kernel(EmlocoResetBufs t, EmlocoSimDev s, const int32_t *fall, const int32_t *recover, int n, int half, const float *rnd_fall,
                    const float *rnd_recover) {
    const int lane = threadIdx.x, which = (int)blockIdx.x >= half ? 1 : 0;
    const int32_t *ids = which ? recover : fall;
    const float *rnd = which ? rnd_recover : rnd_fall;
    for (int bi = (int)blockIdx.x - which * half; bi < n; bi += half) {
        const int env = ids[bi];
        if (env < 0) break;
        __shared__ float sm[TRAJ_SM_FLOATS];
        getup_finish_env(t, s, bi, env, rnd + (long)bi * EMLOCO_RESET_RND, lane, sm);
        __syncthreads();                              // LDS is reused by the next list entry
    }
}

// _init_amp_obs_default (humanoid_amp.py:499-502)
__global__ void __launch_bounds__(64)
getup_amp_default_kernel(float *amp_obs_buf, int amp_ring, const int32_t *ids, int n) {
    const int lane = threadIdx.x;
    for (int bi = blockIdx.x; bi < n; bi += gridDim.x) {
        const int env = ids[bi];
        if (env < 0) break;
        float *base = amp_obs_buf + (long)env * EMLOCO_AMP_STEPS * EMLOCO_AMP_ROW;
        const float *cur = base + (long)EMLOCO_AMP_PHYS_ROW(amp_ring, 0) * EMLOCO_AMP_ROW;
        for (int i = lane; i < EMLOCO_AMP_ROW; i += 64) {
            const float v = cur[i];
            for (int k = 1; k < EMLOCO_AMP_STEPS; ++k) base[(long)EMLOCO_AMP_PHYS_ROW(amp_ring, k) * EMLOCO_AMP_ROW + i] = v;
        }
    }
}

// _update_recovery_count :191-194 + _compute_reset :199-203
#define GETUP_FLAGS_THREADS 256
__global__ void __launch_bounds__(GETUP_FLAGS_THREADS)
getup_flags_kernel(EmlocoGetupBufs g) {
    const int env = blockIdx.x * GETUP_FLAGS_THREADS + threadIdx.x;
    int c = 0;
    if (env < g.n_env) {
        c = g.recovery_counter[env] - 1;
        c = c < 0 ? 0 : c;
        g.recovery_counter[env] = c;
        if (c > 0) { g.reset_buf[env] = 0; g.terminate_buf[env] = 0; g.progress_buf[env] -= 1; }
    }
    if (g.stats) {                                   // integer sums: the order of the atomic adds does not show
        int sum = c, held = c > 0 ? 1 : 0;
        for (int off = 32; off >= 1; off >>= 1) { sum += __shfl_xor(sum, off); held += __shfl_xor(held, off); }
        if ((threadIdx.x & 63) == 0) {
            if (sum) atomicAdd((unsigned long long *)(g.stats + EMLOCO_GETUP_STAT_COUNTER_SUM), (unsigned long long)sum);
            if (held) atomicAdd((unsigned long long *)(g.stats + EMLOCO_GETUP_STAT_HELD), (unsigned long long)held);
            if (env == 0) atomicAdd((unsigned long long *)(g.stats + EMLOCO_GETUP_STAT_FLAG_CALLS), 1ull);
        }
    }
}

}  // namespace emloco
