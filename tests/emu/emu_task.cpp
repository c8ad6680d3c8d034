// TEST INFRASTRUCTURE ONLY: runs emloco_amd/csrc/task_kernels.hip on the CPU through tests/emu/hip/.
#include <cstring>
#include "hip/hip_runtime.h"
#include "../../emloco_amd/csrc/task_kernels.hip"
#include "../../emloco_amd/csrc/reset_kernels.hip"
#include "../../emloco_amd/csrc/chain_kernels.hip"
#include "../../emloco_amd/csrc/traj_kernels.hip"
#include "../../emloco_amd/csrc/topology.h"
#include "../../emloco_amd/csrc/model_pack.h"

extern "C" int emu_task_post_physics(const EmlocoTaskBufs *b, int mode, const int32_t *env_ids, int n) {
    const int count = env_ids ? n : b->n_env;
    EmlocoTaskBufs t = *b;
    emu::launch((unsigned)count, 64, [&] { emloco::post_physics_kernel(t, mode, env_ids, count); });
    return 0;
}

extern "C" int emu_task_amp_rows(int n, const float *root_pos, const float *root_rot, const float *root_vel,
                                 const float *root_ang, const float *dof_pos, const float *dof_vel, const float *key_pos,
                                 const float *betas, const int32_t *subset, int n_sub, float *out) {
    emu::launch((unsigned)n, 64, [&] {
        emloco::amp_rows_kernel(n, root_pos, root_rot, root_vel, root_ang, dof_pos, dof_vel, key_pos, betas, subset, n_sub, out);
    });
    return 0;
}

extern "C" int emu_task_pd_targets(int n_env, const float *actions, const float *offset, const float *scale,
                                   const uint8_t *zero_mask, float *out) {
    const int total = n_env * 69;
    emu::launch((unsigned)((total + 255) / 256), 256, [&] { emloco::pd_targets_kernel(total, actions, offset, scale, zero_mask, out, (float *)nullptr); });
    return 0;
}

// the launch of emloco_task_pd_targets_copy: the targets and (actions_copy != NULL) a copy of the actions in one pass
extern "C" int emu_task_pd_targets_copy(int n_env, const float *actions, const float *offset, const float *scale,
                                        const uint8_t *zero_mask, float *out, float *actions_copy) {
    const int total = n_env * 69;
    emu::launch((unsigned)((total + 255) / 256), 256, [&] { emloco::pd_targets_kernel(total, actions, offset, scale, zero_mask, out, actions_copy); });
    return 0;
}

extern "C" int emu_compact_flags(const int64_t *flags, int n, int32_t *ids) {
    emu::launch(1, 1024, [&] { emloco::compact_flags_kernel(flags, n, ids, (int64_t *)nullptr); });
    return 0;
}

extern "C" int emu_task_traj_reset(const EmlocoResetBufs *b, const int32_t *env_ids, int n, const float *rnd,
                                   const float *init_pos, const float *root_vel) {
    EmlocoResetBufs t = *b;
    emu::launch((unsigned)n, 64, [&] { emloco::traj_reset_kernel(t, env_ids, n, rnd, init_pos, root_vel); });
    return 0;
}

extern "C" int emu_task_get_heights(const int16_t *hf, int rows, int cols, float hscale, float vscale, const float *pose7, int n,
                                    int grid, float *out_h, int64_t *out_px, int64_t *out_py) {
    emu::launch((unsigned)n, 64, [&] { emloco::get_heights_kernel(hf, rows, cols, hscale, vscale, pose7, n, grid, out_h, out_px, out_py); });
    return 0;
}

// the two-workgroup launch of the fused chain: block 0 compacts the flags (+ snapshot), block 1 sorts the dispatch order
extern "C" int emu_compact_order(const int64_t *flags, int n, int32_t *ids, int64_t *snapshot, const unsigned *ticks, int n_order, int *order,
                                 unsigned char *bucket_ws) {
    emu::launch(ticks ? 2u : 1u, 1024, [&] { emloco::compact_order_kernel(flags, n, ids, snapshot, ticks, n_order, order, bucket_ws); });
    return 0;
}

// reset_obs_kernel with an empty finished-env list: only the observation role does work (post-physics pass `live_mode` of every env
// whose snapshot entry is zero) -- the role arithmetic of the launch on the CPU
extern "C" int emu_reset_obs_live(const EmlocoTaskBufs *pb, int live_mode, const int64_t *skip, const int32_t *ids, int n, int n_slots, int h_slots, int n_hist) {
    EmlocoResetBufs rb; memset(&rb, 0, sizeof(rb));
    EmlocoSimDev sd; memset(&sd, 0, sizeof(sd));
    emloco::ChainArgs a; memset(&a, 0, sizeof(a));
    a.n = n; a.n_slots = n_slots; a.h_slots = h_slots; a.n_hist = n_hist; a.live_mode = live_mode; a.reset_mode = EMLOCO_POST_OBS | EMLOCO_POST_AMP_ROW;
    a.seeded = 1; a.ids = ids; a.skip = skip;
    const unsigned grid = (unsigned)(n_slots + h_slots * n_hist + pb->n_env);
    emu::launch(grid, 64, [&] { emloco::reset_obs_kernel(*pb, rb, sd, a); });
    return 0;
}

// the flags launch with the LocoVal return bookkeeping of every env behind its reward and reset flag
extern "C" int emu_task_post_physics_returns(const EmlocoTaskBufs *b, int mode, const EmlocoLocoValStep *step, const uint8_t *inverted) {
    EmlocoLocoValStep lv = *step;
    emu::launch((unsigned)b->n_env, 64, [&] { emloco::post_physics_returns_kernel(*b, mode, lv, inverted); });
    return 0;
}

// traj_densify_kernel with the arguments of emloco_traj_densify (include/emloco_task.h), all arrays on the host; validation and packing
// are the product's own (emloco::densify_pack), the launch is the emulator's
static const char *g_densify_why = "";

extern "C" const char *emu_traj_densify_error(void) { return g_densify_why; }

extern "C" int emu_traj_densify(const float *knot_t, int n_knots, const float *way, int64_t n_traj, const float *query_t, int n_query,
                                float *out, uint8_t *valid, int flags) {
    emloco::DensifyArgs a;
    const char *why = emloco::densify_pack(knot_t, n_knots, (long long)n_traj, query_t, n_query, flags, &a);
    g_densify_why = why ? why : "";
    if (why) return -1;
    if (n_traj == 0) return 0;
    if (!way || !out) return -1;
    emu::launch((unsigned)((n_traj + emloco::DENSIFY_TPB - 1) / emloco::DENSIFY_TPB), emloco::DENSIFY_THREADS,
                [&] { emloco::traj_densify_kernel(a, way, out, valid); });
    blockIdx.x = 0;
    return 0;
}

// ---- the reset kernels (reset_kernels.hip) and the reset roles of reset_obs_kernel, launched with the launcher's own grid rule
// (task_capi.hip: min(n, 256) workgroups; (grid, 14) for the AMP history).  The simulator block is built as emu_sim_fk builds it:
// emloco::pack_models, the topology block, host arrays.
namespace {
struct EmuSimDev {
    EmlocoSimDev d{};
    std::vector<int32_t> topo;
    std::vector<float> mdl;
    bool build(const EmlocoModelDesc *m, float *root, float *dof, float *rb, float *contact, float *lambda_ws) {
        emloco::Topology t;
        if (!t.build(m->parent, m->geom_type)) return false;
        d.n_env = m->n_env; d.n_cand = t.n_cand; d.max_depth = t.max_depth;
        topo = emloco::pack_topology(t, nullptr, 0);
        mdl = emloco::pack_models(m->n_env, m->joint_off, m->mass, m->com, m->inertia, m->geom_a, m->geom_b, m->geom_r, m->kp, m->kd,
                                  m->armature, m->effort, nullptr, nullptr, nullptr);
        d.topo = topo.data(); d.model = mdl.data();
        d.root_state = root; d.dof_state = dof; d.rb_state = rb; d.contact_force = contact; d.lambda_ws = lambda_ws;
        return true;
    }
};
unsigned reset_grid(int n) { return (unsigned)(n < 256 ? n : 256); }
}  // namespace

extern "C" int emu_reset_fill_rnd(const int32_t *ids, int n, uint64_t seed, float *rnd) {
    if (n < 1) return 0;
    emu::launch(reset_grid(n), 64, [&] { emloco::reset_fill_rnd_kernel(ids, n, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), rnd); });
    return 0;
}

enum { EMU_RESET_SAMPLE = 1, EMU_RESET_FK = 2, EMU_RESET_FINISH = 4, EMU_RESET_HISTORY = 8 };

// the launches of emloco_task_reset one by one (stages: EMU_RESET_* bits, in the launcher's order)
extern "C" int emu_task_reset_stages(int stages, const EmlocoResetBufs *b, const EmlocoModelDesc *m, float *root, float *dof, float *rb,
                                     float *contact, float *lambda_ws, const int32_t *ids, int n, const float *rnd) {
    EmuSimDev s;
    if (!s.build(m, root, dof, rb, contact, lambda_ws)) return -1;
    if (n < 1) return 0;
    const EmlocoResetBufs t = *b;
    const EmlocoSimDev d = s.d;
    const unsigned grid = reset_grid(n);
    if (stages & EMU_RESET_SAMPLE) emu::launch(grid, 64, [&] { emloco::reset_sample_kernel(t, d, ids, n, rnd); });
    if (stages & EMU_RESET_FK)
        emu::launch(grid, 64, [&] {
            for (int bi = (int)blockIdx.x; bi < n; bi += (int)gridDim.x) {
                const int env = ids[bi];
                if (env < 0) break;
                __shared__ float sm[FK_SM_FLOATS];
                emloco::fk_env(d, env, (int)threadIdx.x, sm);
                __syncthreads();
            }
        });
    if (stages & EMU_RESET_FINISH) emu::launch(grid, 64, [&] { emloco::reset_finish_kernel(t, d, ids, n, rnd); });
    if (stages & EMU_RESET_HISTORY) {
        gridDim.y = EMLOCO_AMP_STEPS - 1;
        for (unsigned y = 0; y < EMLOCO_AMP_STEPS - 1; ++y) {
            blockIdx.y = y;
            emu::launch(grid, 64, [&] { emloco::reset_amp_history_kernel(t, ids, n); });
        }
        blockIdx.y = 0; gridDim.y = 1;
    }
    return 0;
}

// emloco_task_reset_obs_pooled on the CPU: every role of reset_obs_kernel.  The pool rules, ChainArgs, the keyed reset buffers and
// the grid are the product's own (emloco::chain_pool_error, emloco::chain_pack: what task_capi.hip calls); only the launch is the
// emulator's.  ids holds n + 1 entries when a pool is passed (ids[n]: the number of finished envs).  -1: a refused pool argument.
static const char *g_chain_why = "";
static long long *g_chain_prof = nullptr;

// the 16 wall-clock stamps of emloco_task_chain_profile: a host buffer that every later emu_task_reset_obs launch stamps (NULL: none)
extern "C" void emu_task_set_chain_prof(long long *host16) { g_chain_prof = host16; }

extern "C" const char *emu_task_reset_obs_error(void) { return g_chain_why; }

extern "C" int emu_task_reset_obs(const EmlocoTaskBufs *pb, const EmlocoResetBufs *b, const EmlocoModelDesc *m, float *root, float *dof, float *rb,
                                  float *contact, float *lambda_ws, const int32_t *ids, int n, uint64_t seed, float *rnd_ws, const float *rnd,
                                  const EmlocoResetPool *pool, int live_mode, const int64_t *skip) {
    const char *why = emloco::chain_pool_error(pool);
    g_chain_why = why ? why : "";
    if (why) return -1;
    EmuSimDev s;
    if (!s.build(m, root, dof, rb, contact, lambda_ws)) return -2;
    emloco::ChainArgs a; memset(&a, 0, sizeof(a));
    EmlocoResetBufs keyed;
    const unsigned grid = emloco::chain_pack(*b, pb->n_env, live_mode, skip, ids, n, seed, rnd_ws, rnd, pool, g_chain_prof, &a, &keyed);
    if (grid == 0) return 0;
    const EmlocoTaskBufs p = *pb;
    const EmlocoSimDev d = s.d;
    emu::launch(grid, 64, [&] { emloco::reset_obs_kernel(p, keyed, d, a); });
    return 0;
}
