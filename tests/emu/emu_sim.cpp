#include <vector>
#include <cstdlib>
// TEST INFRASTRUCTURE ONLY: runs emloco_amd/csrc/sim_kernels.hip on the CPU through the emulation
// header in tests/emu/hip/, so the kernel's logic can be compared with the oracle without a GPU.
#include "hip/hip_runtime.h"
#ifdef EMLOCO_SIM_PAIR      /* EMLOCO_EMU_EXTRA="-DEMLOCO_SIM_PAIR=1": the two-envs-per-wave kernel (round 6, experimental) */
#include "../../emloco_amd/csrc/sim_pair_kernels.hip"
#define EMU_ENVS_PER_WG 2
#else
#include "../../emloco_amd/csrc/sim_kernels.hip"
#define EMU_ENVS_PER_WG 1
#endif
#include "../../emloco_amd/csrc/topology.h"
#include "../../emloco_amd/csrc/model_pack.h"

static const EmlocoSelfCollisionDesc *g_sc = nullptr;      // set by emu_sim_set_self_collision for the next emu_sim_step calls
extern "C" void emu_sim_set_self_collision(const EmlocoSelfCollisionDesc *sc) { g_sc = sc; }

struct EmuHeightfield { const short *samples; int nx, ny; float hs, vs, ox, oy; const unsigned char *mv; };
static EmuHeightfield g_hf = {nullptr, 0, 0, 0, 0, 0, 0, nullptr};   // set by emu_sim_set_heightfield for the next emu_sim_step calls
extern "C" void emu_sim_set_heightfield(const short *samples, int nx, int ny, float hs, float vs, float ox, float oy, const unsigned char *mv) {
    g_hf = {samples, nx, ny, hs, vs, ox, oy, mv};       // mv: packed vertex moves of the slope-corrected mesh (emloco_types.h: hf_mv) or NULL
}

static unsigned *g_ticks = nullptr;   // set by emu_sim_set_cost_ticks: [n_env] words that take the key of the cost-ordered dispatch (or NULL)
extern "C" void emu_sim_set_cost_ticks(unsigned *ticks) { g_ticks = ticks; }

// The launch-level arguments of emloco_sim_step / emloco_sim_step_subset (csrc/sim_capi.hip) for the next emu_sim_step calls:
// `order` [n_env] the dispatch order of a full launch (emloco_sim_set_cost_order), `ids` [n_ids] a compacted id list (valid ids
// first, -1 after them: workgroup i steps entry i, never split), `skip` [n_env] int64 flags (non-zero: left untouched), `parts`
// the split (emloco_sim_set_split; 0: EMLOCO_EMU_PARTS decides).  All NULL / 0: the plain step.
// `grid_pad`: workgroups beyond the launch's last one (a launcher that rounds its grid up): the kernel's guard sends them home.
struct EmuLaunch { const int *order; const int *ids; int n_ids; const long long *skip; int parts; int grid_pad; };
static EmuLaunch g_launch = {nullptr, nullptr, 0, nullptr, 0, 0};
extern "C" void emu_sim_set_launch(const int *order, const int *ids, int n_ids, const long long *skip, int parts, int grid_pad) {
    g_launch = {order, ids, n_ids, skip, parts, grid_pad};
}

extern "C" int emu_sim_step(const EmlocoSimParams *prm, const EmlocoModelDesc *m, float *root_state,
                            float *dof_state, const float *pd_target, float *rb_state, float *contact_force,
                            float *dof_force, float *lambda_ws, int n_calls) {
    emloco::Topology t;
    if (!t.build(m->parent, m->geom_type)) return -1;
    EmlocoSimDev d{};
    d.n_env = m->n_env; d.n_cand = t.n_cand; d.max_depth = t.max_depth;
    const bool sc_on = g_sc && g_sc->n_pairs > 0;
    const int n_seg = (sc_on && g_sc->n_seg > 0 && g_sc->seg_body) ? g_sc->n_seg : EMLOCO_NB;
    const unsigned char *seg_body = (sc_on && g_sc->n_seg > 0) ? g_sc->seg_body : nullptr;
    const std::vector<int32_t> topo = emloco::pack_topology(t, sc_on ? g_sc->pairs : nullptr, sc_on ? g_sc->n_pairs : 0, seg_body);
    const std::vector<float> mdl = emloco::pack_models(m->n_env, m->joint_off, m->mass, m->com, m->inertia, m->geom_a, m->geom_b, m->geom_r,
                                                       m->kp, m->kd, m->armature, m->effort, sc_on ? g_sc->cap_a : nullptr,
                                                       sc_on ? g_sc->cap_b : nullptr, sc_on ? g_sc->cap_r : nullptr, n_seg, seg_body);
    d.topo = topo.data(); d.model = mdl.data();
    d.root_state = root_state; d.dof_state = dof_state; d.pd_target = pd_target;
    d.rb_state = rb_state; d.contact_force = contact_force; d.dof_force = dof_force; d.lambda_ws = lambda_ws;
    if (sc_on) { d.sc_nseg = n_seg; d.sc_n = g_sc->n_pairs; d.sc_k = g_sc->k; d.sc_c = g_sc->c; d.sc_max_pen = g_sc->max_pen; d.sc_mu = g_sc->mu; }
    if (g_hf.samples) {
        d.hf = g_hf.samples; d.hf_nx = g_hf.nx; d.hf_ny = g_hf.ny; d.hf_hs = g_hf.hs; d.hf_inv_hs = 1.0f / g_hf.hs; d.hf_vs = g_hf.vs;
        d.hf_ox = g_hf.ox; d.hf_oy = g_hf.oy; d.hf_mv = g_hf.mv;
    }
    EmlocoSimParams p = *prm;
    p.n_sub = prm->n_sub * n_calls;
    // EMLOCO_EMU_PARTS=n: the split launch (emloco_sim_set_split) -- n workgroups per env, all first parts first
    const char *pe = getenv("EMLOCO_EMU_PARTS");
    int n_parts = g_launch.parts > 0 ? g_launch.parts : (pe ? atoi(pe) : 1);
    if (n_parts > p.n_sub) n_parts = p.n_sub;             // at least one substep per part, as emloco_sim_step clamps it
    if (g_launch.ids) n_parts = 1;                        // the list launch is not split (emloco_sim_step_subset)
    // the hand-over buffers exist only for a split launch, as emloco_sim_set_split allocates them
    std::vector<float> part_state(n_parts > 1 ? (size_t)m->n_env * EMLOCO_PART_WORDS : 0, 0.0f);
    std::vector<unsigned> part_flag(n_parts > 1 ? (size_t)m->n_env : 0, 0u);
    d.n_parts = n_parts; d.part_seq = 1;
    d.part_state = n_parts > 1 ? part_state.data() : nullptr; d.part_flag = n_parts > 1 ? part_flag.data() : nullptr;
    // EMLOCO_EMU_POISON=env: the first part of that env withholds its hand-over flag (emloco_sim_debug_poison_part); the
    // device error word is the return value (0: fine)
    const char *po = getenv("EMLOCO_EMU_POISON");
    unsigned err = 0u;
    d.part_spin_max = 4; d.part_poison = po ? atoi(po) : -1; d.err = &err;
    d.n_slots = g_launch.ids ? g_launch.n_ids : m->n_env;
    d.step_ticks = g_ticks;
    d.step_ids = g_launch.ids; d.step_skip = g_launch.skip;
    d.step_order = g_launch.ids ? nullptr : g_launch.order;     // a list launch takes its envs from the list (emloco_sim_step_subset)
    if (d.n_slots < 1) return 0;
    emu::launch((unsigned)(((d.n_slots + EMU_ENVS_PER_WG - 1) / EMU_ENVS_PER_WG) * n_parts + g_launch.grid_pad), 64, [&] { if (d.hf) emloco::sim_step_kernel<1>(p, d); else emloco::sim_step_kernel<0>(p, d); });
    return (int)err;
}

// env_ids NULL: every env; else the listed ones, up to the first -1 (a device-compacted list).  grid < 1: one workgroup per entry,
// else `grid` workgroups stride over the list (the launcher's cap of 256).
extern "C" int emu_sim_fk(const EmlocoModelDesc *m, float *root_state, float *dof_state, float *rb_state, const int *env_ids, int n_ids, int grid) {
    emloco::Topology t;
    if (!t.build(m->parent, m->geom_type)) return -1;
    EmlocoSimDev d{};
    d.n_env = m->n_env; d.n_cand = t.n_cand; d.max_depth = t.max_depth;
    const std::vector<int32_t> topo = emloco::pack_topology(t, nullptr, 0);
    const std::vector<float> mdl = emloco::pack_models(m->n_env, m->joint_off, m->mass, m->com, m->inertia, m->geom_a, m->geom_b, m->geom_r,
                                                       m->kp, m->kd, m->armature, m->effort, nullptr, nullptr, nullptr);
    d.topo = topo.data(); d.model = mdl.data();
    d.root_state = root_state; d.dof_state = dof_state; d.rb_state = rb_state;
    if (!env_ids) n_ids = m->n_env;
    if (n_ids < 1) return 0;
    emu::launch((unsigned)(grid < 1 ? n_ids : grid), 64, [&] { emloco::sim_fk_kernel(d, env_ids, n_ids); });
    return 0;
}

// copy_rows_kernel as the *_indexed setters launch it when `dev_full` is not the simulator's own tensor: one workgroup per list entry
extern "C" void emu_sim_copy_rows(const float *src, float *dst, const int *ids, int n_ids, int row_len, int n_env, int grid_pad) {
    if (n_ids < 1) return;
    emu::launch((unsigned)(n_ids + grid_pad), 64, [&] { emloco::copy_rows_kernel(src, dst, ids, n_ids, row_len, n_env); });
}
