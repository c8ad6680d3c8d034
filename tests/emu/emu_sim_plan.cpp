// TEST INFRASTRUCTURE ONLY: the emulator's rigid-body driver (emu_sim.cpp, included whole: its setters and statics are this
// library's own copies) plus a step that launches by a part plan (emloco_sim_set_plan, csrc/sim_plan.h) and the plan's host
// functions.  Built on its own by tests/test_sim_plan_cpu.py together with emu_runtime.cpp.
#include "emu_sim.cpp"
#include <string>

static std::vector<unsigned> g_plan;          // emu_sim_plan_set: the plan of the next emu_sim_step_plan calls (empty: none)
static int g_plan_n_sub = 0;
static std::string g_plan_err;

extern "C" const char *emu_sim_plan_error() { return g_plan_err.c_str(); }
extern "C" void emu_sim_plan_clear() { g_plan.clear(); g_plan_n_sub = 0; }

// as emloco_sim_set_plan: build, check, keep.  0, or -1 with the reason in emu_sim_plan_error() and the plan in force kept.
extern "C" int emu_sim_plan_set(int n_env, int n_sub, const int *classes, int n_classes, int tail, int shift) {
    std::vector<unsigned> plan;
    const char *why = emloco::sim_plan_build(n_env, n_sub, classes, n_classes, tail, shift, plan);
    if (!why) why = emloco::sim_plan_check(plan.data(), (int)plan.size(), n_env, n_sub);
    g_plan_err = why ? why : "";
    if (why) return -1;
    g_plan.swap(plan); g_plan_n_sub = n_sub;
    return 0;
}

// the words of the plan in force (up to `cap`); returns their number
extern "C" int emu_sim_plan_words(unsigned *out, int cap) {
    for (int i = 0; i < (int)g_plan.size() && i < cap; ++i) out[i] = g_plan[i];
    return (int)g_plan.size();
}

// the checker alone, on any words
extern "C" int emu_sim_plan_check(const unsigned *plan, int plan_n, int n_env, int n_sub) {
    const char *why = emloco::sim_plan_check(plan, plan_n, n_env, n_sub);
    g_plan_err = why ? why : "";
    return why ? -1 : 0;
}

// emu_sim_step with the launch of emloco_sim_step / emloco_sim_step_subset under a plan: the full launch (and the skip-flag launch) takes
// one workgroup per word of the plan when the plan was built for this launch's substep count; the id-list launch stays unsplit
extern "C" int emu_sim_step_plan(const EmlocoSimParams *prm, const EmlocoModelDesc *m, float *root_state,
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
    int n_parts = g_launch.parts > 0 ? g_launch.parts : 1;
    if (n_parts > p.n_sub) n_parts = p.n_sub;
    if (g_launch.ids) n_parts = 1;
    const bool planned = !g_launch.ids && !g_plan.empty() && g_plan_n_sub == p.n_sub;
    const bool handover = planned || n_parts > 1;
    std::vector<float> part_state(handover ? (size_t)m->n_env * EMLOCO_PART_WORDS : 0, 0.0f);
    d.n_parts = n_parts; d.part_seq = 1;
    d.part_state = handover ? part_state.data() : nullptr;
    const char *po = getenv("EMLOCO_EMU_POISON");
    unsigned err = 0u;
    d.part_spin_max = 4; d.part_poison = po ? atoi(po) : -1; d.err = &err;
    d.n_slots = g_launch.ids ? g_launch.n_ids : m->n_env;
    d.step_ticks = g_ticks;
    d.step_ids = g_launch.ids; d.step_skip = g_launch.skip;
    d.step_order = g_launch.ids ? nullptr : g_launch.order;
    if (d.n_slots < 1) return 0;
    unsigned grid = (unsigned)(d.n_slots * n_parts);
    if (planned) { d.plan = g_plan.data(); d.plan_n = (int)g_plan.size(); grid = (unsigned)g_plan.size(); }
    emu::launch(grid + (unsigned)g_launch.grid_pad, 64, [&] { if (d.hf) emloco::sim_step_kernel<1>(p, d); else emloco::sim_step_kernel<0>(p, d); });
    return (int)err;
}
