// sim_plan.h -- internal: the part plan of the rigid-body step's full launch (emloco_sim_set_plan).
//
// The split launch cuts an env.step into dependent workgroups, the parts of an env.  Which workgroup of the launch runs which
// substeps of which env used to be arithmetic on the workgroup index (part = index / n_env: all first parts, then all second
// parts, ...).  A plan is that mapping as a table: one 32-bit word per workgroup, in dispatch (= index) order.  It changes
// only which workgroup runs which substeps and when -- parts continue from plain copies and envs are independent, so every
// plan the checker accepts computes the fused step bit for bit.
//
//   bits  0..15  rank        position in the dispatch order: env = step_order[rank] (cost order on) or rank itself
//   bits 16..18  part        this env's part index, 0 .. 4
//   bits 19..21  sub_lo      first substep of the part
//   bits 22..24  n_sub_here  substeps of the part; 0: a tail part (final kinematics pass and write-back alone)
//   bit  25      publishes   stores the hand-over granules when it is done
//   bit  26      consumes    waits for its predecessor's hand-over (tag of part - 1)
//   bit  27      final       runs the final kinematics pass, the write-back and the cost key
//
// The plan depends on n_env, n_sub and the plan parameters alone -- not on the state, not on the order of the step -- so the host
// builds it once when the plan is set (sim_plan_build), checks it (sim_plan_check) and uploads it; the kernel reads its word
// with one scalar load (sim_plan_decode).  Parameters: rank classes {lo, hi, parts} that tile [0, n_env) in ascending order,
// each class cutting its envs' substeps into `parts` equal parts of 1, 2 or 4 substeps; `tail`: every env gets one more workgroup that does only the
// final pass and the write-back; `shift`: the parts of every class but the first stand `shift` stages later (earlier, when
// negative) in the index order.  Index order = by stage, within a stage by rank; the stage of an env's j-th workgroup is
// j (+ shift), so an env's workgroups always ascend in index -- a consumer is dispatched behind its producer, and the bounded
// poll of the hand-over (sim_kernels.hip) never holds a slot its producer still needs.
#pragma once
#include <vector>

#define EMLOCO_PLAN_RANK_BITS 16
#define EMLOCO_PLAN_MAX_ENVS (1 << EMLOCO_PLAN_RANK_BITS)
#define EMLOCO_PLAN_MAX_SUB 7          /* sub_lo and n_sub_here are 3-bit fields */
#define EMLOCO_PLAN_MAX_PARTS 5        /* four publishing parts (EMLOCO_PART_TAG keeps two bits for the part) and a tail */
#define EMLOCO_PLAN_MAX_CLASSES 8
#define EMLOCO_PLAN_MAX_SHIFT 4
#define EMLOCO_PLAN_PUBLISHES (1u << 25)
#define EMLOCO_PLAN_CONSUMES (1u << 26)
#define EMLOCO_PLAN_FINAL (1u << 27)

#ifndef EMLOCO_PLAN_HD
#define EMLOCO_PLAN_HD __host__ __device__ __forceinline__
#endif

namespace emloco {

EMLOCO_PLAN_HD unsigned sim_plan_word(int rank, int part, int sub_lo, int n_here, bool publishes, bool consumes, bool final) {
    return (unsigned)rank | (unsigned)part << 16 | (unsigned)sub_lo << 19 | (unsigned)n_here << 22 |
           (publishes ? EMLOCO_PLAN_PUBLISHES : 0u) | (consumes ? EMLOCO_PLAN_CONSUMES : 0u) | (final ? EMLOCO_PLAN_FINAL : 0u);
}

// What one workgroup of the step launch does.  The part index and the three flags stay packed as in the plan word and are
// taken out where they are used -- ONE scalar register lives through the kernel's loop instead of four (the rigid-body kernel
// runs at its register cap: every further live scalar is a spill to a vector lane and a v_readlane in the loop).  The substep
// range stands beside them: the uniform split knows no bound on n_sub, the plan word's 3-bit fields do.
struct SimPlanWork {
    unsigned word;            // part and flags, laid out as in the plan word
    int slot;                 // rank in the dispatch order (full launch) or entry of the id list
    int sub_lo, sub_hi;       // its substeps [sub_lo, sub_hi)
    bool valid;               // false: a workgroup past the launch's last one (a grid rounded up)
    EMLOCO_PLAN_HD int part() const { return (int)(word >> 16 & 7u); }          // the tag of its hand-over is EMLOCO_PART_TAG(seq, part)
    EMLOCO_PLAN_HD bool publishes() const { return (word & EMLOCO_PLAN_PUBLISHES) != 0u; }
    EMLOCO_PLAN_HD bool consumes() const { return (word & EMLOCO_PLAN_CONSUMES) != 0u; }
    EMLOCO_PLAN_HD bool final() const { return (word & EMLOCO_PLAN_FINAL) != 0u; }
};

// Workgroup `wg` of a launch over `n_slots` slots.  plan == NULL: the uniform split, n_parts equal parts per slot, all first
// parts, then all second parts, ... (n_parts = 1: the fused step); else word `wg` of the plan.
EMLOCO_PLAN_HD SimPlanWork sim_plan_decode(const unsigned *plan, int plan_n, unsigned wg, int n_slots, int n_parts, int n_sub) {
    SimPlanWork w;
    if (plan) {
        w.valid = wg < (unsigned)plan_n;
        w.word = w.valid ? plan[wg] : 0u;
        w.slot = (int)(w.word & (EMLOCO_PLAN_MAX_ENVS - 1));
        w.sub_lo = (int)(w.word >> 19 & 7u);
        w.sub_hi = w.sub_lo + (int)(w.word >> 22 & 7u);
    } else {
        const int part = (int)wg / n_slots;
        w.slot = (int)wg - part * n_slots;
        w.valid = part < n_parts;
        w.sub_lo = (n_sub * part) / n_parts;
        w.sub_hi = (n_sub * (part + 1)) / n_parts;
        w.word = w.valid ? sim_plan_word(0, part, 0, 0, part < n_parts - 1, part > 0, part == n_parts - 1) : 0u;
    }
    return w;
}

// The plan of `n_env` envs with `n_sub` substeps.  classes: n_classes triples {lo, hi, parts}.  Returns NULL and fills `out`,
// or the reason for the refusal.
inline const char *sim_plan_build(int n_env, int n_sub, const int *classes, int n_classes, int tail, int shift, std::vector<unsigned> &out) {
    out.clear();
    if (n_env < 1 || n_env > EMLOCO_PLAN_MAX_ENVS) return "1 to 65536 envs";
    if (n_sub < 1 || n_sub > EMLOCO_PLAN_MAX_SUB) return "1 to 7 substeps";
    if (!classes || n_classes < 1 || n_classes > EMLOCO_PLAN_MAX_CLASSES) return "1 to 8 rank classes";
    if (tail != 0 && tail != 1) return "tail is 0 or 1";
    if (shift < -EMLOCO_PLAN_MAX_SHIFT || shift > EMLOCO_PLAN_MAX_SHIFT) return "shift of -4 to 4 stages";
    int at = 0;
    for (int c = 0; c < n_classes; ++c) {
        const int lo = classes[3 * c], hi = classes[3 * c + 1], parts = classes[3 * c + 2];
        if (hi < lo) return "a class with descending bounds";
        if (lo < at) return "rank classes overlap or descend";
        if (lo > at) return "rank classes leave a gap";
        if (parts < 1 || parts > 4 || n_sub % parts != 0) return "the parts of a class (1 to 4) must divide the substeps";
        if (n_sub / parts == 3 || n_sub / parts > 4) return "the parts of a class must divide the substeps into parts of 1, 2 or 4";
        at = hi;
    }
    if (at != n_env) return "rank classes must end at n_env";
    for (int stage = -EMLOCO_PLAN_MAX_SHIFT; stage < EMLOCO_PLAN_MAX_PARTS + EMLOCO_PLAN_MAX_SHIFT; ++stage)
        for (int c = 0; c < n_classes; ++c) {
            const int lo = classes[3 * c], hi = classes[3 * c + 1], parts = classes[3 * c + 2];
            const int j = stage - (c > 0 ? shift : 0), n_wg = parts + tail, per = n_sub / parts;
            if (j < 0 || j >= n_wg) continue;
            const bool is_tail = j == parts, last = j == n_wg - 1;
            for (int rank = lo; rank < hi; ++rank)
                out.push_back(sim_plan_word(rank, j, is_tail ? n_sub : j * per, is_tail ? 0 : per, !last, j > 0, last));
        }
    return nullptr;
}

// Is `plan` a launch that computes the step of every rank exactly once?  NULL, or what is wrong with it.
//  - every (rank, substep) is covered exactly once and in order: a rank's parts are numbered 0, 1, ... in index order, each
//    starts at the substep its predecessor stopped at, and the last one stops at n_sub;
//  - exactly one workgroup per rank is final, it comes behind (or holds) the rank's last substep and nothing follows it;
//  - a consumer's index is greater than its producer's, the producer published and the first part consumes nothing;
//  - at most four publishing parts per rank, numbered 0 .. 3 (EMLOCO_PART_TAG).
inline const char *sim_plan_check(const unsigned *plan, int plan_n, int n_env, int n_sub) {
    if (!plan || plan_n < 1) return "empty plan";
    if (n_env < 1 || n_env > EMLOCO_PLAN_MAX_ENVS || n_sub < 1 || n_sub > EMLOCO_PLAN_MAX_SUB) return "n_env / n_sub out of range";
    struct Rank { int parts = 0, next_sub = 0, publishers = 0; bool published = false, done = false; };
    std::vector<Rank> rk((size_t)n_env);
    for (int i = 0; i < plan_n; ++i) {
        const SimPlanWork w = sim_plan_decode(plan, plan_n, (unsigned)i, n_env, 1, n_sub);
        if (plan[i] >> 28) return "unknown bits set";
        if (w.slot >= n_env) return "rank beyond n_env";
        const int part = w.part(), sub_lo = w.sub_lo, sub_hi = w.sub_hi;
        const bool consumes = w.consumes(), publishes = w.publishes(), final = w.final();
        Rank &r = rk[(size_t)w.slot];
        if (r.done) return "a workgroup behind the final one of its rank";
        if (part != r.parts) return "parts of a rank not numbered in index order";           // with it: producer's index < consumer's
        if (sub_lo != r.next_sub) return "a part does not start where its predecessor stopped";
        const int n_here = sub_hi - sub_lo;
        if (n_here != 0 && n_here != 1 && n_here != 2 && n_here != 4) return "a part of 0, 1, 2 or 4 substeps";
        if (sub_hi > n_sub) return "substeps beyond n_sub";
        if (consumes != (part > 0)) return "the first part consumes nothing, every later part its predecessor's hand-over";
        if (consumes && !r.published) return "a consumer whose producer does not publish";
        if (publishes == final) return "a part either publishes or is final";
        if (n_here == 0 && !final) return "only a final part may be empty";
        if (final && sub_hi != n_sub) return "the final part comes ahead of the last substep";
        if (publishes && (part > 3 || ++r.publishers > 4)) return "more than four publishing parts";
        r.parts++; r.next_sub = sub_hi; r.published = publishes; r.done = final;
    }
    for (int e = 0; e < n_env; ++e)
        if (!rk[(size_t)e].done) return "a rank without its final part";
    return nullptr;
}

}  // namespace emloco
