// crowd_contact_kernels.hip -- the crowd contact audit (include/emloco_task.h: EmlocoCrowdContacts): capsule overlaps BETWEEN the
// humanoids of a group, from the collision segments the self-collision step uses.  Included by crowd_capi.hip, which is built
// without fused-multiply-add contraction: plain fp32 in the order the header states, so the CPU emulation gives the same bytes.
//   crowd_contact_prep_kernel     one wave per env: root-relative segments, bound, finiteness
//   crowd_contact_kernel          one wave per env: root test over the group's members, narrow phase per surviving member (two at a time)
//   crowd_contact_accumulate_kernel   one thread per env: the game's accumulators, records, epoch totals
//   crowd_contact_reduce_kernel / crowd_contact_epoch_kernel   one workgroup each, double, fixed tree order
// No LDS in the geometry kernels: a member's segment sits in its lane's registers, the env's own segments are 1 KB of a workspace read
// at wave-uniform addresses, and the lanes of a wave exchange through ballots and shuffles only, so nothing needs a barrier.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_math.h"
#include "../../include/emloco_sim.h"
#include "../../include/emloco_task.h"

namespace emloco {

constexpr int kContactThreads = 256;
constexpr int kContactWaves = kContactThreads / 64;
constexpr int kContactBodies = 24;
constexpr int kContactReduceThreads = 256;
constexpr float kContactCullSlack = 1e-3f;

static_assert(sizeof(EmlocoCrowdContactNow) == 32 && sizeof(EmlocoCrowdContactRecord) == 48, "the audit's records are 32 / 48 bytes");

__device__ __forceinline__ bool cc_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float cc_norm3(const float *v) { return sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// One wave per env (grid-stride over waves): lanes 0 .. 167 / 64 test the 24 x 7 position and quaternion values, lane i < n_seg
// places segment i; the bound is a wave maximum.
__global__ __launch_bounds__(kContactThreads) void crowd_contact_prep_kernel(const EmlocoCrowdContacts c) {
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int env = (int)blockIdx.x * kContactWaves + wave; env < c.n_env; env += (int)gridDim.x * kContactWaves) {
        const float *rb = c.rb_state + (long)env * kContactBodies * 13;
        bool ok = true;
        for (int v = lane; v < kContactBodies * 7; v += 64) {
            const int b = v / 7, k = v - b * 7;
            ok = ok && cc_finite(rb[b * 13 + k]);
        }
        const bool finite = __ballot(!ok) == 0ull;
        float reach = 0.0f;
        float *out = c.caps_ws + ((long)env * EMLOCO_SC_MAXSEG + lane) * 8;
        if (lane < c.n_seg) {
            float A[3] = {0.0f, 0.0f, 0.0f}, B[3] = {0.0f, 0.0f, 0.0f}, r = 0.0f, hr = 0.0f;
            if (finite) {
                int b = (int)c.seg_body[lane];
                b = b < kContactBodies ? b : kContactBodies - 1;
                const float *pb = rb + b * 13;
                float R[9], o[3], ra[3], rbv[3];
                q2mat(pb + 3, R);
                for (int k = 0; k < 3; ++k) o[k] = pb[k] - rb[k];
                matvec3(R, c.cap_a + ((long)env * c.n_seg + lane) * 3, ra);
                matvec3(R, c.cap_b + ((long)env * c.n_seg + lane) * 3, rbv);
                for (int k = 0; k < 3; ++k) { A[k] = o[k] + ra[k]; B[k] = o[k] + rbv[k]; }
                r = c.cap_r[(long)env * c.n_seg + lane];
                const float na = cc_norm3(A), nb = cc_norm3(B);
                reach = (na > nb ? na : nb) + r;
                const float h[3] = {0.5f * (B[0] - A[0]), 0.5f * (B[1] - A[1]), 0.5f * (B[2] - A[2])};
                hr = cc_norm3(h) + r;                               // the segment lies within hr of its midpoint: the pair cull's radius
            }
            out[0] = A[0]; out[1] = A[1]; out[2] = A[2]; out[3] = r;
            out[4] = B[0]; out[5] = B[1]; out[6] = B[2]; out[7] = hr;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float other = __shfl_xor(reach, off);
            reach = other > reach ? other : reach;
        }
        if (lane < 4) c.roots_ws[(long)env * 4 + lane] = !finite ? (lane == 3 ? -1.0f : 0.0f) : (lane == 3 ? reach : rb[lane]);
    }
}

// One wave per env.  Lane l tests member c0 + l of the group for each chunk c0 of 64 members (one 16-byte record each); the survivors
// of the member cull leave a ballot and are visited in ascending order TWO at a time, one per half wave: lane j of a half holds
// segment j of its member, moved by s, in registers, and all lanes walk the env's own segments i together (wave-uniform addresses:
// scalar loads on the device).  A pair is skipped when the midpoints are farther apart than hr_i + hr_j + 1e-3 allows.
// A lane keeps its deepest (pen, member, pair) under strict >, members and own segments ascending, i.e. the lexicographically lowest
// key of its j; one wave reduction at the end picks the maximum and, among equals, the lowest key (member, i, j).
__global__ __launch_bounds__(kContactThreads) void crowd_contact_kernel(const EmlocoCrowdContacts c, EmlocoCrowdContactNow *now) {
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, j = lane & 31;
    const int n_seg = c.n_seg, gs = c.group_size;
    for (int env_v = (int)blockIdx.x * kContactWaves + wave; env_v < c.n_env; env_v += (int)gridDim.x * kContactWaves) {
        const int env = __builtin_amdgcn_readfirstlane(env_v);     // (the same in every lane: lets the own segments come by scalar loads)
        const float *own_root = c.roots_ws + (long)env * 4;
        const float bound_e = own_root[3];
        if (bound_e < 0.0f) {                                      // (wave-uniform) non-finite: flagged, nobody's neighbour
            if (lane == 0) {
                EmlocoCrowdContactNow o;
                o.nearest = 0.0f; o.pen = 0.0f; o.nearest_member = -1; o.pen_member = -1; o.pen_segs = -1; o.n_pen = 0; o.n_near = 0; o.flags = 1;
                now[env] = o;
            }
            continue;
        }
        const float rx = own_root[0], ry = own_root[1], rz = own_root[2];
        const int g0 = (env / gs) * gs;
        const float *own_caps = c.caps_ws + (long)env * EMLOCO_SC_MAXSEG * 8;
        float near_d = 0.0f, best_pen = 0.0f;
        int near_m = 0x7fffffff, best_key = 0x7fffffff, n_near = 0, n_pen = 0;
        for (int c0 = 0; c0 < gs; c0 += 64) {
            const int ml = c0 + lane, m = g0 + ml;
            bool valid = ml < gs && m != env, cand = false;
            float s[3] = {0.0f, 0.0f, 0.0f};
            if (valid) {
                const float *mr = c.roots_ws + (long)m * 4;
                const float bound_m = mr[3];
                valid = !(bound_m < 0.0f);
                if (valid) {
                    s[0] = mr[0] - rx; s[1] = mr[1] - ry; s[2] = mr[2] - rz;
                    const float d_xy = sqrtf(s[0] * s[0] + s[1] * s[1]);
                    if (near_m == 0x7fffffff || d_xy < near_d) { near_d = d_xy; near_m = m; }      // (members ascend within a lane)
                    cand = cc_norm3(s) <= (bound_e + bound_m) + kContactCullSlack;
                    valid = d_xy < c.near_dist;
                }
            }
            n_near += __popcll(__ballot(valid));
            unsigned long long todo = __ballot(cand);
            while (todo) {                                         // (wave-uniform)
                const int src0 = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const int src1 = todo ? __builtin_ctzll(todo) : -1;
                if (todo) todo &= todo - 1ull;
                const int src = (half && src1 >= 0) ? src1 : src0;
                const bool active = j < n_seg && (half == 0 || src1 >= 0);
                const float sx = __shfl(s[0], src), sy = __shfl(s[1], src), sz = __shfl(s[2], src);
                const int ml_c = c0 + src;                          // the member of this half wave, within the group
                const float *sj = c.caps_ws + ((long)(g0 + ml_c) * EMLOCO_SC_MAXSEG + (j < n_seg ? j : 0)) * 8;
                const float Q0[3] = {sj[0] + sx, sj[1] + sy, sj[2] + sz}, Q1[3] = {sj[4] + sx, sj[5] + sy, sj[6] + sz};
                const float rj = sj[3], hrj = sj[7] + kContactCullSlack;
                const float mj[3] = {0.5f * (Q0[0] + Q1[0]), 0.5f * (Q0[1] + Q1[1]), 0.5f * (Q0[2] + Q1[2])};
                bool hit = false;
                for (int i = 0; i < n_seg; ++i) {                  // (every lane: the same i)
                    const float *si = own_caps + i * 8;
                    const float A[3] = {si[0], si[1], si[2]}, B[3] = {si[4], si[5], si[6]};
                    const float dm[3] = {0.5f * (A[0] + B[0]) - mj[0], 0.5f * (A[1] + B[1]) - mj[1], 0.5f * (A[2] + B[2]) - mj[2]};
                    const float reach = si[7] + hrj;
                    if (!active || (dm[0] * dm[0] + dm[1] * dm[1]) + dm[2] * dm[2] > reach * reach) continue;
                    const float rs = si[3] + rj;
                    float c1[3], c2[3];
                    seg_seg_closest(A, B, Q0, Q1, c1, c2);
                    const float dv[3] = {c1[0] - c2[0], c1[1] - c2[1], c1[2] - c2[2]};
                    const float dist2 = (dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2];
                    if (dist2 < rs * rs) {
                        const float pen = rs - sqrtf(dist2);
                        hit = hit || pen > 0.0f;
                        if (pen > best_pen) { best_pen = pen; best_key = (ml_c << 10) | (i * n_seg + j); }
                    }
                }
                const unsigned long long hits = __ballot(hit);
                n_pen += ((hits & 0xffffffffull) != 0ull ? 1 : 0) + ((hits >> 32) != 0ull ? 1 : 0);
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(near_d, off), op = __shfl_xor(best_pen, off);
            const int om = __shfl_xor(near_m, off), ok = __shfl_xor(best_key, off);
            if (om != 0x7fffffff && (near_m == 0x7fffffff || od < near_d || (od == near_d && om < near_m))) { near_d = od; near_m = om; }
            if (op > best_pen || (op == best_pen && ok < best_key)) { best_pen = op; best_key = ok; }
        }
        if (lane == 0) {
            EmlocoCrowdContactNow o;
            const bool any = near_m != 0x7fffffff, touch = best_pen > 0.0f;
            const int p = best_key & 1023, i = p / n_seg, j = p - i * n_seg;
            o.nearest = any ? near_d : 0.0f;
            o.pen = touch ? best_pen : 0.0f;
            o.nearest_member = any ? near_m : -1;
            o.pen_member = touch ? g0 + (best_key >> 10) : -1;
            o.pen_segs = touch ? (i | (j << 8)) : -1;
            o.n_pen = n_pen; o.n_near = n_near; o.flags = 0;
            now[env] = o;
        }
    }
}

// the game's accumulators: EMLOCO_CROWD_CONTACT_WS words per env, all zeros at a game's start
struct CrowdContactGame {
    double sum_nearest;
    float min_nearest, max_pen;
    int32_t calls, steps, nonfinite_steps, neighbour_steps, near_steps, contact_steps, contacts;
    int32_t pen_member, pen_segs, pen_step, first_contact_step;       // first_contact_step 0: none yet
    int32_t _pad;
};
static_assert(sizeof(CrowdContactGame) == 4 * EMLOCO_CROWD_CONTACT_WS, "EMLOCO_CROWD_CONTACT_WS words hold a game's accumulators");

__global__ __launch_bounds__(256) void crowd_contact_accumulate_kernel(const EmlocoCrowdContacts c, const EmlocoCrowdContactNow *now) {
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (e >= c.n_env) return;
    CrowdContactGame *ws = (CrowdContactGame *)c.game_ws + e;
    CrowdContactGame g = *ws;
    const EmlocoCrowdContactNow n = now[e];
    const bool finite = (n.flags & 1) == 0, neighbour = finite && n.nearest_member >= 0;
    double *tot = c.totals ? c.totals + (long)e * EMLOCO_CROWD_CONTACT_TOTALS : nullptr;
    g.calls += 1;
    if (finite) g.steps += 1; else g.nonfinite_steps += 1;
    if (neighbour) {
        g.sum_nearest += (double)n.nearest;
        g.min_nearest = (g.neighbour_steps == 0 || n.nearest < g.min_nearest) ? n.nearest : g.min_nearest;
        g.neighbour_steps += 1;
        if (n.n_near > 0) g.near_steps += 1;
        if (n.n_pen > 0) {
            g.contact_steps += 1;
            g.contacts += n.n_pen;
            if (g.first_contact_step == 0) g.first_contact_step = g.calls;
            if (n.pen > g.max_pen) { g.max_pen = n.pen; g.pen_member = n.pen_member; g.pen_segs = n.pen_segs; g.pen_step = g.calls; }
        }
    }
    if (tot) {
        tot[EMLOCO_CCT_STEPS] += finite ? 1.0 : 0.0;
        tot[EMLOCO_CCT_NONFINITE_STEPS] += finite ? 0.0 : 1.0;
        if (neighbour) {
            const double d = (double)n.nearest, p = (double)n.pen;
            tot[EMLOCO_CCT_MIN_NEAREST] = (tot[EMLOCO_CCT_NEIGHBOUR_STEPS] == 0.0 || d < tot[EMLOCO_CCT_MIN_NEAREST]) ? d : tot[EMLOCO_CCT_MIN_NEAREST];
            tot[EMLOCO_CCT_NEIGHBOUR_STEPS] += 1.0;
            tot[EMLOCO_CCT_SUM_NEAREST] += d;
            tot[EMLOCO_CCT_NEAR_STEPS] += n.n_near > 0 ? 1.0 : 0.0;
            tot[EMLOCO_CCT_CONTACT_STEPS] += n.n_pen > 0 ? 1.0 : 0.0;
            tot[EMLOCO_CCT_CONTACTS] += (double)n.n_pen;
            tot[EMLOCO_CCT_SUM_PEN] += p;
            tot[EMLOCO_CCT_MAX_PEN] = p > tot[EMLOCO_CCT_MAX_PEN] ? p : tot[EMLOCO_CCT_MAX_PEN];
        }
    }
    const bool done = c.done8 ? c.done8[e] != 0 : (c.done64 ? c.done64[e] != 0 : false);
    if (done) {
        if (tot) {
            tot[EMLOCO_CCT_GAMES] += 1.0;
            tot[EMLOCO_CCT_GAMES_CONTACT] += g.contact_steps > 0 ? 1.0 : 0.0;
            tot[EMLOCO_CCT_GAMES_START_CONTACT] += g.first_contact_step == 1 ? 1.0 : 0.0;
        }
        if (c.records) {
            const int slot = c.slot[e];
            if (slot >= 0 && slot < c.games_per_env) {
                EmlocoCrowdContactRecord r;
                const bool touch = g.max_pen > 0.0f;
                r.min_nearest = g.neighbour_steps > 0 ? g.min_nearest : -1.0f;
                r.mean_nearest = g.neighbour_steps > 0 ? (float)(g.sum_nearest / (double)g.neighbour_steps) : 0.0f;
                r.max_pen = g.max_pen;
                r.steps = g.steps; r.nonfinite_steps = g.nonfinite_steps;
                r.near_steps = g.near_steps; r.contact_steps = g.contact_steps; r.contacts = g.contacts;
                r.pen_member = touch ? g.pen_member : -1; r.pen_segs = touch ? g.pen_segs : -1; r.pen_step = touch ? g.pen_step : -1;
                r.first_contact_step = g.first_contact_step > 0 ? g.first_contact_step : -1;
                c.records[(long)e * c.games_per_env + slot] = r;
            }
        }
        CrowdContactGame z;
        z.sum_nearest = 0.0; z.min_nearest = 0.0f; z.max_pen = 0.0f;
        z.calls = z.steps = z.nonfinite_steps = z.neighbour_steps = z.near_steps = z.contact_steps = z.contacts = 0;
        z.pen_member = z.pen_segs = z.pen_step = z.first_contact_step = z._pad = 0;
        g = z;
    }
    *ws = g;
}

// One workgroup: thread t sums the contiguous slots [t c, (t + 1) c) of records (env-major, game-minor; the recorded games only), then
// a pairwise tree in LDS in a fixed order, as locoval_track_reduce_kernel.
__global__ void __launch_bounds__(kContactReduceThreads)
crowd_contact_reduce_kernel(int n_env, int games_per_env, const EmlocoCrowdContactRecord *records, const int32_t *games, double *moments) {
    __shared__ double sm[EMLOCO_CROWD_CONTACT_MOMENTS][kContactReduceThreads];
    const int tid = (int)threadIdx.x;
    const long total = (long)n_env * games_per_env;
    const long c = (total + kContactReduceThreads - 1) / kContactReduceThreads;
    const long lo = tid * c, hi = (lo + c < total) ? lo + c : total;
    double m[EMLOCO_CROWD_CONTACT_MOMENTS];
    for (int k = 0; k < EMLOCO_CROWD_CONTACT_MOMENTS; ++k) m[k] = 0.0;
    for (long i = lo; i < hi; ++i) {
        const long e = i / games_per_env;
        const int g = (int)(i - e * games_per_env);
        if (g >= games[e]) continue;
        const EmlocoCrowdContactRecord r = records[i];
        m[EMLOCO_CCM_GAMES] += 1.0;
        m[EMLOCO_CCM_STEPS] += r.steps;
        m[EMLOCO_CCM_CONTACT_STEPS] += r.contact_steps;
        m[EMLOCO_CCM_NEAR_STEPS] += r.near_steps;
        m[EMLOCO_CCM_CONTACTS] += r.contacts;
        m[EMLOCO_CCM_NONFINITE_STEPS] += r.nonfinite_steps;
        if (r.contact_steps > 0) {
            const double p = r.max_pen;
            m[EMLOCO_CCM_GAMES_CONTACT] += 1.0;
            m[EMLOCO_CCM_GAMES_START_CONTACT] += r.first_contact_step == 1 ? 1.0 : 0.0;
            m[EMLOCO_CCM_SUM_MAX_PEN] += p;
            m[EMLOCO_CCM_SUM_MAX_PEN2] += p * p;
        }
        if (r.min_nearest >= 0.0f) {
            m[EMLOCO_CCM_GAMES_NEIGHBOUR] += 1.0;
            m[EMLOCO_CCM_SUM_MIN_NEAREST] += r.min_nearest;
            m[EMLOCO_CCM_SUM_MEAN_NEAREST] += r.mean_nearest;
        }
    }
    for (int k = 0; k < EMLOCO_CROWD_CONTACT_MOMENTS; ++k) sm[k][tid] = m[k];
    __syncthreads();
    for (int off = kContactReduceThreads / 2; off > 0; off >>= 1) {
        if (tid < off)
            for (int k = 0; k < EMLOCO_CROWD_CONTACT_MOMENTS; ++k) sm[k][tid] += sm[k][tid + off];
        __syncthreads();
    }
    if (tid < EMLOCO_CROWD_CONTACT_MOMENTS) moments[tid] = sm[tid][0];
}

__device__ __forceinline__ double cct_fold(int k, double x, double y) {
    if (k == EMLOCO_CCT_MIN_NEAREST) return y < x ? y : x;
    if (k == EMLOCO_CCT_MAX_PEN) return y > x ? y : x;
    return x + y;
}

// One workgroup, as episode_stats_reduce_kernel: thread t folds the contiguous envs [t c, (t + 1) c) in ascending order, then a pairwise
// tree in a fixed order, and clears the totals it has read.  The minimum only looks at envs with a neighbour step (+inf stands for
// "none" inside the tree; a vector without one carries 0).
__global__ void __launch_bounds__(kContactReduceThreads) crowd_contact_epoch_kernel(int n_env, double *totals, double *epoch) {
    __shared__ double sm[EMLOCO_CROWD_CONTACT_TOTALS][kContactReduceThreads];
    const int tid = (int)threadIdx.x;
    const int c = (n_env + kContactReduceThreads - 1) / kContactReduceThreads;
    const long lo = (long)tid * c, hi = (lo + c < n_env) ? lo + c : n_env;
    double m[EMLOCO_CROWD_CONTACT_TOTALS];
    for (int k = 0; k < EMLOCO_CROWD_CONTACT_TOTALS; ++k) m[k] = 0.0;
    m[EMLOCO_CCT_MIN_NEAREST] = __builtin_inf();
    for (long e = lo; e < hi; ++e) {
        double *tot = totals + e * EMLOCO_CROWD_CONTACT_TOTALS;
        const bool met = tot[EMLOCO_CCT_NEIGHBOUR_STEPS] > 0.0;
        for (int k = 0; k < EMLOCO_CROWD_CONTACT_TOTALS; ++k) {
            const double x = tot[k];
            if (k != EMLOCO_CCT_MIN_NEAREST || met) m[k] = cct_fold(k, m[k], x);
            tot[k] = 0.0;
        }
    }
    for (int k = 0; k < EMLOCO_CROWD_CONTACT_TOTALS; ++k) sm[k][tid] = m[k];
    __syncthreads();
    for (int off = kContactReduceThreads / 2; off > 0; off >>= 1) {
        if (tid < off)
            for (int k = 0; k < EMLOCO_CROWD_CONTACT_TOTALS; ++k) sm[k][tid] = cct_fold(k, sm[k][tid], sm[k][tid + off]);
        __syncthreads();
    }
    if (tid < EMLOCO_CROWD_CONTACT_TOTALS) {
        double v = sm[tid][0];
        if (tid == EMLOCO_CCT_MIN_NEAREST && !(sm[EMLOCO_CCT_NEIGHBOUR_STEPS][0] > 0.0)) v = 0.0;
        epoch[tid] = v;
    }
}

// what the four entry points refuse, by name (NULL: complete); host code, shared with the CPU emulation of the launches
inline const char *crowd_contacts_refusal(const EmlocoCrowdContacts *c, const void *now, bool accumulate) {
    if (!c) return "null structure";
    if (!now) return "null now";
    if (c->n_env < 1) return "n_env < 1";
    if (accumulate) {
        if (!c->game_ws) return "null game_ws";
        if (c->done8 && c->done64) return "done8 and done64 both given";
        if (c->records && !c->slot) return "records without slot";
        if (c->records && c->games_per_env < 1) return "records with games_per_env < 1";
        return nullptr;
    }
    if (c->group_size < 2) return "group_size < 2";
    if (c->n_env % c->group_size != 0) return "group_size does not divide n_env";
    if (c->n_seg < kContactBodies || c->n_seg > EMLOCO_SC_MAXSEG) return "n_seg outside 24 .. EMLOCO_SC_MAXSEG";
    if (!(c->near_dist > 0.0f) || !(c->near_dist <= 3.0e38f)) return "near_dist not finite and positive";
    if (!c->rb_state) return "null rb_state";
    if (!c->cap_a) return "null cap_a";
    if (!c->cap_b) return "null cap_b";
    if (!c->cap_r) return "null cap_r";
    if (!c->seg_body) return "null seg_body";
    if (!c->caps_ws) return "null caps_ws";
    if (!c->roots_ws) return "null roots_ws";
    return nullptr;
}

inline const char *crowd_contacts_reduce_refusal(int n_env, int games_per_env, const void *records, const void *games, const void *moments) {
    if (n_env < 1) return "n_env < 1";
    if (games_per_env < 1) return "games_per_env < 1";
    if (!records) return "null records";
    if (!games) return "null games";
    if (!moments) return "null moments";
    return nullptr;
}

}  // namespace emloco
