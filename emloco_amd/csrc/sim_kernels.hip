// sim_kernels.hip -- rigid-body step of the vectorised humanoid rollout for gfx950 (MI355X).
//
// Stands where the reference calls gym.simulate (pacer/pacer/env/tasks/base_task.py:792-797; engine
// parameters pacer/pacer/utils/config.py:143-163, pacer/pacer/data/cfg/pacer.yaml:93-104).  The reference's
// engine (PhysX 5) is absent; the scheme is this repo's own:
// articulated-body dynamics with implicit PD drives + maximal-coordinate ground contacts solved by
// projected Gauss-Seidel on the Gram-form contact matrix.
//
// Mapping: ONE 64-lane wave per env (workgroup = 1 wave, so __syncthreads() is free of cross-wave
// waits); all `n_sub` substeps of an env.step are fused in one launch and the env's state lives in
// LDS / registers between them.  Lane roles change per phase:
//   lane = body      (24 active)  kinematics, inertia, bias forces, articulated-body passes (level-synchronous)
//   lane = candidate (<=128, 2/lane) ground-contact detection, wave ballot + popcount compaction
//   lane = contact row (<=60)     chain propagation, contact-matrix column, Gauss-Seidel multiplier
// Gauss-Seidel row products are reduced on the DPP crossbar in a fixed association order (wave_sum), which is
// also the order the CPU oracle uses, so multipliers agree bit for bit.
//
// HBM traffic per env.step is ~9 KB (state in/out + per-env model), the kernel is latency/occupancy
// bound, not bandwidth bound.
#include <hip/hip_runtime.h>
#include "dev_math.h"
#include "sim_math.h"
// the rigid-body kernels use the fused helper set (sim_math.h); undone at the end of this file
#define cross3 fcross3
#define dot3 fdot3
#define dot6 fdot6
#define qmul fqmul
#define qnormalize fqnormalize
#define q2mat fq2mat
#define matvec3 fmatvec3
#define rotvec2quat frotvec2quat
#define quat2rotvec fquat2rotvec
#include "emloco_types.h"
#include "fk_device.h"
#include "order_device.h"
#include "sim_plan.h"

namespace emloco {

#define NB EMLOCO_NB
#define NDOF EMLOCO_NDOF
#define MAXC EMLOCO_MAXC
#define MAXR (3 * EMLOCO_MAXC)
#define MAXCAND EMLOCO_MAXCAND
#define EMLOCO_WH_MAX 1.0f /* largest link rotation per substep [rad]: 120 rad/s at h = 1/120 -- above the asset's max_angular_velocity = 100
                            * (humanoid.py:685-688), which is therefore the cap that binds (phase 1; 0.4 = 48 rad/s before the angular-momentum balance) */
#define YLEN 30 /* chain-propagation vector: 6 root + 3 per tree level (depth <= 8) */

// index into a packed symmetric 6x6 (upper triangle, row-major): (a<=b)
__device__ __forceinline__ constexpr int sidx(int a, int b) {
    return a <= b ? (a * (13 - a)) / 2 + (b - a) : (b * (13 - b)) / 2 + (a - b);
}

// (a, b) of a symmetric matrix stored as its packed lower triangle, branch-free
__device__ __forceinline__ int tri_index(int a, int b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    return ((hi * (hi + 1)) >> 1) + lo;
}

// the two layouts of the contact matrix in LDS (sim_step_env, phases 6b / 6c)
struct ContactMatrixSquare { static constexpr bool square = true; };
struct ContactMatrixPacked { static constexpr bool square = false; };
// the three entries (ls, r .. r + 2) of one contact: square layout -- three consecutive words at the lane's running row offset `ao`;
// packed lower triangle -- tri_index per entry
template <bool SQ>
__device__ __forceinline__ void contact_entries3(const float *sh_A, int ao, int ls, int r, float &x0, float &x1, float &x2) {
    if (SQ) { x0 = sh_A[ao]; x1 = sh_A[ao + 1]; x2 = sh_A[ao + 2]; }
    else { x0 = sh_A[tri_index(ls, r)]; x1 = sh_A[tri_index(ls, r + 1)]; x2 = sh_A[tri_index(ls, r + 2)]; }
}

// Hand-over of a split launch (emloco_sim_set_split): self-tagged 16-byte granules {a, tag, b, tag} -- each 8-byte half carries
// one payload word and the tag of the publishing part (EMLOCO_PART_TAG) -- written with `sc1` (write-through) stores and read
// with `sc1` loads, coherent across the XCDs' L2s and the CUs' L1s access by access (MI355X_MICROARCH.md, inter-workgroup
// visibility: "sc1 stores and loads both sides"; hand-off by data-tagged granules).  The producer stores and leaves: no drain,
// no flag.  The consumer loads all its granules in one burst and takes them when every half carries the awaited tag -- one
// memory round trip where the flag form took two (poll the flag, then load) behind the producer's s_waitcnt vmcnt(0).  Only the
// 8-byte halves are relied on to arrive whole (observed on gfx950, not an architectural guarantee), hence a tag in each.
// Layout of an env's block (EMLOCO_PART_WORDS), one lane address for every instruction:
//   granules [0, 128)    lane + 64 k, k = 0, 1: every lane -- a body lane's joint quaternion; lanes NB .. NB + 31 one 4-word
//                        group of LDS state each (root 4 | momentum 2 | multipliers 16 | slot map 8 | work | angular momentum)
//   granules [128, 200)  128 + lane + NB k, k = 0 .. 2: body lanes only -- joint rates | rotation vector
// Measured alternatives to sc1 accesses: agent-scope fences on every lane (__threadfence) write back / invalidate whole caches
// per workgroup: launch 0.54 -> 0.68 ms; one 4-byte agent atomic per word: every word is a fabric write of its own (HBM
// counters 46 -> 124 MB per launch).
typedef float part_f4 __attribute__((ext_vector_type(4)));
#define PART_G1 (64 * 4)              /* words from a lane's first granule to its second */
#define PART_GB (128 * 4)             /* first word of the body lanes' region */
static_assert(EMLOCO_PART_WORDS >= PART_GB + 3 * EMLOCO_NB * 4, "hand-over block too small for its layout");
#ifdef EMLOCO_EMU
__device__ __forceinline__ void part_st16(float *p, float a, float b, float c, float d) { p[0] = a; p[1] = b; p[2] = c; p[3] = d; }
__device__ __forceinline__ void part_ld80(const float *pa, const float *pb, float *v) {
    for (int k = 0; k < 4; ++k) { v[k] = pa[k]; v[4 + k] = pa[PART_G1 + k]; }
    for (int g = 0; g < 3; ++g) for (int k = 0; k < 4; ++k) v[8 + 4 * g + k] = pb[g * 4 * EMLOCO_NB + k];
}
__device__ __forceinline__ void part_err_raise(unsigned *e, unsigned bit) { if (e) *e |= bit; }
#else
__device__ __forceinline__ void part_st16(float *p, float a, float b, float c, float d) {
    const part_f4 v = {a, b, c, d};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(p), "v"(v) : "memory");
}
// a lane's two granules at pa and its three at pb (lanes without a body hand in pa again: loaded, never looked at)
__device__ __forceinline__ void part_ld80(const float *pa, const float *pb, float *v) {
    part_f4 a, b, c, e, f;
    static_assert(PART_G1 * 4 == 1024 && EMLOCO_NB * 16 == 384, "granule-major hand-over: the offsets of a lane's granules");
    asm volatile("global_load_dwordx4 %0, %5, off sc1\n\tglobal_load_dwordx4 %1, %5, off offset:1024 sc1\n\t"
                 "global_load_dwordx4 %2, %6, off sc1\n\tglobal_load_dwordx4 %3, %6, off offset:384 sc1\n\t"
                 "global_load_dwordx4 %4, %6, off offset:768 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(e), "=&v"(f) : "v"(pa), "v"(pb) : "memory");
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w; v[12] = e.x; v[13] = e.y; v[14] = e.z; v[15] = e.w;
    v[16] = f.x; v[17] = f.y; v[18] = f.z; v[19] = f.w;
}
__device__ __forceinline__ void part_err_raise(unsigned *e, unsigned bit) { if (e) __hip_atomic_fetch_or(e, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
#endif

// 16-byte load of a model record: base is workgroup-uniform (scalar registers), off a 32-bit lane offset in words
#ifdef EMLOCO_EMU
__device__ __forceinline__ void ld4(const float *base, int off, float *v) { for (int k = 0; k < 4; ++k) v[k] = base[off + k]; }
#else
__device__ __forceinline__ void ld4(const float *base, int off, float *v) {
    const part_f4 a = *(const part_f4 *)(base + off);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
#endif

// Register diet.  Everything a lane derives from its index alone (LDS row addresses at a dozen strides, model-record offsets,
// tree constants, the compare masks of the level loops) is launch-invariant, and the compiler hoists all of it out of the
// substep loop and keeps it in registers for the whole launch -- at 168 registers per lane (3 waves per SIMD) that was ~60
// spilled dwords.  Each phase therefore starts from a lane index the compiler cannot see through (an empty asm that
// redefines it): what a phase derives from it dies with the phase, and is recomputed (a handful of integer instructions)
// by the next one.  The tree constants of a body come from one packed LDS word per phase.
#ifdef EMLOCO_EMU
#define FRESH_LANE() do { } while (0)
#else
#define FRESH_LANE() asm volatile("" : "+v"(lane))
#endif
// pd_pack word (topology.h): parent | depth << 5 | index among the bodies of its depth << 9 | children << 12, 17, 22 (31: none)
#define PD_PARENT(w) ((w) & 31)
#define PD_DEPTH(w) (((w) >> 5) & 15)
#define PD_SLOT(w) (((w) >> 9) & 7)
#define PD_CHILD(w, i) (((w) >> (12 + 5 * (i))) & 31)

#ifdef EMLOCO_SIM_PROFILE
#define PSTAMP(i) do { if (d.prof && env == 0 && lane == 0) d.prof[sub * 16 + (i)] = (long long)wall_clock64(); FRESH_LANE(); } while (0)
#else
#define PSTAMP(i) FRESH_LANE()
#endif

// Schedule trace (diagnostic build -DEMLOCO_SIM_SCHED=1, tools/exp/sim_sched.py): with the start stamps switched on
// (emloco_sim_cost_ticks) every workgroup leaves four words in step_start [5 parts][n_env][4] -- wall clock at its first
// instruction, once its predecessor's hand-over is in, at its last instruction, and part | rank << 8 | workgroup index << 32.
#ifdef EMLOCO_SIM_SCHED
#define SCHED_HANDED() do { if (d.step_start && threadIdx.x == 0) d.step_start[((size_t)part * d.n_env + env) * 4 + 1] = (unsigned long long)wall_clock64(); } while (0)
#else
#define SCHED_HANDED() do { } while (0)
#endif

// Height-field ground under the world point (cx, cy): height zt of the cell triangle's plane there and its unit normal.
// Cell (i, j) holds the mesh triangles (v00, v10, v11) [u >= v] and (v00, v11, v01) [u < v] (u, v: position in the cell
// along x, y), as terrain_utils.convert_heightfield_to_trimesh lays them out; beyond the map the border cell's plane extends.
// `id` names the triangle that was used: (cell i, cell j, which half)
__device__ __forceinline__ void hf_plane(const EmlocoSimDev &d, float cx, float cy, float &zt, float n[3], int &id) {
    const float gx = (cx - d.hf_ox) * d.hf_inv_hs, gy = (cy - d.hf_oy) * d.hf_inv_hs;
    int i = (int)floorf(gx), j = (int)floorf(gy);
    i = i < 0 ? 0 : (i > d.hf_nx - 2 ? d.hf_nx - 2 : i);
    j = j < 0 ? 0 : (j > d.hf_ny - 2 ? d.hf_ny - 2 : j);
    const float u = gx - (float)i, v = gy - (float)j;
    id = ((i << 15) + j) * 2 + (u >= v ? 1 : 0);
    const short *c = d.hf + (long)i * d.hf_ny + j;
    const float h00 = d.hf_vs * (float)c[0], h01 = d.hf_vs * (float)c[1];
    const float h10 = d.hf_vs * (float)c[d.hf_ny], h11 = d.hf_vs * (float)c[d.hf_ny + 1];
    float zx, zy;
    if (u >= v) { zx = h10 - h00; zy = h11 - h10; } else { zy = h01 - h00; zx = h11 - h01; }
    zt = fmaf(v, zy, fmaf(u, zx, h00));
    const float sx = zx * d.hf_inv_hs, sy = zy * d.hf_inv_hs;
    const float inv = 1.0f / sqrtf(fmaf(sx, sx, fmaf(sy, sy, 1.0f)));
    n[0] = 0.0f - sx * inv; n[1] = 0.0f - sy * inv; n[2] = inv;
}
// the triangle under a point, without its plane
__device__ __forceinline__ int hf_triangle(const EmlocoSimDev &d, float cx, float cy) {
    const float gx = (cx - d.hf_ox) * d.hf_inv_hs, gy = (cy - d.hf_oy) * d.hf_inv_hs;
    int i = (int)floorf(gx), j = (int)floorf(gy);
    i = i < 0 ? 0 : (i > d.hf_nx - 2 ? d.hf_nx - 2 : i);
    j = j < 0 ? 0 : (j > d.hf_ny - 2 ? d.hf_ny - 2 : j);
    const float u = gx - (float)i, v = gy - (float)j;
    return ((i << 15) + j) * 2 + (u >= v ? 1 : 0);
}

// ---- the slope-corrected mesh (terrain_utils.convert_heightfield_to_trimesh with a slope threshold, built by the task at
// humanoid_pedestrain_terrain.py:859-881): where the step between two neighbouring samples exceeds the threshold the LOWER vertex
// sits one cell sideways, under the upper one -- the cell between them is a vertical face (a stair riser), the cell on the low
// side is stretched.  d.hf_mv carries the moves; xy in grid units (integers as floats), z in metres.
struct MeshV { float x, y, z; };
__device__ __forceinline__ MeshV mesh_vert(const EmlocoSimDev &d, int ci, int cj) {
    const long k = (long)ci * d.hf_ny + cj;
    const int b = d.hf_mv[k];
    MeshV v;
    v.x = (float)(ci + (b & 3) - 1); v.y = (float)(cj + ((b >> 2) & 3) - 1); v.z = d.hf_vs * (float)d.hf[k];
    return v;
}
// cell (ci, cj), triangle t: t = 0 (v00, v10, v11) [id half 1], t = 1 (v00, v11, v01) [id half 0]: the mesh's winding, normals out of the solid
__device__ __forceinline__ void mesh_tri(const EmlocoSimDev &d, int ci, int cj, int t, MeshV &A, MeshV &B, MeshV &Cc) {
    A = mesh_vert(d, ci, cj);
    if (t == 0) { B = mesh_vert(d, ci + 1, cj); Cc = mesh_vert(d, ci + 1, cj + 1); }
    else { B = mesh_vert(d, ci + 1, cj + 1); Cc = mesh_vert(d, ci, cj + 1); }
}
// The mesh surface under the world point (cx, cy): the highest of the (at most 18) triangles of the 3 x 3 cells around the point's
// regular cell that cover it.  Cells whose 4 x 4 vertex block carries no move take the regular-grid formula (bit-equal to the
// uncorrected height field), and so do points no triangle covers (beyond the map).
__device__ __noinline__ void mesh_plane(const EmlocoSimDev &d, float cx, float cy, float &zt, float n[3], int &id) {
    if (!d.hf_mv) { hf_plane(d, cx, cy, zt, n, id); return; }
    const float gx = (cx - d.hf_ox) * d.hf_inv_hs, gy = (cy - d.hf_oy) * d.hf_inv_hs;
    int i = (int)floorf(gx), j = (int)floorf(gy);
    i = i < 0 ? 0 : (i > d.hf_nx - 2 ? d.hf_nx - 2 : i);
    j = j < 0 ? 0 : (j > d.hf_ny - 2 ? d.hf_ny - 2 : j);
    if (!(d.hf_mv[(long)i * d.hf_ny + j] & 16)) { hf_plane(d, cx, cy, zt, n, id); return; }
    bool found = false;
    int bid = 0;
    float bz = 0.0f, bsx = 0.0f, bsy = 0.0f;
    for (int a = -1; a <= 1; ++a) {
        const int ci = i + a;
        if (ci < 0 || ci > d.hf_nx - 2) continue;
        for (int b = -1; b <= 1; ++b) {
            const int cj = j + b;
            if (cj < 0 || cj > d.hf_ny - 2) continue;
            for (int t = 0; t < 2; ++t) {
                MeshV A, B, Cc;
                mesh_tri(d, ci, cj, t, A, B, Cc);
                const float bx = B.x - A.x, by = B.y - A.y, qx = Cc.x - A.x, qy = Cc.y - A.y;
                const float ar = bx * qy - by * qx;
                if (ar == 0.0f) continue;                                   // collapsed: a vertical face, see mesh_walls
                const float px = gx - A.x, py = gy - A.y;
                const float eb = px * qy - py * qx, ec = bx * py - by * px;
                const bool in = ar > 0.0f ? (eb >= 0.0f && ec >= 0.0f && eb + ec <= ar) : (eb <= 0.0f && ec <= 0.0f && eb + ec >= ar);
                if (!in) continue;
                const float zb = B.z - A.z, zc = Cc.z - A.z;
                const float sx = (zb * qy - zc * by) / ar, sy = (zc * bx - zb * qx) / ar;
                const float z = fmaf(py, sy, fmaf(px, sx, A.z));
                if (!found || z > bz) { found = true; bz = z; bsx = sx; bsy = sy; bid = ((ci << 15) + cj) * 2 + (t == 0 ? 1 : 0); }
            }
        }
    }
    if (!found) { hf_plane(d, cx, cy, zt, n, id); return; }
    zt = bz; id = bid;
    const float sx = bsx * d.hf_inv_hs, sy = bsy * d.hf_inv_hs;
    const float inv = 1.0f / sqrtf(fmaf(sx, sx, fmaf(sy, sy, 1.0f)));
    n[0] = 0.0f - sx * inv; n[1] = 0.0f - sy * inv; n[2] = inv;
}
__device__ __forceinline__ float dot3f(const float *a, const float *b) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }
// The vertical faces of the mesh near the world point P (centre of a contact sphere): every collapsed triangle of the 3 x 3 cells
// around P's regular cell, closest point by regions (vertex, edge, face).  dsel / nsel hold the signed distance of P to the nearest
// surface found so far and its normal (>= 0: P is outside the terrain solid).  Outside: a face P is in front of wins when it is
// nearer, normal from its closest point to P.  Inside: a face P is behind wins when the foot of P's perpendicular lies in it and
// it is nearer than the surface above, normal = the face's.
__device__ __noinline__ void mesh_walls(const EmlocoSimDev &d, const float P[3], float &dsel, float nsel[3]) {
    const float gx = (P[0] - d.hf_ox) * d.hf_inv_hs, gy = (P[1] - d.hf_oy) * d.hf_inv_hs;
    int i = (int)floorf(gx), j = (int)floorf(gy);
    i = i < 0 ? 0 : (i > d.hf_nx - 2 ? d.hf_nx - 2 : i);
    j = j < 0 ? 0 : (j > d.hf_ny - 2 ? d.hf_ny - 2 : j);
    if (!(d.hf_mv[(long)i * d.hf_ny + j] & 16)) return;
    for (int a = -1; a <= 1; ++a) {
        const int ci = i + a;
        if (ci < 0 || ci > d.hf_nx - 2) continue;
        for (int b = -1; b <= 1; ++b) {
            const int cj = j + b;
            if (cj < 0 || cj > d.hf_ny - 2) continue;
            for (int t = 0; t < 2; ++t) {
                MeshV A, B, Cc;
                mesh_tri(d, ci, cj, t, A, B, Cc);
                if ((B.x - A.x) * (Cc.y - A.y) - (B.y - A.y) * (Cc.x - A.x) != 0.0f) continue;
                // corners relative to P, metres
                const float va[3] = {fmaf(A.x, d.hf_hs, d.hf_ox) - P[0], fmaf(A.y, d.hf_hs, d.hf_oy) - P[1], A.z - P[2]};
                const float vb[3] = {fmaf(B.x, d.hf_hs, d.hf_ox) - P[0], fmaf(B.y, d.hf_hs, d.hf_oy) - P[1], B.z - P[2]};
                const float vc[3] = {fmaf(Cc.x, d.hf_hs, d.hf_ox) - P[0], fmaf(Cc.y, d.hf_hs, d.hf_oy) - P[1], Cc.z - P[2]};
                const float ab[3] = {vb[0] - va[0], vb[1] - va[1], vb[2] - va[2]}, ac[3] = {vc[0] - va[0], vc[1] - va[1], vc[2] - va[2]};
                const float fn[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
                const float fn2 = dot3f(fn, fn);
                if (fn2 == 0.0f) continue;                                  // no area in space either
                // closest point q of the triangle to the origin (= P), by regions
                const float ap[3] = {0.0f - va[0], 0.0f - va[1], 0.0f - va[2]}, bp[3] = {0.0f - vb[0], 0.0f - vb[1], 0.0f - vb[2]};
                const float cp[3] = {0.0f - vc[0], 0.0f - vc[1], 0.0f - vc[2]};
                const float d1 = dot3f(ab, ap), d2 = dot3f(ac, ap), d3 = dot3f(ab, bp), d4 = dot3f(ac, bp), d5 = dot3f(ab, cp), d6 = dot3f(ac, cp);
                float q[3];
                bool face = false;
                const float vcc = d1 * d4 - d3 * d2, vbb = d5 * d2 - d1 * d6, vaa = d3 * d6 - d5 * d4;
                if (d1 <= 0.0f && d2 <= 0.0f) { q[0] = va[0]; q[1] = va[1]; q[2] = va[2]; }
                else if (d3 >= 0.0f && d4 <= d3) { q[0] = vb[0]; q[1] = vb[1]; q[2] = vb[2]; }
                else if (vcc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { const float w = d1 / (d1 - d3); for (int k = 0; k < 3; ++k) q[k] = fmaf(w, ab[k], va[k]); }
                else if (d6 >= 0.0f && d5 <= d6) { q[0] = vc[0]; q[1] = vc[1]; q[2] = vc[2]; }
                else if (vbb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { const float w = d2 / (d2 - d6); for (int k = 0; k < 3; ++k) q[k] = fmaf(w, ac[k], va[k]); }
                else if (vaa <= 0.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f) {
                    const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
                    for (int k = 0; k < 3; ++k) q[k] = fmaf(w, vc[k] - vb[k], vb[k]);
                } else {
                    const float den = 1.0f / (vaa + vbb + vcc), v = vbb * den, w = vcc * den;
                    for (int k = 0; k < 3; ++k) q[k] = fmaf(w, ac[k], fmaf(v, ab[k], va[k]));
                    face = true;
                }
                const float dv[3] = {0.0f - q[0], 0.0f - q[1], 0.0f - q[2]};
                const float side = dot3f(dv, fn);
                const float ifn = 1.0f / sqrtf(fn2);
                if (dsel >= 0.0f) {
                    const float dist = sqrtf(dot3f(dv, dv));
                    if (side >= 0.0f && dist < dsel) {
                        dsel = dist;
                        if (dist > 1.0e-6f) { const float id_ = 1.0f / dist; for (int k = 0; k < 3; ++k) nsel[k] = dv[k] * id_; }
                        else for (int k = 0; k < 3; ++k) nsel[k] = fn[k] * ifn;
                    }
                } else if (side < 0.0f && face) {
                    const float dw = side * ifn;
                    if (dw > dsel) { dsel = dw; for (int k = 0; k < 3; ++k) nsel[k] = fn[k] * ifn; }
                }
            }
        }
    }
}

#ifndef EMLOCO_SIM_WAVES_PER_SIMD
#define EMLOCO_SIM_WAVES_PER_SIMD 3   /* register budget 168 per lane and 12.4 KB of LDS per env: three resident waves per SIMD, 12 envs per CU */
#endif
// one env's step: the body of both kernels below (one 64-lane wave)
template <int HF>
__device__ __forceinline__ void sim_step_env(const EmlocoSimParams &prm, const EmlocoSimDev &d, const int env, int &work, const SimPlanWork &pw) {
    int lane = threadIdx.x;                                   // redefined at every phase boundary (FRESH_LANE)
    work = 0;                                                 // contact work of this step: sum over substeps of (10 + contacts) where there are any

    // ---------------------------------------------------------------- LDS: one blob, 13.0 KB per env (12 envs per CU need <= 13.3 KB)
    // Every per-body row starts on a 16-byte boundary and is padded to a multiple of four words, so a lane moves its row with
    // ds_read_b128 / ds_write_b128 (R | r share a 12-word row; 6-vectors take 8 words, 21-word inertias 24, W 20).
    // Persistent part first, then the region G whose members are live in different phases of a substep:
    //   Ia (articulated inertias)   phase 3 only; its first 180 words hold the contact frames (height field) from phase 5 to 7
    //   pa   phases 3 and 7         a    phases 3-4 and 7
    //   V                           phase 1 -> end of 4   Vf   end of 4 -> 6a        Aacc phase 1 -> 2     fext phase 1b -> 2
    //   pq (world position | quaternion)   phase 1 -> 5, and the final pass
    // (body inertias and bias forces never reach LDS: phase 2b leaves them in the lane's registers for its level of phase 3.)
    // The contact matrix (1830 words, phases 6b-6c: everything above is dead then) lies over [Ia tail .. pq] and 90 words
    // past it, the staged Jacobian rows of phase 7 (720 words) over [Ia tail .. a] -- dead again before pa / a are written --
    // and the limb-limb scratch (phase 1b) over [Ia tail .. a].  Barriers separate the phases.
    enum { O_ROOT = 0, O_P = 16, O_V0 = 24, O_L = 36, O_PD = 48, O_R = O_PD + NB, O_W = O_R + NB * 12,
           O_L0 = O_W + NB * 24, O_CB = O_L0 + 44, O_CX = O_CB + MAXC / 4 + 3, O_CDIST = O_CX + 3 * MAXC, O_LAM = O_CDIST + MAXC,
           O_SLOT = O_LAM + MAXR, O_CRANGE = O_SLOT + 32, O_IA = O_CRANGE + 2 * NB / 4, O_G = O_IA + 180,
           O_PA = O_IA + NB * 24, O_A_ = O_PA + NB * 8, O_V = O_A_ + NB * 8,
           O_VF = O_V + NB * 8, O_AACC = O_VF + NB * 8, O_FEXT = O_AACC + NB * 8, O_PQ = O_FEXT + NB * 8,
           LDS_WORDS = (O_PQ + NB * 8 > O_G + MAXR * (MAXR + 1) / 2) ? O_PQ + NB * 8 : O_G + MAXR * (MAXR + 1) / 2 };
    static_assert(O_R % 4 == 0 && O_W % 4 == 0 && O_IA % 4 == 0 && O_PA % 4 == 0 && O_PQ % 4 == 0, "rows must be 16-byte aligned");
    static_assert(O_V - O_G >= EMLOCO_SC_MAXSEG * 8 + EMLOCO_SC_MAXHITS * 8 + 256, "limb-limb scratch does not fit its overlay");
    static_assert(LDS_WORDS * 4 <= 13312, "LDS per env above 160 KiB / 12 in 512-byte granules (three waves per SIMD, 12 envs per CU)");
    // The contact matrix has two layouts, chosen per env-substep on the contact count (wave-uniform): up to SQ_MAXC contacts
    // the full square, entry (s, r) at s * SQ_LD + r, both triangles stored -- a lane walks its own row with one running
    // address; above, the packed lower triangle (a 60 x 60 square does not fit).  The odd stride keeps the 64 lanes of a column
    // walk on different banks.  The sweeps read one contact past the last one (never used): three words beyond a row.
    enum { SQ_MAXC = 14, SQ_ROWS = 3 * SQ_MAXC, SQ_LD = SQ_ROWS + 1 };
    static_assert(SQ_ROWS * SQ_LD <= LDS_WORDS - O_G && (SQ_ROWS - 1) * SQ_LD + SQ_ROWS + 3 <= LDS_WORDS - O_G,
                  "the square contact matrix (and the read one contact ahead of its last row) does not fit the matrix region");
    static_assert(SQ_ROWS > 32 && SQ_ROWS <= 64 && SQ_MAXC <= MAXC, "square layout: at most two tile rows of the Gram build");
    __shared__ __attribute__((aligned(16))) float lds[LDS_WORDS];
    float *sh_root = lds + O_ROOT;                            // p0[3] q0[4] V0[6]
    float *sh_V0 = lds + O_V0;                                // lane 0's hand-over between phases: free root twist [0..5], impulse change [6..11]
    float *sh_P = lds + O_P;                                  // linear momentum: expected [0..2], of the current substep [3..5]; total mass [6]
    float *sh_L = lds + O_L;                                  // angular momentum about the centre of mass: expected [0..2], "a balance exists" [3] (1 / 0), of the current substep [4..6]; centre of mass relative to O [8..10]
    int *sh_pd = (int *)(lds + O_PD);                         // per body: tree constants, packed (PD_PARENT / PD_DEPTH / PD_SLOT / PD_CHILD)
    float (*sh_R)[12] = (float (*)[12])(lds + O_R);           // rotation matrix [0..8] | position relative to O [9..11]
    float (*sh_W)[24] = (float (*)[24])(lds + O_W);           // per joint: W = U K^T (6 x 3) [0..17] | K, the inverse Cholesky factor of D (packed lower) [18..23]
    float *sh_L0 = lds + O_L0, *sh_L0i = lds + O_L0 + 36;    // root Cholesky factor and 1 / its diagonal
    unsigned char *sh_cbody = (unsigned char *)(lds + O_CB);  // body of each contact (bytes)
    float (*sh_cx)[3] = (float (*)[3])(lds + O_CX);
    float *sh_cdist = lds + O_CDIST;
    float *sh_lam = lds + O_LAM;                              // per contact row: warm-start multiplier (6a), solved multiplier (after 6c)
    signed char *sh_crange = (signed char *)(lds + O_CRANGE); // per body (bytes): first [0..NB) and last [NB..2NB) contact of the current substep
    unsigned char *sh_slot = (unsigned char *)(lds + O_SLOT); // per candidate: its contact slot of the latest substep (255: none)
    float (*sh_Ia)[24] = (float (*)[24])(lds + O_IA);
    float (*sh_cdir)[9] = (float (*)[9])(lds + O_IA);        // contact frames [normal | tangent 1 | tangent 2] (height-field ground)
    float (*sh_pa)[8] = (float (*)[8])(lds + O_PA);
    float (*sh_a)[8] = (float (*)[8])(lds + O_A_);
    float (*sh_V)[8] = (float (*)[8])(lds + O_V);
    float (*sh_Vf)[8] = (float (*)[8])(lds + O_VF);
    float (*sh_Aacc)[8] = (float (*)[8])(lds + O_AACC);
    float (*sh_fext)[8] = (float (*)[8])(lds + O_FEXT);      // limb-limb penalty wrench per body (self-collision), about O
    float (*sh_pq)[8] = (float (*)[8])(lds + O_PQ);          // world position [0..2] | world rotation quaternion [4..7]
    float *sh_A = lds + O_G;                                  // contact matrix: square (s, r) at s * SQ_LD + r up to SQ_MAXC contacts, else lower triangle: (r, s<=r) at r(r+1)/2 + s
    constexpr bool hf_on = HF != 0;          // compile time: the plane instantiation carries none of the height-field code

    // ---------------------------------------------------------------- per-lane constants
    const int *topo = d.topo;
    // This env's model block and state rows: workgroup-uniform bases (scalar registers) + 32-bit lane offsets.  Model
    // constants, drive gains and targets are re-read (L2 hits) where they are used instead of pinned in registers for the launch.
    const float *mdl = d.model + (size_t)env * EMLOCO_MODEL_WORDS;
#define o_dyn (EMLOCO_MB_DYN + (lane < NB ? lane : 0) * 16)                                     /* this body's dynamics record */
#define jdof ((lane >= 1 && lane < NB) ? (lane - 1) * 3 : 0)                                  /* first dof of this body's joint */
#define o_drv (EMLOCO_MB_DRV + jdof * 4)
    const float *tgt_env = d.pd_target + (size_t)env * NDOF;
    float *dofs_env = d.dof_state + (size_t)env * NDOF * 2;
    float *cf_env = d.contact_force + (size_t)env * NB * 3;
    float *lws_env = d.lambda_ws + (size_t)env * MAXCAND * 3;
    // Part prologue: what does not depend on the predecessor is requested BEFORE the hand-over is polled -- the topology word and
    // the model record of the first substep's phase 1 (joint offset | mass) -- and is in flight during the wait; the topology
    // word reaches LDS behind it.
    const int pd_w = lane < NB ? topo[EMLOCO_TOPO_PDPACK + lane] : 0;
    float jm[4];                                     // joint offset xyz | body mass
    ld4(mdl, o_dyn, jm);
    sh_slot[lane] = 255; sh_slot[lane + 64] = 255;

    // ---------------------------------------------------------------- state -> registers
    // Split launch: the substeps [sub_lo, sub_hi) of this workgroup; part 0 starts from the state tensors like the whole
    // step, a later part continues from what its predecessor left (joint quaternions / rates / rotation vectors per lane,
    // root, momentum balance, multipliers and their slot map: plain copies, so the parts together are the fused step bit
    // for bit).  Parts are workgroups of ONE launch, the later ones at higher indices: the wave slots that the first
    // parts of short envs free early are taken by second parts instead of idling until the launch's last workgroup ends.
    // Which substeps, and whether the workgroup takes a hand-over, leaves one or finishes the step, is the launch's part plan
    // (sim_plan.h): the uniform split, or the table of emloco_sim_set_plan -- there a part may hold two substeps, or none: the
    // tail part, which enters the loop once for the final kinematics pass and writes back.
    const int part = pw.part(), sub_lo = pw.sub_lo, sub_hi = pw.sub_hi;
    float *pst = d.part_state ? d.part_state + (long)env * EMLOCO_PART_WORDS : nullptr;
    // (the rotation vectors edof could wait in LDS -- they are read twice per substep -- but 96 more words put the 13th KB on the
    // env's LDS and cost the twelfth resident env per CU: measured slower than letting the compiler park them in scratch)
    float qj[4] = {0, 0, 0, 1}, wj[3] = {0, 0, 0}, edof[3] = {0, 0, 0};
    if (!pw.consumes()) {
        if ((lane < NB) && lane >= 1) {
            const float *ds = dofs_env + jdof * 2;
            float e[3] = {ds[0], ds[2], ds[4]};
            rotvec2quat(e, qj);
            wj[0] = ds[1]; wj[1] = ds[3]; wj[2] = ds[5];
            quat2rotvec(qj, edof);
        }
        if (lane == 0) {
            const float *rs = d.root_state + (long)env * 13;
            float q0[4] = {rs[3], rs[4], rs[5], rs[6]};
            qnormalize(q0);
            for (int k = 0; k < 3; ++k) { sh_root[k] = rs[k]; sh_root[7 + k] = rs[10 + k]; sh_root[10 + k] = rs[7 + k]; }
            for (int k = 0; k < 4; ++k) sh_root[3 + k] = q0[k];
        }
    } else {
        // The predecessor publishes its state as self-tagged granules (see part_ld80).  Parts are workgroups of one launch at
        // ascending indices, so in dispatch order the granules are there long before and the first burst takes them; the wait
        // is bounded all the same (a lost hand-over must not hang the device) and a wait that runs out is an ERROR, not a
        // reason to go on from stale hand-over state: the workgroup raises the device error word (emloco_sim_sync / the next
        // step return EMLOCO_E_HIP) and abandons this env's step.  Every lane loads its own granules and checks their tags;
        // the ballot makes the verdict wave-uniform, so no lane leaves the loop on its own.
        const unsigned want = EMLOCO_PART_TAG(d.part_seq, part - 1);
        const float *pa = pst + lane * 4, *pb = lane < NB ? pst + PART_GB + lane * 4 : pa;
        float v[20];
        int spins = 0;
        bool bad;
        for (;;) {
            part_ld80(pa, pb, v);
            bool miss = __float_as_uint(v[1]) != want || __float_as_uint(v[3]) != want || __float_as_uint(v[5]) != want || __float_as_uint(v[7]) != want;
            if (lane < NB)
                for (int k = 9; k < 20; k += 2) miss = miss || __float_as_uint(v[k]) != want;
            bad = __ballot(miss) != 0ull;
            if (!bad || ++spins >= d.part_spin_max) break;
            __builtin_amdgcn_s_sleep(16);
        }
        if (bad) {
            if (lane == 0) part_err_raise(d.err, EMLOCO_ERR_PART_TIMEOUT);
            work = -1;
            return;
        }
        if ((lane < NB)) {          // joint quaternion | rates | rotation vector
            qj[0] = v[0]; qj[1] = v[2]; qj[2] = v[4]; qj[3] = v[6];
            wj[0] = v[8]; wj[1] = v[10]; wj[2] = v[12];
            edof[0] = v[14]; edof[1] = v[16]; edof[2] = v[18];
        } else if (lane < NB + 32) {   // one 4-word group of LDS state per lane: root (4) | momentum (2) | multipliers (16) | slot map (8) | work | angular momentum
            const int g = lane - NB;
            float *dst = g < 4 ? sh_root + 4 * g : g < 6 ? sh_P + 4 * (g - 4) : g < 22 ? sh_lam + 4 * (g - 6) : g < 30 ? (float *)sh_slot + 4 * (g - 22) : sh_L;
            if (g != 30) { dst[0] = v[0]; dst[1] = v[2]; dst[2] = v[4]; dst[3] = v[6]; }
        }
        work = __shfl(__float_as_int(v[0]), NB + 30);          // the work counter so far
    }
    if (lane < NB) sh_pd[lane] = pd_w;
    __syncthreads();
    SCHED_HANDED();

    const float h = prm.h;
    // registers that persist across phases (lane = body)
    // (R, r, V of a body live in LDS; the motion-subspace columns S = [R e_c ; r x R e_c] are re-formed where needed)
    float tau[3], dd[3];
    int sat[3];            // 0: implicit drive; +1 / -1: constant torque at +/- the effort limit; 2: effort drive (the command, clipped).
                           // With it the torque report of the last substep needs no tau: three registers fewer across the contact phases
    float uh[3], qdd[3];

    for (int sub = sub_lo; sub < sub_hi + (pw.final() ? 1 : 0); ++sub) {
        const bool final_pass = (sub == prm.n_sub);   // kinematics only, to write the body states
        const bool last = (sub == prm.n_sub - 1);

        PSTAMP(0);
        // ============================================================ 1. kinematics + velocities (root -> leaves)
        if (lane == 0) {
            float q0[4] = {sh_root[3], sh_root[4], sh_root[5], sh_root[6]}, R[9];
            q2mat(q0, R);
            for (int k = 0; k < 3; ++k) { sh_pq[0][k] = sh_root[k]; sh_R[0][9 + k] = 0.0f; }
            for (int k = 0; k < 4; ++k) sh_pq[0][4 + k] = q0[k];
            for (int k = 0; k < 9; ++k) sh_R[0][k] = R[k];
            for (int k = 0; k < 6; ++k) { sh_V[0][k] = sh_root[7 + k]; sh_Aacc[0][k] = 0.0f; }
        }
        // joint offsets | mass (jm): re-read per substep (L2 hit) instead of held for the launch -- requested ahead of the hand-over
        // (the prologue) or at the end of the substep before, so that the round trip is not paid here
        const float joff[3] = {jm[0], jm[1], jm[2]};
        __syncthreads();
        const int pd1 = sh_pd[lane < NB ? lane : 0];
        for (int lev = 1; lev <= d.max_depth; ++lev) {
            if ((lane < NB) && PD_DEPTH(pd1) == lev) {
                const int p = PD_PARENT(pd1);
                float Rp[9], o[3], qp[4], qw[4], pw[3], R[9], r[3], Sl[3][3], V[6];
                for (int k = 0; k < 9; ++k) Rp[k] = sh_R[p][k];
                for (int k = 0; k < 4; ++k) qp[k] = sh_pq[p][4 + k];
                matvec3(Rp, joff, o);
                for (int k = 0; k < 3; ++k) { pw[k] = sh_pq[p][k] + o[k]; r[k] = pw[k] - sh_root[k]; }
                qmul(qp, qj, qw);
                qnormalize(qw);
                q2mat(qw, R);
                float wv[3], Vp[6];
                for (int k = 0; k < 6; ++k) Vp[k] = sh_V[p][k];
                for (int c = 0; c < 3; ++c) {
                    float ax[3] = {R[c], R[3 + c], R[6 + c]};
                    cross3(r, ax, Sl[c]);
                }
                for (int k = 0; k < 3; ++k) {
                    wv[k] = SOP3(R[k * 3], wj[0], R[k * 3 + 1], wj[1], R[k * 3 + 2], wj[2]);
                    V[k] = Vp[k] + wv[k];
                    V[3 + k] = Vp[3 + k] + SOP3(Sl[0][k], wj[0], Sl[1][k], wj[1], Sl[2][k], wj[2]);
                }
                // velocity-product acceleration c = [w_p x wv ; vj x wv + r x (w_p x wv)]
                float t[3], vj[3], cc[6], t1[3], t2[3];
                cross3(V, r, t);
                for (int k = 0; k < 3; ++k) vj[k] = V[3 + k] + t[k];
                cross3(Vp, wv, cc);
                cross3(vj, wv, t1);
                cross3(r, cc, t2);
                for (int k = 0; k < 3; ++k) cc[3 + k] = t1[k] + t2[k];
                for (int k = 0; k < 3; ++k) { sh_pq[lane][k] = pw[k]; sh_R[lane][9 + k] = r[k]; }
                for (int k = 0; k < 4; ++k) sh_pq[lane][4 + k] = qw[k];
                for (int k = 0; k < 9; ++k) sh_R[lane][k] = R[k];
                for (int k = 0; k < 6; ++k) { sh_V[lane][k] = V[k]; sh_Aacc[lane][k] = sh_Aacc[p][k] + cc[k]; }
            }
            __syncthreads();
        }
        // Link angular-speed limit.  The reference caps link angular velocities (AssetOptions.max_angular_velocity = 100,
        // humanoid.py:685-688); here the cap is min(that, EMLOCO_WH_MAX / h): the velocity-product terms are integrated
        // explicitly and beyond ~0.4 rad per substep they pump energy into fast spinning links.  When the fastest link of the
        // env exceeds the cap (rare, wave-uniform), root angular velocity and joint rates are scaled down uniformly so that
        // link just meets it, and the root's linear velocity is shifted so the linear momentum is unchanged:
        // V_i -> [sc w_i ; v_0' + sc (v_i - v_0)], v_0' = v_0 + (1 - sc)(v_com - v_0); the velocity-product accelerations
        // are quadratic in the angular rates.
        if (!final_pass) {
            float w2 = 0.0f;
            if ((lane < NB)) { const float *Vb = sh_V[lane]; w2 = fmaf(Vb[0], Vb[0], fmaf(Vb[1], Vb[1], Vb[2] * Vb[2])); }
            for (int off = 32; off >= 1; off >>= 1) { const float o = __shfl_xor(w2, off); w2 = o > w2 ? o : w2; }
            float wlim = EMLOCO_WH_MAX / h;
            if (prm.max_ang_vel < wlim) wlim = prm.max_ang_vel;
            if (w2 > wlim * wlim) {
                const float sc = wlim / sqrtf(w2), sc2 = sc * sc;
                float lm = 0.0f, lp[3] = {0.0f, 0.0f, 0.0f};
                if ((lane < NB)) {
                    float Rb[9], cm[4], cw[3], rc[3], wx[3], Vb[6];
                    for (int k = 0; k < 9; ++k) Rb[k] = sh_R[lane][k];
                    ld4(mdl, o_dyn + 4, cm);
                    for (int k = 0; k < 6; ++k) Vb[k] = sh_V[lane][k];
                    matvec3(Rb, cm, cw);
                    for (int k = 0; k < 3; ++k) rc[k] = sh_R[lane][9 + k] + cw[k];
                    cross3(Vb, rc, wx);
                    lm = jm[3];
                    for (int k = 0; k < 3; ++k) lp[k] = lm * (Vb[3 + k] + wx[k]);
                }
                const float M = wave_sum(lm);
                float v0[3], v0n[3];
                for (int k = 0; k < 3; ++k) { v0[k] = sh_root[10 + k]; v0n[k] = v0[k] + (1.0f - sc) * (wave_sum(lp[k]) / M - v0[k]); }
                __syncthreads();
                if ((lane < NB)) {
                    for (int k = 0; k < 3; ++k) { sh_V[lane][k] *= sc; sh_V[lane][3 + k] = v0n[k] + sc * (sh_V[lane][3 + k] - v0[k]); }
                    for (int k = 0; k < 6; ++k) sh_Aacc[lane][k] *= sc2;
                    if (lane >= 1) for (int k = 0; k < 3; ++k) wj[k] *= sc;
                }
                if (lane == 0) for (int k = 0; k < 3; ++k) { sh_root[7 + k] *= sc; sh_root[10 + k] = v0n[k]; sh_L[k] *= sc; }   // (every angular rate scaled: so is L about c)
                __syncthreads();
            }
        }

        // Linear-momentum balance.  The integrator is first order in the velocity products, so the velocity of the centre
        // of mass of a tumbling body would drift (measured: 5 % of g t in a tumbling free fall).  The total linear momentum is
        // therefore carried across the substeps of a launch -- P_exp = P + h (M g + sum of the contact forces), all known
        // exactly -- and the momentum the new generalized velocities actually have (known once the kinematics of the new
        // configuration are: here, and in the final pass that writes the body states) is shifted onto it by a uniform change
        // dv of the linear velocities.  The velocity-product accelerations see dv through v_i x S_i qd_i: + dv x (w_i - w_0).
        {
            float lm = 0.0f, lp[3] = {0.0f, 0.0f, 0.0f}, Vb[6] = {0, 0, 0, 0, 0, 0};
            if ((lane < NB)) {
                float Rb[9], cm[4], cw[3], rc[3], wx[3];
                for (int k = 0; k < 9; ++k) Rb[k] = sh_R[lane][k];
                ld4(mdl, o_dyn + 4, cm);
                for (int k = 0; k < 6; ++k) Vb[k] = sh_V[lane][k];
                matvec3(Rb, cm, cw);
                for (int k = 0; k < 3; ++k) rc[k] = sh_R[lane][9 + k] + cw[k];
                cross3(Vb, rc, wx);
                lm = jm[3];
                for (int k = 0; k < 3; ++k) lp[k] = lm * (Vb[3 + k] + wx[k]);
            }
            const float Mtot = wave_sum(lm);
            float Pact[3];
            for (int k = 0; k < 3; ++k) Pact[k] = wave_sum(lp[k]);
            if (sub > 0) {                                       // wave-uniform: a balance exists from the previous substep
                float dv[3];
                for (int k = 0; k < 3; ++k) dv[k] = (sh_P[k] - Pact[k]) / Mtot;
                if ((lane < NB)) {
                    const float wr[3] = {Vb[0] - sh_V[0][0], Vb[1] - sh_V[0][1], Vb[2] - sh_V[0][2]};
                    float t[3];
                    cross3(dv, wr, t);
                    for (int k = 0; k < 3; ++k) { sh_Aacc[lane][3 + k] += t[k]; sh_V[lane][3 + k] = Vb[3 + k] + dv[k]; }
                }
                if (lane == 0) for (int k = 0; k < 3; ++k) { sh_root[10 + k] += dv[k]; sh_P[3 + k] = sh_P[k]; }
            } else if (lane == 0) {
                for (int k = 0; k < 3; ++k) sh_P[3 + k] = Pact[k];
            }
            if (lane == 0) sh_P[6] = Mtot;
            __syncthreads();
            // Angular-momentum balance (oracle_sim.c: project_angular_momentum).  The velocity products are integrated explicitly: a
            // free body tumbling at 13 rad/s gained 50 % kinetic energy a second, which is why links used to be capped at 48 rad/s.
            // Like the linear momentum, the angular momentum about the centre of mass c is carried across the substeps of a launch --
            // L_exp = damp (L + sum of (x - c) x contact impulse) -- and what the new generalized velocities have in the new
            // configuration is moved onto it by a rigid rotation rate dw of the whole body about c: J dw = L_exp - L (J: composite
            // inertia about c, joints locked), every body twist gains [dw ; c x dw] about O -- the linear momentum is untouched.
            {
                // the twelve wave sums are taken about O (none waits for another) and moved to c afterwards:
                // L_c = L_O - c x P,  J_c = J_O - M ((c.c) E - c c^T)
                float lc[3] = {0.0f, 0.0f, 0.0f}, ll[3] = {0.0f, 0.0f, 0.0f}, lj[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, Vn[6] = {0, 0, 0, 0, 0, 0};
                if ((lane < NB)) {
                    float Rb[9], cm[4], cw[3], rcb[3], wx[3], vcb[3], in6[8], Rc[9], Ic[6], ru[3], Iw[3];
                    for (int k = 0; k < 9; ++k) Rb[k] = sh_R[lane][k];
                    ld4(mdl, o_dyn + 4, cm);
                    ld4(mdl, o_dyn + 8, in6); ld4(mdl, o_dyn + 12, in6 + 4);
                    for (int k = 0; k < 6; ++k) Vn[k] = sh_V[lane][k];
                    matvec3(Rb, cm, cw);
                    for (int k = 0; k < 3; ++k) rcb[k] = sh_R[lane][9 + k] + cw[k];
                    cross3(Vn, rcb, wx);
                    for (int k = 0; k < 3; ++k) vcb[k] = Vn[3 + k] + wx[k];
                    const float Ib[9] = {in6[0], in6[3], in6[4], in6[3], in6[1], in6[5], in6[4], in6[5], in6[2]};
                    for (int a = 0; a < 3; ++a)
                        for (int q = 0; q < 3; ++q) Rc[a * 3 + q] = SOP3(Rb[a * 3], Ib[q], Rb[a * 3 + 1], Ib[3 + q], Rb[a * 3 + 2], Ib[6 + q]);
                    const int ja[6] = {0, 1, 2, 0, 0, 1}, jb[6] = {0, 1, 2, 1, 2, 2};          // upper triangle: 00 11 22 01 02 12
                    for (int e = 0; e < 6; ++e) {
                        const int a = ja[e], q = jb[e];
                        Ic[e] = SOP3(Rc[a * 3], Rb[q * 3], Rc[a * 3 + 1], Rb[q * 3 + 1], Rc[a * 3 + 2], Rb[q * 3 + 2]);
                    }
                    cross3(rcb, vcb, ru);
                    Iw[0] = SOP3(Ic[0], Vn[0], Ic[3], Vn[1], Ic[4], Vn[2]);
                    Iw[1] = SOP3(Ic[3], Vn[0], Ic[1], Vn[1], Ic[5], Vn[2]);
                    Iw[2] = SOP3(Ic[4], Vn[0], Ic[5], Vn[1], Ic[2], Vn[2]);
                    const float rr = dot3(rcb, rcb);
                    for (int k = 0; k < 3; ++k) { lc[k] = lm * rcb[k]; ll[k] = Iw[k] + lm * ru[k]; }
                    for (int e = 0; e < 6; ++e) {
                        const int a = ja[e], q = jb[e];
                        lj[e] = Ic[e] + lm * ((a == q ? rr : 0.0f) - rcb[a] * rcb[q]);
                    }
                }
                float Cc[3], LO[3], JO[6], Lact[3], Jc[6], cP[3];
                for (int k = 0; k < 3; ++k) Cc[k] = wave_sum(lc[k]) / Mtot;
                for (int k = 0; k < 3; ++k) LO[k] = wave_sum(ll[k]);
                for (int e = 0; e < 6; ++e) JO[e] = wave_sum(lj[e]);
                {
                    const float Pc[3] = {sh_P[3], sh_P[4], sh_P[5]};
                    cross3(Cc, Pc, cP);
                    for (int k = 0; k < 3; ++k) Lact[k] = LO[k] - cP[k];
                    const int ja[6] = {0, 1, 2, 0, 0, 1}, jb[6] = {0, 1, 2, 1, 2, 2};
                    const float cc = dot3(Cc, Cc);
                    for (int e = 0; e < 6; ++e) Jc[e] = JO[e] - Mtot * ((ja[e] == jb[e] ? cc : 0.0f) - Cc[ja[e]] * Cc[jb[e]]);
                }
                const bool havL = sub > 0 && sh_L[3] != 0.0f;        // wave-uniform
                float dw[3] = {0.0f, 0.0f, 0.0f}, dvO[3] = {0.0f, 0.0f, 0.0f};
                bool moved = false;
                if (havL) {
                    const float b0 = sh_L[0] - Lact[0], b1 = sh_L[1] - Lact[1], b2 = sh_L[2] - Lact[2];
                    const float c00 = Jc[1] * Jc[2] - Jc[5] * Jc[5], c01 = Jc[4] * Jc[5] - Jc[3] * Jc[2], c02 = Jc[3] * Jc[5] - Jc[4] * Jc[1];
                    const float c11 = Jc[0] * Jc[2] - Jc[4] * Jc[4], c12 = Jc[3] * Jc[4] - Jc[0] * Jc[5], c22 = Jc[0] * Jc[1] - Jc[3] * Jc[3];
                    const float det = SOP3(Jc[0], c00, Jc[3], c01, Jc[4], c02);
                    if (det > 1e-12f) {
                        dw[0] = SOP3(c00, b0, c01, b1, c02, b2) / det;
                        dw[1] = SOP3(c01, b0, c11, b1, c12, b2) / det;
                        dw[2] = SOP3(c02, b0, c12, b1, c22, b2) / det;
                        cross3(Cc, dw, dvO);
                        moved = true;
                    }
                }
                __syncthreads();                                      // every lane has read sh_L / sh_P / sh_V
                if (moved && (lane < NB))
                    for (int k = 0; k < 3; ++k) { sh_V[lane][k] = Vn[k] + dw[k]; sh_V[lane][3 + k] = Vn[3 + k] + dvO[k]; }
                if (lane == 0) {
                    if (moved) for (int k = 0; k < 3; ++k) { sh_root[7 + k] += dw[k]; sh_root[10 + k] += dvO[k]; }
                    for (int k = 0; k < 3; ++k) { sh_L[4 + k] = moved ? sh_L[k] : Lact[k]; sh_L[8 + k] = Cc[k]; }
                }
                __syncthreads();
            }
        }
        if (final_pass) break;
        // drive gains and targets of phase 2: requested here, a phase ahead, so that the limb-limb phase covers the round trip
        float drv[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}, tgv[3] = {0, 0, 0};    // kp, kd, armature, effort limit | target of each dof
        if ((lane < NB))
            for (int k = 0; k < 3; ++k) { ld4(mdl, o_drv + 4 * k, drv[k]); tgv[k] = tgt_env[jdof + k]; }

        // ============================================================ 1b. limb-limb contacts (self-collision, penalty)
        // lane = body: world collision capsule -> LDS; lane = pair (4 rounds of 64): closest points, spring-damper force;
        // hits are compacted in pair order (ballot) and every body adds the wrenches that act on it in that order.
        if (d.sc_n > 0) {
            // lane = collision segment: one sphere-swept segment per body, and a second one for a box much wider than thick (the
            // ankle boxes: two capsules along the long edges); the segment's record names its body
            float *sh_seg = sh_A;                                  // [MAXSEG][8]   (sh_A is free until the contact phase)
            float *sh_hitw = sh_A + EMLOCO_SC_MAXSEG * 8;          // [MAXHITS][6] wrench on body i about O (body j gets the negative)
            int *sh_hitb = (int *)(sh_A + EMLOCO_SC_MAXSEG * 8 + EMLOCO_SC_MAXHITS * 6);   // [MAXHITS][2]
            if (lane < d.sc_nseg) {
                float R[9], r[3], ca[4], cb[4], pa[3], pb[3];
                ld4(mdl, EMLOCO_MB_CAP + lane * 8, ca); ld4(mdl, EMLOCO_MB_CAP + lane * 8 + 4, cb);     // end a xyz, radius | end b xyz, body
                const int sb = (int)cb[3];
                for (int k = 0; k < 9; ++k) R[k] = sh_R[sb][k];
                for (int k = 0; k < 3; ++k) r[k] = sh_R[sb][9 + k];
                matvec3(R, ca, pa); matvec3(R, cb, pb);
                for (int k = 0; k < 3; ++k) { sh_seg[lane * 8 + k] = r[k] + pa[k]; sh_seg[lane * 8 + 3 + k] = r[k] + pb[k]; }
                sh_seg[lane * 8 + 6] = ca[3];
                const float ax[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
                sh_seg[lane * 8 + 7] = 0.5f * sqrtf(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);      // half length of the capsule's segment
            }
            __syncthreads();
            // broad phase: two capsules can only touch when their segment midpoints are closer than the two radii plus the two
            // half lengths (triangle inequality; 1 mm of slack covers the rounding): the pairs that pass -- a few dozen of the
            // 245 -- are compacted in pair order and only they run the closest-point test, in one round instead of four.
            // A culled pair cannot hit, so the hit list (and every force) is what the full sweep gives.
            int *sh_cand = (int *)(sh_A + EMLOCO_SC_MAXSEG * 8 + EMLOCO_SC_MAXHITS * 8);
            int ncand = 0;
            for (int q0 = 0; q0 < d.sc_n; q0 += 64) {
                const int q = q0 + lane;
                bool keep = false;
                if (q < d.sc_n) {
                    const int pr = topo[EMLOCO_TOPO_SCPAIR + q], bi = pr & 0xff, bj = (pr >> 8) & 0xff;      // segments
                    float dm2 = 0.0f;
                    for (int k = 0; k < 3; ++k) {
                        const float dm = (sh_seg[bi * 8 + k] + sh_seg[bi * 8 + 3 + k]) - (sh_seg[bj * 8 + k] + sh_seg[bj * 8 + 3 + k]);   // 2 (m_i - m_j)
                        dm2 += dm * dm;
                    }
                    const float bound = (sh_seg[bi * 8 + 6] + sh_seg[bj * 8 + 6]) + (sh_seg[bi * 8 + 7] + sh_seg[bj * 8 + 7]) + 1e-3f;
                    keep = dm2 <= 4.0f * bound * bound;
                }
                const unsigned long long bal = __ballot(keep);
                if (keep) sh_cand[ncand + __popcll(bal & ((1ull << lane) - 1ull))] = q;
                ncand += __popcll(bal);
            }
            __syncthreads();
            int nh = 0;
            for (int c0 = 0; c0 < ncand; c0 += 64) {
                const int q = (c0 + lane < ncand) ? sh_cand[c0 + lane] : d.sc_n;
                bool hit = false;
                float w6[6] = {0, 0, 0, 0, 0, 0};
                int bi = 0, bj = 0;
                if (q < d.sc_n) {
                    const int pr = topo[EMLOCO_TOPO_SCPAIR + q];
                    const int si = pr & 0xff, sj = (pr >> 8) & 0xff;                 // the two segments ...
                    bi = (pr >> 16) & 0xff; bj = (pr >> 24) & 0xff;                  // ... and the bodies they belong to
                    float p0[3], p1[3], g0[3], g1[3], c1[3], c2[3];
                    for (int k = 0; k < 3; ++k) { p0[k] = sh_seg[si * 8 + k]; p1[k] = sh_seg[si * 8 + 3 + k]; g0[k] = sh_seg[sj * 8 + k]; g1[k] = sh_seg[sj * 8 + 3 + k]; }
                    const float rsum = sh_seg[si * 8 + 6] + sh_seg[sj * 8 + 6];
                    seg_seg_closest(p0, p1, g0, g1, c1, c2);
                    const float dv[3] = {c1[0] - c2[0], c1[1] - c2[1], c1[2] - c2[2]};
                    const float dist2 = dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2];
                    if (dist2 < rsum * rsum && dist2 > 1e-12f) {
                        const float dist = sqrtf(dist2);
                        float pen = rsum - dist;
                        const float n[3] = {dv[0] / dist, dv[1] / dist, dv[2] / dist};
                        const float off = sh_seg[sj * 8 + 6] - 0.5f * pen;     // contact point: middle of the overlap
                        const float pt[3] = {c2[0] + n[0] * off, c2[1] + n[1] * off, c2[2] + n[2] * off};
                        float Vi[6], Vj[6], wi[3], wjx[3];
                        for (int k = 0; k < 6; ++k) { Vi[k] = sh_V[bi][k]; Vj[k] = sh_V[bj][k]; }
                        cross3(Vi, pt, wi); cross3(Vj, pt, wjx);
                        const float vn = ((Vi[3] + wi[0]) - (Vj[3] + wjx[0])) * n[0] + ((Vi[4] + wi[1]) - (Vj[4] + wjx[1])) * n[1]
                                       + ((Vi[5] + wi[2]) - (Vj[5] + wjx[2])) * n[2];
                        if (pen > d.sc_max_pen) pen = d.sc_max_pen;
                        float F = d.sc_k * pen - d.sc_c * vn;
                        if (F > 0.0f) {
                            float Fv[3] = {n[0] * F, n[1] * F, n[2] * F};
                            if (d.sc_mu > 0.0f) {      // Coulomb friction capped by the contact's damper: - min(mu F / |v_t|, c) v_t
                                const float vr[3] = {(Vi[3] + wi[0]) - (Vj[3] + wjx[0]), (Vi[4] + wi[1]) - (Vj[4] + wjx[1]),
                                                     (Vi[5] + wi[2]) - (Vj[5] + wjx[2])};
                                const float vt[3] = {vr[0] - vn * n[0], vr[1] - vn * n[1], vr[2] - vn * n[2]};
                                const float vt2 = vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2];
                                if (vt2 > 1e-12f) {
                                    float g = d.sc_mu * F / sqrtf(vt2);
                                    if (g > d.sc_c) g = d.sc_c;
                                    for (int k = 0; k < 3; ++k) Fv[k] -= g * vt[k];
                                }
                            }
                            cross3(pt, Fv, w6);
                            w6[3] = Fv[0]; w6[4] = Fv[1]; w6[5] = Fv[2];
                            hit = true;
                        }
                    }
                }
                const unsigned long long bal = __ballot(hit);
                const int slot = nh + __popcll(bal & ((1ull << lane) - 1ull));
                if (hit && slot < EMLOCO_SC_MAXHITS) {
                    for (int k = 0; k < 6; ++k) sh_hitw[slot * 6 + k] = w6[k];
                    sh_hitb[slot * 2] = bi; sh_hitb[slot * 2 + 1] = bj;
                }
                nh += __popcll(bal);
            }
            if (nh > EMLOCO_SC_MAXHITS) nh = EMLOCO_SC_MAXHITS;
            __syncthreads();
            if ((lane < NB)) {
                float fe[6] = {0, 0, 0, 0, 0, 0};
                for (int hh = 0; hh < nh; ++hh) {
                    const int bi = sh_hitb[hh * 2], bj = sh_hitb[hh * 2 + 1];
                    if (bi == lane) for (int k = 0; k < 6; ++k) fe[k] += sh_hitw[hh * 6 + k];
                    else if (bj == lane) for (int k = 0; k < 6; ++k) fe[k] -= sh_hitw[hh * 6 + k];
                }
                for (int k = 0; k < 6; ++k) sh_fext[lane][k] = fe[k];
            }
            __syncthreads();                                       // the scratch in sh_A is overwritten by phase 2
        }

        PSTAMP(1);
        // ============================================================ 2. drive
        if ((lane < NB)) {
            // implicit PD drive: tau~ = kp (q* - q) - (kd + h kp) qd, joint-space diagonal d = armature + h kd + h^2 kp
            for (int k = 0; k < 3; ++k) {
                const float *dr = drv[k];                        // kp, kd, armature, effort limit of this dof
                const float kp = lane >= 1 ? dr[0] : 0.0f, kd = lane >= 1 ? dr[1] : 0.0f;
                const float arm = lane >= 1 ? dr[2] : 0.0f, tgt = lane >= 1 ? tgv[k] : 0.0f;
                const float e = tgt - edof[k];
                if (prm.drive_mode == 1) {       // effort drive (gymapi.DOF_MODE_EFFORT): the given torque within the limit, nothing implicit
                    const float eff = lane >= 1 ? dr[3] : 0.0f;
                    sat[k] = 2; tau[k] = tgt > eff ? eff : (tgt < -eff ? -eff : tgt); dd[k] = arm;
                } else {
                    sat[k] = 0; tau[k] = kp * e - (kd + h * kp) * wj[k]; dd[k] = arm + h * kd + h * h * kp;
                }
            }
        }

        PSTAMP(2);
#if defined(EMLOCO_DUMMY_VALU) || defined(EMLOCO_DUMMY_LDS) || defined(EMLOCO_DUMMY_SALU)
        {   // sensitivity probes (diagnostic builds only): extra instructions of one kind per substep, results discarded
#ifdef EMLOCO_DUMMY_VALU
            float z0 = h, z1 = h + 1.0f, z2 = h + 2.0f, z3 = h + 3.0f;
            for (int i = 0; i < EMLOCO_DUMMY_VALU / 4; ++i)
                asm volatile("v_fma_f32 %0, %0, %0, %1\n\tv_fma_f32 %1, %1, %1, %2\n\tv_fma_f32 %2, %2, %2, %3\n\tv_fma_f32 %3, %3, %3, %0"
                             : "+v"(z0), "+v"(z1), "+v"(z2), "+v"(z3));
            if (z0 + z1 + z2 + z3 == 12345.678f) sh_V0[11] = z0;
#endif
#ifdef EMLOCO_DUMMY_LDS
            part_f4 q0, q1, q2, q3;
            const unsigned la = (unsigned)(lane & 15) * 48u + (unsigned)(O_R * 4);
            for (int i = 0; i < EMLOCO_DUMMY_LDS / 4; ++i)
                asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b128 %2, %4 offset:32\n\tds_read_b128 %3, %4 offset:64\n\ts_waitcnt lgkmcnt(0)"
                             : "=v"(q0), "=v"(q1), "=v"(q2), "=v"(q3) : "v"(la) : "memory");
            if (q0.x + q1.x + q2.x + q3.x == 12345.678f) sh_V0[11] = q0.x;
#endif
#ifdef EMLOCO_DUMMY_SALU
            int c0 = sub, c1 = sub + 1;
            for (int i = 0; i < EMLOCO_DUMMY_SALU / 4; ++i)
                asm volatile("s_add_i32 %0, %0, %1\n\ts_xor_b32 %1, %1, %0\n\ts_add_i32 %0, %0, 7\n\ts_xor_b32 %1, %1, 5" : "+s"(c0), "+s"(c1));
            if (c0 + c1 == 123456789) sh_V0[11] = 1.0f;
#endif
        }
#endif
        // Phases 3-4 run once with every drive implicit.  The torque such a drive delivers over the substep is
        // tau~ - (h kd + h^2 kp) qdd; where that exceeds the effort limit the drive becomes a constant torque at the limit
        // (no implicit terms) and the env repeats the two phases once (rare: wave-uniform branch per env).
        float pA[6];
        int cand_w[2] = {0, 0};              // topology words of this lane's two ground-contact candidates (phase 5)
        for (int pass = 0; pass < 2; ++pass) {
        // ============================================================ 2b. inertia about O and bias force of every body (lane = body)
        // They stay in this lane's registers until its level of the up pass below takes them over in place -- no trip through
        // LDS (768 words per env, which is what let a third wave per SIMD in); the rare second pass recomputes them.
        float IA[21];
        for (int k = 0; k < 21; ++k) IA[k] = 0.0f;
        if ((lane < NB)) {
            float R[9], r[3], V[6];
            for (int k = 0; k < 9; ++k) R[k] = sh_R[lane][k];
            for (int k = 0; k < 3; ++k) r[k] = sh_R[lane][9 + k];
            for (int k = 0; k < 6; ++k) V[k] = sh_V[lane][k];
            float Rc[9], Ic[9], cw[3], c[3], in6[8], bcom[4];
            ld4(mdl, o_dyn + 8, in6); ld4(mdl, o_dyn + 12, in6 + 4);            // mass properties: re-read per substep (L2 hits)
            ld4(mdl, o_dyn + 4, bcom);
            const float bmass = mdl[o_dyn + 3];
            const float Ib[9] = {in6[0], in6[3], in6[4], in6[3], in6[1], in6[5], in6[4], in6[5], in6[2]};
            for (int a = 0; a < 3; ++a)
                for (int q = 0; q < 3; ++q) Rc[a * 3 + q] = SOP3(R[a * 3], Ib[q], R[a * 3 + 1], Ib[3 + q], R[a * 3 + 2], Ib[6 + q]);
            for (int a = 0; a < 3; ++a)
                for (int q = a; q < 3; ++q) {
                    Ic[a * 3 + q] = SOP3(Rc[a * 3], R[q * 3], Rc[a * 3 + 1], R[q * 3 + 1], Rc[a * 3 + 2], R[q * 3 + 2]);
                    Ic[q * 3 + a] = Ic[a * 3 + q];
                }
            matvec3(R, bcom, cw);
            for (int k = 0; k < 3; ++k) c[k] = r[k] + cw[k];
            const float ms = bmass, cc = dot3(c, c);
            for (int a = 0; a < 3; ++a)
                for (int q = a; q < 3; ++q) IA[sidx(a, q)] = Ic[a * 3 + q] + ms * ((a == q ? cc : 0.0f) - c[a] * c[q]);
            const float cx[9] = {0.0f, -c[2], c[1], c[2], 0.0f, -c[0], -c[1], c[0], 0.0f};
            for (int a = 0; a < 3; ++a)
                for (int q = 0; q < 3; ++q) IA[sidx(a, 3 + q)] = ms * cx[a * 3 + q];
            for (int a = 0; a < 3; ++a)
                for (int q = a; q < 3; ++q) IA[sidx(3 + a, 3 + q)] = (a == q) ? ms : 0.0f;
            float Aa[6], hI[6], IAc[6], x1[3], x2[3];
            for (int k = 0; k < 6; ++k) Aa[k] = sh_Aacc[lane][k];
            for (int a = 0; a < 6; ++a) {
                const float Ir[6] = {IA[sidx(a, 0)], IA[sidx(a, 1)], IA[sidx(a, 2)], IA[sidx(a, 3)], IA[sidx(a, 4)], IA[sidx(a, 5)]};
                hI[a] = fdot6(Ir, V);
                IAc[a] = fdot6(Ir, Aa);
            }
            cross3(V, hI, x1); cross3(V + 3, hI + 3, x2);
            for (int k = 0; k < 3; ++k) pA[k] = IAc[k] + x1[k] + x2[k];
            cross3(V, hI + 3, x1);
            for (int k = 0; k < 3; ++k) pA[3 + k] = IAc[3 + k] + x1[k];
            float fg[3] = {0.0f, 0.0f, ms * prm.gravity_z}, ng[3];
            cross3(c, fg, ng);
            for (int k = 0; k < 3; ++k) { pA[k] -= ng[k]; pA[3 + k] -= fg[k]; }
            if (d.sc_n > 0) for (int k = 0; k < 6; ++k) pA[k] -= sh_fext[lane][k];     // external wrench: f -= [p x F ; F]
        }
        // ============================================================ 3. articulated-body factorisation + up pass (leaves -> root)
        const int pd3 = sh_pd[lane < NB ? lane : 0];
        for (int lev = d.max_depth; lev >= 0; --lev) {
            if ((lane < NB) && PD_DEPTH(pd3) == lev) {
                float Wm[18], Km[6];
                float R[9], r[3], Sl[3][3];
                for (int k = 0; k < 9; ++k) R[k] = sh_R[lane][k];
                for (int k = 0; k < 3; ++k) r[k] = sh_R[lane][9 + k];
                for (int c = 0; c < 3; ++c) { const float ax[3] = {R[c], R[3 + c], R[6 + c]}; cross3(r, ax, Sl[c]); }
                for (int ci = 0; ci < 3; ++ci) {     // children in descending body index
                    const int ch = PD_CHILD(pd3, ci);
                    if (ch != 31) {
                        for (int k = 0; k < 21; ++k) IA[k] += sh_Ia[ch][k];
                        for (int k = 0; k < 6; ++k) pA[k] += sh_pa[ch][k];
                    }
                }
                if (lev > 0) {
                    float U[18], D[9];
                    for (int c = 0; c < 3; ++c) {
                        const float Sc[6] = {R[c], R[3 + c], R[6 + c], Sl[c][0], Sl[c][1], Sl[c][2]};
                        for (int a = 0; a < 6; ++a)
                        { const float Ir[6] = {IA[sidx(a, 0)], IA[sidx(a, 1)], IA[sidx(a, 2)], IA[sidx(a, 3)], IA[sidx(a, 4)], IA[sidx(a, 5)]}; U[a * 3 + c] = fdot6(Ir, Sc); }
                    }
                    for (int a = 0; a < 3; ++a) {
                        const float Sa[6] = {R[a], R[3 + a], R[6 + a], Sl[a][0], Sl[a][1], Sl[a][2]};
                        for (int q = 0; q < 3; ++q) {
                            float acc = 0.0f;
                            for (int k = 0; k < 6; ++k) acc = fmaf(Sa[k], U[k * 3 + q], acc);
                            D[a * 3 + q] = acc + (a == q ? dd[a] : 0.0f);
                        }
                    }
                    // reciprocals of the pivots first: the off-diagonal entries multiply instead of divide
                    const float l00 = sqrtf(D[0]), k00 = 1.0f / l00, l10 = D[3] * k00, l20 = D[6] * k00;
                    const float l11 = sqrtf(fmaf(-l10, l10, D[4])), k11 = 1.0f / l11, l21 = fmaf(-l20, l10, D[7]) * k11;
                    const float l22 = sqrtf(fmaf(-l21, l21, fmaf(-l20, l20, D[8]))), k22 = 1.0f / l22;
                    const float k10 = -l10 * k00 * k11, k21 = -l21 * k11 * k22, k20 = -SOP2(l20, k00, l21, k10) * k22;
                    Km[0] = k00; Km[1] = k10; Km[2] = k11; Km[3] = k20; Km[4] = k21; Km[5] = k22;
                    for (int a = 0; a < 6; ++a) {
                        Wm[a * 3 + 0] = U[a * 3] * k00;
                        Wm[a * 3 + 1] = SOP2(U[a * 3], k10, U[a * 3 + 1], k11);
                        Wm[a * 3 + 2] = SOP3(U[a * 3], k20, U[a * 3 + 1], k21, U[a * 3 + 2], k22);
                    }
                    float u[3];
                    for (int c = 0; c < 3; ++c) {
                        const float Sc[6] = {R[c], R[3 + c], R[6 + c], Sl[c][0], Sl[c][1], Sl[c][2]};
                        u[c] = tau[c] - fdot6(Sc, pA);
                    }
                    uh[0] = Km[0] * u[0];
                    uh[1] = SOP2(Km[1], u[0], Km[2], u[1]);
                    uh[2] = SOP3(Km[3], u[0], Km[4], u[1], Km[5], u[2]);
                    for (int a = 0; a < 6; ++a)
                        for (int q = a; q < 6; ++q)
                            sh_Ia[lane][sidx(a, q)] = SUB_SOP3(IA[sidx(a, q)], Wm[a * 3], Wm[q * 3], Wm[a * 3 + 1], Wm[q * 3 + 1], Wm[a * 3 + 2], Wm[q * 3 + 2]);
                    for (int k = 0; k < 6; ++k)
                        sh_pa[lane][k] = ADD_SOP3(pA[k], Wm[k * 3], uh[0], Wm[k * 3 + 1], uh[1], Wm[k * 3 + 2], uh[2]);
                    for (int k = 0; k < 18; ++k) sh_W[lane][k] = Wm[k];
                    for (int k = 0; k < 6; ++k) sh_W[lane][18 + k] = Km[k];
                } else {
                    // root: Cholesky of the 6x6 articulated inertia, a0 = -IA0^-1 pA0
                    float L[21], Li[6];    // lower triangle, (a, q<=a) at a(a+1)/2 + q; reciprocal pivots
#define LT(a, q) L[(a) * ((a) + 1) / 2 + (q)]
                    for (int a = 0; a < 6; ++a)
                        for (int q = 0; q <= a; ++q) {
                            float acc = IA[sidx(a, q)];
                            for (int k = 0; k < q; ++k) acc = fmaf(-LT(a, k), LT(q, k), acc);
                            if (a == q) { LT(a, q) = sqrtf(acc); Li[a] = 1.0f / LT(a, q); }
                            else LT(a, q) = acc * Li[q];
                        }
                    float y[6], x[6];
                    for (int a = 0; a < 6; ++a) {
                        float acc = -pA[a];
                        for (int k = 0; k < a; ++k) acc = fmaf(-LT(a, k), y[k], acc);
                        y[a] = acc * Li[a];
                    }
                    for (int a = 5; a >= 0; --a) {
                        float acc = y[a];
                        for (int k = a + 1; k < 6; ++k) acc = fmaf(-LT(k, a), x[k], acc);
                        x[a] = acc * Li[a];
                    }
                    for (int a = 0; a < 6; ++a)
                        for (int q = 0; q <= a; ++q) sh_L0[a * 6 + q] = LT(a, q);
                    for (int a = 0; a < 6; ++a) sh_L0i[a] = Li[a];
#undef LT
                    for (int k = 0; k < 6; ++k) sh_a[0][k] = x[k];
                }
            }
            __syncthreads();
        }

        PSTAMP(3);
        // ============================================================ 4. down pass: joint accelerations, v_free
        // drive gains and limits for the effort check behind the down pass: requested ahead of it (the level loop covers the round trip)
        float drc[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        if (pass == 0 && (lane < NB) && lane >= 1)
            for (int k = 0; k < 3; ++k) ld4(mdl, o_drv + 4 * k, drc[k]);
        // ... and the candidates' topology words for phase 5 (their geometry records hang on them: two dependent round trips)
        for (int s = 0; s < 2; ++s) cand_w[s] = lane + 64 * s < d.n_cand ? topo[EMLOCO_TOPO_CAND + lane + 64 * s] : 0;
        const int pd4 = sh_pd[lane < NB ? lane : 0];
        for (int lev = 1; lev <= d.max_depth; ++lev) {
            if ((lane < NB) && PD_DEPTH(pd4) == lev) {
                float ap[6], t[3], a[6], Wm[18], Km[6];
                float R[9], r[3], Sl[3][3];
                for (int k = 0; k < 9; ++k) R[k] = sh_R[lane][k];
                for (int k = 0; k < 3; ++k) r[k] = sh_R[lane][9 + k];
                for (int c = 0; c < 3; ++c) { const float ax[3] = {R[c], R[3 + c], R[6 + c]}; cross3(r, ax, Sl[c]); }
                for (int k = 0; k < 18; ++k) Wm[k] = sh_W[lane][k];
                for (int k = 0; k < 6; ++k) Km[k] = sh_W[lane][18 + k];
                for (int k = 0; k < 6; ++k) ap[k] = sh_a[PD_PARENT(pd4)][k];
                for (int c = 0; c < 3; ++c) {
                    float acc = 0.0f;
                    for (int k = 0; k < 6; ++k) acc = fmaf(Wm[k * 3 + c], ap[k], acc);
                    t[c] = uh[c] - acc;
                }
                qdd[0] = SOP3(Km[0], t[0], Km[1], t[1], Km[3], t[2]);
                qdd[1] = SOP2(Km[2], t[1], Km[4], t[2]);
                qdd[2] = Km[5] * t[2];
                for (int k = 0; k < 3; ++k) {
                    a[k] = ADD_SOP3(ap[k], R[k * 3], qdd[0], R[k * 3 + 1], qdd[1], R[k * 3 + 2], qdd[2]);
                    a[3 + k] = ADD_SOP3(ap[3 + k], Sl[0][k], qdd[0], Sl[1][k], qdd[1], Sl[2][k], qdd[2]);
                }
                for (int k = 0; k < 6; ++k) sh_a[lane][k] = a[k];
            }
            __syncthreads();
        }
        if (pass == 0) {
            bool over = false;
            if ((lane < NB) && lane >= 1)
                for (int k = 0; k < 3; ++k) {
                    const float *dr = drc[k];
                    const float kp = dr[0], kd = dr[1], eff = dr[3];
                    const float ti = tau[k] - (h * kd + h * h * kp) * qdd[k];
                    if (sat[k] == 0 && fabsf(ti) > eff) { sat[k] = ti > 0.0f ? 1 : -1; tau[k] = ti > 0.0f ? eff : -eff; dd[k] = dr[2]; over = true; }
                }
            if (__ballot(over) == 0ull) break;
        }
        }   // pass
        if ((lane < NB)) {
            for (int k = 0; k < 6; ++k) sh_Vf[lane][k] = fmaf(h, sh_a[lane][k], sh_V[lane][k]);
            if (lane == 0) for (int k = 0; k < 6; ++k) { sh_V0[k] = fmaf(h, sh_a[0][k], sh_root[7 + k]); sh_V0[6 + k] = 0.0f; }
        }

        PSTAMP(4);
        // ============================================================ 5. ground-contact candidates (lane = candidate)
        // two candidates per lane (`lane`, `lane + 64`); their body-frame points are re-derived from the model each
        // substep (L2 hits) rather than held in registers across the launch
        // What a candidate leaves for the contact list -- its contact point and, on a height field, the ground normal there -- waits
        // in LDS (arrays that are dead in this phase: Ia tail | pa | a | V) instead of 12 registers per lane across the ballots
        float *sh_stage = lds + O_G;                           // [128][7]
        static_assert(O_VF - O_G >= 128 * 7, "candidate staging does not fit the arrays that are dead in phase 5");
        int cb[2]; float cdist[2]; bool act[2];
        for (int s = 0; s < 2; ++s) {
            const int c = lane + 64 * s;
            cb[s] = -1; act[s] = false; cdist[s] = 0.0f;
            if (c < d.n_cand) {
                const int cp = cand_w[s], body = cp & 0xff, k = (cp >> 8) & 0xff, gt = cp >> 16;
                float ga[4], gb[4], clp[3];                      // geom a xyz, radius | geom b xyz
                ld4(mdl, EMLOCO_MB_GEO + body * 8, ga); ld4(mdl, EMLOCO_MB_GEO + body * 8 + 4, gb);
                const float crad = ga[3];
                cb[s] = body;
                if (gt == EMLOCO_GEOM_SPHERE) { clp[0] = ga[0]; clp[1] = ga[1]; clp[2] = ga[2]; }
                else if (gt == EMLOCO_GEOM_CAPSULE) {
                    const float *src = k == 0 ? ga : gb;
                    clp[0] = src[0]; clp[1] = src[1]; clp[2] = src[2];
                } else {
                    clp[0] = ga[0] + ((k & 1) ? gb[0] : -gb[0]);
                    clp[1] = ga[1] + ((k & 2) ? gb[1] : -gb[1]);
                    clp[2] = ga[2] + ((k & 4) ? gb[2] : -gb[2]);
                }
                float Rb[9], wp[3], cxw[3];
                for (int k2 = 0; k2 < 9; ++k2) Rb[k2] = sh_R[body][k2];
                matvec3(Rb, clp, wp);
                const float z = sh_pq[body][2] + wp[2];
                float *stg = sh_stage + c * 7;
                if (!hf_on) {
                    cdist[s] = (z - prm.ground_z) - crad;
                    cxw[0] = sh_R[body][9] + wp[0];
                    cxw[1] = sh_R[body][10] + wp[1];
                    cxw[2] = (sh_R[body][11] + wp[2]) - crad;
                } else {
                    // sphere of the candidate against the plane of the terrain triangle under its centre -- and, for a sphere with a
                    // radius, against the triangles under four probes one radius out along +-x / +-y: a neighbouring face (the ramp
                    // of a stair riser) is met when the sphere's SURFACE reaches it, not when its centre has crossed into the face's
                    // cell.  A probed triangle counts when the foot of the centre's perpendicular lies in it (its plane is not the
                    // terrain elsewhere) and its plane is nearer than what has been found; one contact per candidate, the nearest.
                    float zt, cnrm[3];
                    int tid0;
                    const float pcx = sh_pq[body][0] + wp[0], pcy = sh_pq[body][1] + wp[1];
                    mesh_plane(d, pcx, pcy, zt, cnrm, tid0);
                    float dperp = (z - zt) * cnrm[2];
                    if (crad > 0.0f)
                        for (int q = 0; q < 4; ++q) {
                            const float ex = q == 0 ? crad : (q == 1 ? 0.0f - crad : 0.0f), ey = q == 2 ? crad : (q == 3 ? 0.0f - crad : 0.0f);
                            float ztq, nq[3];
                            int tidq;
                            mesh_plane(d, pcx + ex, pcy + ey, ztq, nq, tidq);
                            const float dq = fmaf(z - ztq, nq[2], 0.0f - fmaf(ex, nq[0], ey * nq[1]));
                            int tidf;
                            if (d.hf_mv) { float zf, nf[3]; mesh_plane(d, pcx - dq * nq[0], pcy - dq * nq[1], zf, nf, tidf); }
                            else tidf = hf_triangle(d, pcx - dq * nq[0], pcy - dq * nq[1]);
                            if (tidq != tid0 && tidf == tidq && dq < dperp) { dperp = dq; cnrm[0] = nq[0]; cnrm[1] = nq[1]; cnrm[2] = nq[2]; }
                        }
                    if (d.hf_mv) {                                   // the corrected mesh's vertical faces
                        const float P[3] = {pcx, pcy, z};
                        mesh_walls(d, P, dperp, cnrm);
                    }
                    cdist[s] = dperp - crad;
                    for (int k2 = 0; k2 < 3; ++k2) { cxw[k2] = (sh_R[body][9 + k2] + wp[k2]) - crad * cnrm[k2]; stg[3 + k2] = cnrm[k2]; }
                }
                for (int k2 = 0; k2 < 3; ++k2) stg[k2] = cxw[k2];
                act[s] = cdist[s] < prm.contact_offset;
            }
        }
        unsigned long long m0 = __ballot(act[0]), m1 = __ballot(act[1]);
        int nc = __popcll(m0) + __popcll(m1);
#ifdef EMLOCO_SIM_NCHIST
        // diagnostic build (tools/exp/contact_hist.py): histogram over env-substeps of the candidates inside the contact offset
        // [0..63] and of the contacts kept [64 + 0..MAXC], in the buffer the phase stamps use (emloco_sim_profile)
        if (d.prof && lane == 0) {
            atomicAdd((unsigned long long *)&d.prof[nc < 63 ? nc : 63], 1ull);
            atomicAdd((unsigned long long *)&d.prof[64 + (nc < MAXC ? nc : MAXC)], 1ull);
        }
#endif
        while (nc > MAXC) {   // rare: drop the shallowest candidate (largest dist; ties -> highest candidate id)
            float best = -3.0e38f; int bid = -1;
            for (int s = 0; s < 2; ++s)
                if (act[s] && (cdist[s] > best || (cdist[s] == best && lane + 64 * s > bid))) { best = cdist[s]; bid = lane + 64 * s; }
            for (int off = 32; off >= 1; off >>= 1) {
                const float ob = __shfl_xor(best, off); const int oi = __shfl_xor(bid, off);
                if (ob > best || (ob == best && oi > bid)) { best = ob; bid = oi; }
            }
            if (bid == lane) act[0] = false;
            if (bid == lane + 64) act[1] = false;
            m0 = __ballot(act[0]); m1 = __ballot(act[1]);
            nc = __popcll(m0) + __popcll(m1);
        }
        // Warm start: the multipliers a candidate carried at the end of the previous substep (from the previous launch for
        // substep 0).  Every lane first fetches the old values of its own candidates -- old slot map and old multipliers are
        // still in place -- then, behind a barrier, the new contact list, its slot map and the warm values are written.
        float wl[2][3];
        for (int s = 0; s < 2; ++s) {
            wl[s][0] = wl[s][1] = wl[s][2] = 0.0f;
            const int c = lane + 64 * s;
            if (act[s]) {
                if (sub == 0) {
                    for (int k = 0; k < 3; ++k) wl[s][k] = lws_env[c * 3 + k];
                } else {
                    const int os = sh_slot[c];
                    if (os != 255) for (int k = 0; k < 3; ++k) wl[s][k] = sh_lam[3 * os + k];
                }
            }
        }
        __syncthreads();
        {
            const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
            const int i0 = __popcll(m0 & below), i1 = __popcll(m0) + __popcll(m1 & below);
            for (int s = 0; s < 2; ++s) {
                const int ci = s == 0 ? i0 : i1;
                sh_slot[lane + 64 * s] = act[s] ? (unsigned char)ci : (unsigned char)255;
                if (act[s]) {
                    const float *stg = sh_stage + (lane + 64 * s) * 7;      // this lane's own entry: no other lane touches it
                    sh_cbody[ci] = (unsigned char)cb[s]; sh_cdist[ci] = cdist[s];
                    for (int k = 0; k < 3; ++k) { sh_cx[ci][k] = stg[k]; sh_lam[3 * ci + k] = wl[s][k]; }
                    if (hf_on) {      // frame: normal, t1 = (y x n) / |y x n|, t2 = n x t1
                        const float n[3] = {stg[3], stg[4], stg[5]};
                        const float l2 = fmaf(n[2], n[2], n[0] * n[0]);
                        float *D = sh_cdir[ci];
                        D[0] = n[0]; D[1] = n[1]; D[2] = n[2];
                        if (l2 >= 0.1f) {
                            const float il = 1.0f / sqrtf(l2);
                            const float t1x = n[2] * il, t1z = 0.0f - n[0] * il;
                            D[3] = t1x; D[4] = 0.0f; D[5] = t1z;
                            D[6] = n[1] * t1z; D[7] = fmaf(n[2], t1x, -(n[0] * t1z)); D[8] = 0.0f - n[1] * t1x;
                        } else {      // a face looking along y (a riser across the y axis): t1 = (n x x) / |n x x|, t2 = n x t1
                            const float il = 1.0f / sqrtf(fmaf(n[2], n[2], n[1] * n[1]));
                            const float t1y = n[2] * il, t1z = 0.0f - n[1] * il;
                            D[3] = 0.0f; D[4] = t1y; D[5] = t1z;
                            D[6] = fmaf(n[1], t1z, -(n[2] * t1y)); D[7] = 0.0f - n[0] * t1z; D[8] = n[0] * t1y;
                        }
                    }
                }
            }
        }
        __syncthreads();
        const int nr = 3 * nc;
        work += nc > 0 ? 10 + nc : 0;

        PSTAMP(5);
        // ============================================================ 6a. rows: Jacobian, rhs, chain propagation (lane = row)
        float J[6] = {0, 0, 0, 0, 0, 0}, rhs = 0.0f, lam = 0.0f;
        float ys[YLEN];                                   // this row's chain-propagation vector (level-indexed: the compiler keeps it in
                                                          // scratch); entries beyond the row's own chain are never written NOR read
        // contacts come out of the compaction sorted by body (the candidate list is body-major): first / last contact of a body
        if ((lane < NB)) { sh_crange[lane] = 0; sh_crange[NB + lane] = -1; }
        __syncthreads();
        if (lane < nc) {
            const int cb_ = sh_cbody[lane];
            if (lane == 0 || sh_cbody[lane - 1] != cb_) sh_crange[cb_] = (signed char)lane;
            if (lane == nc - 1 || sh_cbody[lane + 1] != cb_) sh_crange[NB + cb_] = (signed char)lane;
        }
        const int myc = lane / 3, myd = lane - 3 * myc;
        int rbody = 0, rdep = 0;
        unsigned code = 0u;
        float p[6] = {0, 0, 0, 0, 0, 0};
        if (lane < nr) {
            rbody = sh_cbody[myc];
            float dir[3] = {myd == 1 ? 1.0f : 0.0f, myd == 2 ? 1.0f : 0.0f, myd == 0 ? 1.0f : 0.0f};
            if (hf_on) for (int k = 0; k < 3; ++k) dir[k] = sh_cdir[myc][3 * myd + k];
            float x[3] = {sh_cx[myc][0], sh_cx[myc][1], sh_cx[myc][2]};
            cross3(x, dir, J);
            J[3] = dir[0]; J[4] = dir[1]; J[5] = dir[2];
            float Vb[6];
            for (int k = 0; k < 6; ++k) Vb[k] = sh_Vf[rbody][k];
            const float vel = dot6(J, Vb);
            float bias = 0.0f;
            if (myd == 0) {
                const float dist = sh_cdist[myc];
                if (dist > 0.0f) bias = dist / h;
                else { bias = prm.erp * dist / h; if (bias < -prm.max_depen_vel) bias = -prm.max_depen_vel; }
            }
            rhs = vel + bias;
            for (int k = 0; k < 6; ++k) p[k] = -J[k];
            rdep = PD_DEPTH(sh_pd[rbody]);
        }
        // chain propagation, one tree level per (statically unrolled) step from the deepest level up: a row takes part from the
        // level of its own body on; `ci` is its chain body at the current level.  The level index is static, so ys[] stays in
        // registers; levels below every contact body are skipped wave-uniformly.
        int rdmax = rdep;
        for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(rdmax, off); rdmax = o > rdmax ? o : rdmax; }
        const int dmax = __builtin_amdgcn_readfirstlane(rdmax);              // deepest chain among the contact bodies
        {
            int ci = rbody;
#pragma unroll
            for (int lev = 7; lev >= 0; --lev) {
                if (lev < dmax) {
                    if (lane < nr && lev < rdep) {
                        const int i = ci;
                        float Ri[9], ri[3], u[3], uhh[3];
                        for (int k = 0; k < 9; ++k) Ri[k] = sh_R[i][k];
                        for (int k = 0; k < 3; ++k) ri[k] = sh_R[i][9 + k];
                        for (int a = 0; a < 3; ++a) {
                            float ax[3] = {Ri[a], Ri[3 + a], Ri[6 + a]}, sl[3];
                            cross3(ri, ax, sl);
                            const float Sa[6] = {ax[0], ax[1], ax[2], sl[0], sl[1], sl[2]};
                            u[a] = -dot6(Sa, p);
                        }
                        const float *W = sh_W[i], *K = W + 18;
                        uhh[0] = K[0] * u[0]; uhh[1] = SOP2(K[1], u[0], K[2], u[1]); uhh[2] = SOP3(K[3], u[0], K[4], u[1], K[5], u[2]);
                        const int pdi = sh_pd[i];
                        code |= (unsigned)(PD_SLOT(pdi) + 1) << (3 * lev);
                        ys[6 + 3 * lev] = uhh[0]; ys[6 + 3 * lev + 1] = uhh[1]; ys[6 + 3 * lev + 2] = uhh[2];
                        for (int k = 0; k < 6; ++k) p[k] = ADD_SOP3(p[k], W[k * 3], uhh[0], W[k * 3 + 1], uhh[1], W[k * 3 + 2], uhh[2]);
                        ci = PD_PARENT(pdi);
                    }
                }
            }
        }
        if (lane < nr) {
            for (int a = 0; a < 6; ++a) {   // L0 y = p
                float acc = p[a];
                for (int k = 0; k < a; ++k) acc = fmaf(-sh_L0[a * 6 + k], ys[k], acc);
                ys[a] = acc * sh_L0i[a];
            }
            lam = prm.warm * sh_lam[lane];
        }
        __syncthreads();

        PSTAMP(6);
        // ============================================================ 6b. contact matrix A = Y Y^T on the matrix cores
        // A[r][s] = <y_r, y_s> over the common-ancestor prefix (6 root entries + 3 per shared tree level): the sum, in ascending
        // level order, of the level blocks of the chain bodies that BOTH rows have on their chains.  One v_mfma_f32_32x32x2_f32
        // chain per 32 x 32 tile -- bit-equal to the fmaf chain in ascending k (measured: tools/exp/mfma_exact.hip): the root
        // block for all pairs, then per tree level one masked block per chain body present at that level, with the operands of
        // the rows that do not pass through that body set to zero.  A pair gets its non-zero terms exactly from the bodies it
        // shares (every other term adds an exact zero), so the accumulator IS the prefix sum: no snapshots, no per-pair depth
        // look-ups, 16 accumulator registers.  Operands: lanes 0-31 feed k = 2s, lanes 32-63 k = 2s+1; v_permlane32_swap hands
        // both over in one instruction.  The 3-wide level blocks are padded with one 0*0 step.  Tiles: (0,0) [, (1,0), (1,1)].
        // Round 6: the tiles advance in ONE pass over the steps -- three independent accumulator chains behind one operand swap and one
        // ballot / readlane group walk (before: one pass per tile, each paying the swaps, ballots and the matrix instruction's dependent
        // latency on its own; phase 6b 500 -> 330 ticks of 10 ns for a 48-row env).
        {
            typedef float sim_f32x16 __attribute__((vector_size(64)));
            const int h = lane >> 5, j31 = lane & 31;
            const int own_dep = (lane < nr) ? rdep : -1;   // -1: no row in this lane (all operands zero)
            const bool has_row = own_dep >= 0;
            const bool big = nr > 32;                      // wave-uniform: rows beyond the first tile
            sim_f32x16 acc00, acc10, acc11;
            for (int r = 0; r < 16; ++r) { acc00[r] = 0.0f; acc10[r] = 0.0f; acc11[r] = 0.0f; }
#define GRAM_STEP(V0, V1)                                                                                              \
            {                                                                                                      \
                const auto sw_ = __builtin_amdgcn_permlane32_swap(__float_as_uint(V0), __float_as_uint(V1), false, false); \
                const float op0_ = __uint_as_float(sw_[0]), op1_ = __uint_as_float(sw_[1]);                        \
                acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(op0_, op0_, acc00, 0, 0, 0);                          \
                if (big) {                                                                                         \
                    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(op1_, op0_, acc10, 0, 0, 0);                      \
                    acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(op1_, op1_, acc11, 0, 0, 0);                      \
                }                                                                                                  \
            }
            GRAM_STEP(has_row ? ys[0] : 0.0f, has_row ? ys[1] : 0.0f) GRAM_STEP(has_row ? ys[2] : 0.0f, has_row ? ys[3] : 0.0f)
            GRAM_STEP(has_row ? ys[4] : 0.0f, has_row ? ys[5] : 0.0f)
#pragma unroll
            for (int lev = 0; lev < 8; ++lev) {
                if (lev < dmax) {                               // wave-uniform
                    // this row's chain body at the level, as its index within the level + 1 (0: the chain ends above it)
                    const int gid = (lev < own_dep) ? (int)((code >> (3 * lev)) & 7u) : 0;
                    unsigned long long rem = __ballot(gid != 0);
                    while (rem != 0ull) {
                        const int first = __builtin_ctzll(rem);
                        const int g = __builtin_amdgcn_readlane(gid, first);
                        const bool in_g = gid == g;
                        GRAM_STEP(in_g ? ys[6 + 3 * lev] : 0.0f, in_g ? ys[7 + 3 * lev] : 0.0f) GRAM_STEP(in_g ? ys[8 + 3 * lev] : 0.0f, 0.0f)
                        rem &= ~__ballot(in_g);
                    }
                }
            }
#undef GRAM_STEP
            if (nc <= SQ_MAXC) {
                // Square layout.  Tile (0,0) holds every (row, column) of the first 32 rows; its upper half is bit-equal to the mirror
                // image (the products commute, the k order is the same), so the tile goes out whole: one address per lane plus
                // compile-time row offsets, rows and columns beyond nr included (zeros, inside the matrix region).  Tile (1,0) goes
                // to (32 + row, column) and, mirrored, to (column, 32 + row).
                if (nc > 0) {
                    float *t00 = sh_A + 4 * h * SQ_LD + j31;
                    for (int r = 0; r < 16; ++r) t00[((r & 3) + 8 * (r >> 2)) * SQ_LD] = acc00[r];
                    if (big) {
                        float *t10 = sh_A + (32 + 4 * h) * SQ_LD + j31, *t01 = sh_A + j31 * SQ_LD + 32 + 4 * h;
                        for (int r = 0; r < 16; ++r) {
                            const int ro = (r & 3) + 8 * (r >> 2);
                            if (32 + 4 * h + ro < nr) {
                                t10[ro * SQ_LD] = acc10[r];
                                t01[ro] = acc10[r];
                                if (32 + j31 < nr) t10[ro * SQ_LD + 32] = acc11[r];
                            }
                        }
                    }
                }
            } else
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row < nr && j31 <= row) sh_A[row * (row + 1) / 2 + j31] = acc00[r];
                if (big) {
                    const int row1 = 32 + row;
                    if (row1 < nr) sh_A[row1 * (row1 + 1) / 2 + j31] = acc10[r];
                    if (row1 < nr && 32 + j31 <= row1) sh_A[row1 * (row1 + 1) / 2 + 32 + j31] = acc11[r];
                }
            }
        }
        __syncthreads();

        PSTAMP(7);
        // ============================================================ 6c. projected Gauss-Seidel (lane s holds lambda_s)
        // Lane s owns row s: its multiplier `lam`, the running residual w_s = rhs_s + sum_r A_sr lam_r and 1/(A_ss (1+cfm)).
        // A row update happens in lane rr alone; its change is broadcast with one v_readlane and every lane folds it into
        // w with one fma through column rr of the symmetric matrix -- no wave reduction in the loop.
        // The matrix stays in LDS: lane s reads entry (s, rr) of its row for the row being updated, one contact ahead of the
        // sweep.  (Holding each lane's row in 60 registers cost a wave per SIMD in occupancy.)
        // Two instantiations of the same text, chosen wave-uniformly on the contact count (the layout 6b wrote):
        //   square (nc <= SQ_MAXC)  the lane's row is contiguous: one running address, 12 bytes on per contact, the three entries
        //                           of a contact at immediate offsets; the read ahead of the last contact runs three words past
        //                           the row (inside the matrix region, never used), so the loop carries no guard -- with fewer
        //                           than 11 contacts those words may be ones 6b did not write in this substep (stale LDS,
        //                           uninitialised memory on the CPU emulator): they are loaded and dropped, never computed with;
        //   packed lower triangle   entry (ls, rr) through tri_index, per entry.
        // The sweeps read the three entries of the next contact while the current one is being resolved (the reads do not
        // depend on the multipliers).  Leader chain, broadcasts, cone projection and the order of the fmas into w are one text.
        float gl0 = 0.0f, gl1 = 0.0f, gl2 = 0.0f;
        bool leader = false;
        auto pgs = [&](auto layout) {
            constexpr bool SQ = decltype(layout)::square;
            const int ls = lane < nr ? lane : 0;                      // idle lanes shadow lane 0 (their w is never used)
            const int arow = SQ ? ls * SQ_LD : 0;                     // square layout: word offset of this lane's row
            const float ainv = (lane < nr) ? 1.0f / (sh_A[SQ ? arow + ls : ls * (ls + 1) / 2 + ls] * (1.0f + prm.cfm)) : 0.0f;
            // (tri_index is branch-free min / max / multiply arithmetic per lane.  Two cheaper-looking forms -- a compare-and-select
            // between the two triangle forms, and the larger index's offset taken from the scalar unit with a per-lane select --
            // have fewer vector instructions and both measured slower: first sweep 340 -> 430 / 392 ticks)
            float w = rhs;
            {                                                          // warm start (matrix entries read one contact ahead)
                float n0 = 0.0f, n1a = 0.0f, n2a = 0.0f;
                int ao = arow;                                         // square layout: running offset, 3 words on per contact
                if (nc > 0) contact_entries3<SQ>(sh_A, ao, ls, 0, n0, n1a, n2a);
                for (int c = 0; c < nc; ++c) {
                    const int r0 = 3 * c;
                    const float a0 = n0, a1 = n1a, a2 = n2a;
                    if (SQ || c + 1 < nc) {
                        if (SQ) ao += 3;
                        contact_entries3<SQ>(sh_A, ao, ls, r0 + 3, n0, n1a, n2a);
                    }
                    const float l0 = lane_bcast(lam, r0), l1 = lane_bcast(lam, r0 + 1), l2 = lane_bcast(lam, r0 + 2);
                    const float u0 = fmaf(a0, l0, w);
                    w = (l0 != 0.0f) ? u0 : w;
                    const float u1 = fmaf(a1, l1, w);
                    w = (l1 != 0.0f) ? u1 : w;
                    const float u2 = fmaf(a2, l2, w);
                    w = (l2 != 0.0f) ? u2 : w;
                }
            }
            PSTAMP(11);
            // The sweeps resolve a contact inside ONE lane, the lane of its normal row (the leader): it holds the three
            // multipliers of the contact, the reciprocal diagonals and the sub-diagonal of its 3 x 3 block, fetches the residuals
            // of its two tangent rows (two v_readlane of values that are ready since the previous contact) and walks normal ->
            // tangent 1 -> tangent 2 -> friction cone on its own, forming the intermediate residuals exactly as the rows'
            // own lanes will; the three changes (and the two of a cone projection) are then broadcast and every lane folds them
            // into its w in the same order.  Same operations per value as the row-by-row sweep (the oracle's) with a third of the
            // cross-lane round trips; branch-free on purpose (an exec-masked leader block was slower than the row-by-row sweep).
            // A wave issues in order at ~4 cycles per instruction here, so the sweep costs what its instruction count costs:
            // first sweep of a 3-foot-contact env 380 -> 356 ticks of 10 ns.
            const int lr0 = ls - (lane < nr ? myd : 0);               // first row of this lane's contact
            gl0 = __shfl(lam, lr0); gl1 = __shfl(lam, lr0 + 1); gl2 = __shfl(lam, lr0 + 2);
            const float gi1 = __shfl(ainv, lr0 + 1), gi2 = __shfl(ainv, lr0 + 2);
            const int ablk = lr0 * SQ_LD + lr0;                      // square layout: the contact's 3 x 3 diagonal block
            const float gA10 = sh_A[SQ ? ablk + SQ_LD : tri_index(lr0 + 1, lr0)], gA20 = sh_A[SQ ? ablk + 2 * SQ_LD : tri_index(lr0 + 2, lr0)];
            const float gA21 = sh_A[SQ ? ablk + 2 * SQ_LD + 1 : tri_index(lr0 + 2, lr0 + 1)];
            leader = lane < nr && myd == 0;
            for (int it = 0; it < prm.n_iter; ++it) {
                float n0 = 0.0f, n1a = 0.0f, n2a = 0.0f;
                int ao = arow;                                         // square layout: running offset, 3 words on per contact
                if (nc > 0) contact_entries3<SQ>(sh_A, ao, ls, 0, n0, n1a, n2a);
                for (int c = 0; c < nc; ++c) {
                    const int r0 = 3 * c;
                    const float a0 = n0, a1 = n1a, a2 = n2a;
                    if (SQ || c + 1 < nc) {
                        if (SQ) ao += 3;
                        contact_entries3<SQ>(sh_A, ao, ls, r0 + 3, n0, n1a, n2a);
                    }
                    const float w1s = lane_bcast(w, r0 + 1), w2s = lane_bcast(w, r0 + 2);
                    // branch-free: every lane runs the leader's chain on its own contact's values, only lane r0's results are read
                    float nl0 = fmaf(-w, ainv, gl0);
                    if (nl0 < 0.0f) nl0 = 0.0f;
                    const float d0 = nl0 - gl0;
                    const float w1 = fmaf(gA10, d0, w1s);
                    const float nl1 = fmaf(-w1, gi1, gl1);
                    const float d1 = nl1 - gl1;
                    const float w2 = fmaf(gA21, d1, fmaf(gA20, d0, w2s));
                    const float nl2 = fmaf(-w2, gi2, gl2);
                    const float d2 = nl2 - gl2;
                    const bool me = lane == r0;
                    gl0 = me ? nl0 : gl0; gl1 = me ? nl1 : gl1; gl2 = me ? nl2 : gl2;
                    const float lim = prm.mu * nl0;
                    const float m2 = fmaf(nl1, nl1, nl2 * nl2);
                    w = fmaf(a0, lane_bcast(d0, r0), w);
                    w = fmaf(a1, lane_bcast(d1, r0), w);
                    w = fmaf(a2, lane_bcast(d2, r0), w);
                    if (__builtin_expect(__ballot(me && m2 > lim * lim) != 0ull, 0)) {   // wave-uniform: outside the friction cone
                        const float sc = lim / sqrtf(m2);
                        const float n1 = nl1 * sc, n2 = nl2 * sc;
                        gl1 = me ? n1 : gl1; gl2 = me ? n2 : gl2;
                        w = fmaf(a1, lane_bcast(n1 - nl1, r0), w);
                        w = fmaf(a2, lane_bcast(n2 - nl2, r0), w);
                    }
                }
                if (it == 0) PSTAMP(12);
            }
        };
        if (nc <= SQ_MAXC) pgs(ContactMatrixSquare{}); else pgs(ContactMatrixPacked{});
        if (leader) { sh_lam[lane] = gl0; sh_lam[lane + 1] = gl1; sh_lam[lane + 2] = gl2; }
        else if (lane >= nr && lane < MAXR) sh_lam[lane] = 0.0f;
        __syncthreads();
        lam = (lane < nr) ? sh_lam[lane] : 0.0f;

        PSTAMP(8);
        // ============================================================ 7. impulses -> velocity change (second solve)
        float dq[3] = {0, 0, 0};
        if ((lane < NB) && last && nc == 0)
            for (int k = 0; k < 3; ++k) cf_env[lane * 3 + k] = 0.0f;
        if (nc > 0) {
            // every row's lane stages its Jacobian row (and, in the last substep, its share of the reported contact force)
            // in the matrix's LDS, which is dead by now; a body then adds up its rows in contact order with one fma chain
            float (*sh_row)[12] = (float (*)[12])sh_A;
            if (lane < nr) {
                float dir[3] = {myd == 1 ? 1.0f : 0.0f, myd == 2 ? 1.0f : 0.0f, myd == 0 ? 1.0f : 0.0f};
                if (hf_on) for (int k = 0; k < 3; ++k) dir[k] = sh_cdir[myc][3 * myd + k];
                const float x[3] = {sh_cx[myc][0], sh_cx[myc][1], sh_cx[myc][2]};
                float Jr[3];
                cross3(x, dir, Jr);
                for (int k = 0; k < 3; ++k) { sh_row[lane][k] = Jr[k]; sh_row[lane][3 + k] = dir[k]; }
                if (last) for (int k = 0; k < 3; ++k) sh_row[lane][6 + k] = dir[k] * lam / h;
            }
            __syncthreads();
            float pin[6] = {0, 0, 0, 0, 0, 0};
            if ((lane < NB)) {
                float cf[3] = {0, 0, 0};
                const int r_end = 3 * sh_crange[NB + lane] + 3;
                for (int r = 3 * sh_crange[lane]; r < r_end; ++r) {
                    const float l = sh_lam[r];
                    for (int k = 0; k < 6; ++k) pin[k] = fmaf(-sh_row[r][k], l, pin[k]);
                    if (last) for (int k = 0; k < 3; ++k) cf[k] += sh_row[r][6 + k];
                }
                if (last) for (int k = 0; k < 3; ++k) cf_env[lane * 3 + k] = cf[k];
            }
            __syncthreads();                                       // the staged rows lie over pa / a, which are written from here on
            // bodies deeper than every contact body carry no impulse and have no loaded descendant: their share of the up pass
            // is exactly zero (uh = +0, pa = +0), so the pass starts at the deepest contact level
            const int pd7 = sh_pd[lane < NB ? lane : 0];
            if ((lane < NB) && PD_DEPTH(pd7) > dmax) { uh[0] = uh[1] = uh[2] = 0.0f; for (int k = 0; k < 6; ++k) sh_pa[lane][k] = 0.0f; }
            __syncthreads();
            for (int lev = (d.max_depth < dmax ? d.max_depth : dmax); lev >= 0; --lev) {
                if ((lane < NB) && PD_DEPTH(pd7) == lev) {
                    for (int k = 0; k < 6; ++k) pA[k] = pin[k];
                    for (int ci = 0; ci < 3; ++ci) {
                        const int ch = PD_CHILD(pd7, ci);
                        if (ch != 31) for (int k = 0; k < 6; ++k) pA[k] += sh_pa[ch][k];
                    }
                    if (lev > 0) {
                        float u[3], Wm[18], Km[6];
                        float R[9], r[3], Sl[3][3];
                        for (int k = 0; k < 9; ++k) R[k] = sh_R[lane][k];
                        for (int k = 0; k < 3; ++k) r[k] = sh_R[lane][9 + k];
                        for (int c = 0; c < 3; ++c) { const float ax[3] = {R[c], R[3 + c], R[6 + c]}; cross3(r, ax, Sl[c]); }
                        for (int k = 0; k < 18; ++k) Wm[k] = sh_W[lane][k];
                        for (int k = 0; k < 6; ++k) Km[k] = sh_W[lane][18 + k];
                        for (int c = 0; c < 3; ++c) {
                            const float Sc[6] = {R[c], R[3 + c], R[6 + c], Sl[c][0], Sl[c][1], Sl[c][2]};
                            u[c] = 0.0f - fdot6(Sc, pA);
                        }
                        uh[0] = Km[0] * u[0];
                        uh[1] = SOP2(Km[1], u[0], Km[2], u[1]);
                        uh[2] = SOP3(Km[3], u[0], Km[4], u[1], Km[5], u[2]);
                        for (int k = 0; k < 6; ++k)
                            sh_pa[lane][k] = ADD_SOP3(pA[k], Wm[k * 3], uh[0], Wm[k * 3 + 1], uh[1], Wm[k * 3 + 2], uh[2]);
                    } else {
                        float y[6], x[6];
                        for (int a = 0; a < 6; ++a) {
                            float acc = -pA[a];
                            for (int k = 0; k < a; ++k) acc = fmaf(-sh_L0[a * 6 + k], y[k], acc);
                            y[a] = acc * sh_L0i[a];
                        }
                        for (int a = 5; a >= 0; --a) {
                            float acc = y[a];
                            for (int k = a + 1; k < 6; ++k) acc = fmaf(-sh_L0[k * 6 + a], x[k], acc);
                            x[a] = acc * sh_L0i[a];
                        }
                        for (int k = 0; k < 6; ++k) { sh_a[0][k] = x[k]; sh_V0[6 + k] = x[k]; }
                    }
                }
                __syncthreads();
            }
            for (int lev = 1; lev <= d.max_depth; ++lev) {
                if ((lane < NB) && PD_DEPTH(pd7) == lev) {
                    float ap[6], t[3], a[6], Wm[18], Km[6];
                    float R[9], r[3], Sl[3][3];
                    for (int k = 0; k < 9; ++k) R[k] = sh_R[lane][k];
                    for (int k = 0; k < 3; ++k) r[k] = sh_R[lane][9 + k];
                    for (int c = 0; c < 3; ++c) { const float ax[3] = {R[c], R[3 + c], R[6 + c]}; cross3(r, ax, Sl[c]); }
                    for (int k = 0; k < 18; ++k) Wm[k] = sh_W[lane][k];
                    for (int k = 0; k < 6; ++k) Km[k] = sh_W[lane][18 + k];
                    for (int k = 0; k < 6; ++k) ap[k] = sh_a[PD_PARENT(pd7)][k];
                    for (int c = 0; c < 3; ++c) {
                        float acc = 0.0f;
                        for (int k = 0; k < 6; ++k) acc = fmaf(Wm[k * 3 + c], ap[k], acc);
                        t[c] = uh[c] - acc;
                    }
                    dq[0] = SOP3(Km[0], t[0], Km[1], t[1], Km[3], t[2]);
                    dq[1] = SOP2(Km[2], t[1], Km[4], t[2]);
                    dq[2] = Km[5] * t[2];
                    for (int k = 0; k < 3; ++k) {
                        a[k] = ADD_SOP3(ap[k], R[k * 3], dq[0], R[k * 3 + 1], dq[1], R[k * 3 + 2], dq[2]);
                        a[3 + k] = ADD_SOP3(ap[3 + k], Sl[0][k], dq[0], Sl[1][k], dq[1], Sl[2][k], dq[2]);
                    }
                    for (int k = 0; k < 6; ++k) sh_a[lane][k] = a[k];
                }
                __syncthreads();
            }
        }

        {   // momentum the system must have after this substep: gravity and the contact impulses are the only external ones
            float imp[3] = {0.0f, 0.0f, 0.0f};
            if (nc > 0) {
                float dir[3] = {myd == 1 ? 1.0f : 0.0f, myd == 2 ? 1.0f : 0.0f, myd == 0 ? 1.0f : 0.0f};
                if (hf_on && lane < nr) for (int k = 0; k < 3; ++k) dir[k] = sh_cdir[myc][3 * myd + k];
                for (int k = 0; k < 3; ++k) imp[k] = wave_sum(lane < nr ? dir[k] * lam : 0.0f);
            }
            if (lane == 0) {
                for (int k = 0; k < 3; ++k) sh_P[k] = sh_P[3 + k] + imp[k];
                sh_P[2] = fmaf(sh_P[6] * prm.gravity_z, h, sh_P[2]);
            }
        }
        const float damp = 1.0f / (1.0f + h * prm.ang_damping);
        {   // angular momentum about the centre of mass after this substep: the moments of the contact impulses, then the damping
            float tq[3] = {0.0f, 0.0f, 0.0f};
            if (nc > 0) {
                float dir[3] = {myd == 1 ? 1.0f : 0.0f, myd == 2 ? 1.0f : 0.0f, myd == 0 ? 1.0f : 0.0f};
                if (hf_on && lane < nr) for (int k = 0; k < 3; ++k) dir[k] = sh_cdir[myc][3 * myd + k];
                float t[3] = {0.0f, 0.0f, 0.0f};
                if (lane < nr) {
                    float arm[3], ip[3];
                    for (int k = 0; k < 3; ++k) { arm[k] = sh_cx[myc][k] - sh_L[8 + k]; ip[k] = dir[k] * lam; }
                    cross3(arm, ip, t);
                }
                for (int k = 0; k < 3; ++k) tq[k] = wave_sum(t[k]);
            }
            if (lane == 0) for (int k = 0; k < 3; ++k) sh_L[k] = (sh_L[4 + k] + tq[k]) * damp;
        }
        PSTAMP(9);
        // ============================================================ 8. integrate
        bool clamped = false;       // a rate clamped to max_ang_vel changes the angular momentum in a way the balance does not predict: it is skipped once
        if ((lane < NB) && lane >= 1) {
            float wn[3];
            for (int k = 0; k < 3; ++k) {
                wn[k] = fmaf(h, qdd[k], wj[k]) + dq[k];      // free joint rate of phase 4 + the impulses' share
                if (last) {
                    float dr[4];
                    ld4(mdl, o_drv + 4 * k, dr);
                    const float kpk = dr[0], kdk = dr[1], tgk = tgt_env[jdof + k];
                    // torque applied over this substep (the contact impulses moved the implicit drive along; reported within the limit)
                    const float effk = dr[3];
                    float tq = sat[k] == 0 ? kpk * (tgk - edof[k] - h * wn[k]) - kdk * wn[k]
                             : (sat[k] == 2 ? tgk : (sat[k] > 0 ? effk : -effk));         // (clipped to the limit just below)
                    tq = tq > effk ? effk : (tq < -effk ? -effk : tq);
                    d.dof_force[(size_t)env * NDOF + jdof + k] = tq;
                }
                wj[k] = wn[k] * damp;
            }
            const float nj = sqrtf(dot3(wj, wj));
            if (nj > prm.max_ang_vel) { const float sc = prm.max_ang_vel / nj; wj[0] *= sc; wj[1] *= sc; wj[2] *= sc; clamped = true; }
            float e[3] = {h * wj[0], h * wj[1], h * wj[2]}, dqt[4], qn[4];
            rotvec2quat(e, dqt);
            qmul(qj, dqt, qn); qnormalize(qn);
            for (int k = 0; k < 4; ++k) qj[k] = qn[k];
            quat2rotvec(qj, edof);
        }
        if (lane == 0) {
            float V0[6];
            for (int k = 0; k < 6; ++k) V0[k] = sh_V0[k] + sh_V0[6 + k];
            for (int k = 0; k < 3; ++k) V0[k] *= damp;
            const float n = sqrtf(dot3(V0, V0));
            if (n > prm.max_ang_vel) { const float sc = prm.max_ang_vel / n; V0[0] *= sc; V0[1] *= sc; V0[2] *= sc; clamped = true; }
            float e[3], dqt[4], qn[4], q0[4] = {sh_root[3], sh_root[4], sh_root[5], sh_root[6]};
            for (int k = 0; k < 3; ++k) { sh_root[k] += h * V0[3 + k]; e[k] = h * V0[k]; }
            rotvec2quat(e, dqt);
            qmul(dqt, q0, qn); qnormalize(qn);
            for (int k = 0; k < 4; ++k) sh_root[3 + k] = qn[k];
            // the reference point O of the spatial quantities moves with the root origin: re-base the root twist from O to
            // O + h v (velocity of the body-fixed point there: v + w x (h v)); without it the root's linear velocity would not
            // turn with the body and linear momentum would not be conserved
            float wxv[3];
            cross3(V0, V0 + 3, wxv);
            for (int k = 0; k < 3; ++k) V0[3 + k] = fmaf(h, wxv[k], V0[3 + k]);
            for (int k = 0; k < 6; ++k) sh_root[7 + k] = V0[k];
        }
        {
            const bool any_clamped = __ballot(clamped) != 0ull;
            if (lane == 0) sh_L[3] = any_clamped ? 0.0f : 1.0f;
        }
        __syncthreads();
        PSTAMP(10);
        // the next substep's (or the final pass's) joint offsets | mass.  Unconditional on purpose: behind a condition the compiler
        // would have to carry this substep's copy through the whole loop body; a part of one substep drops the request
        ld4(mdl, o_dyn, jm);
    }

    if (pw.publishes()) {             // hand over to the next part (see part_ld80): store the tagged granules and leave
        if (!pw.consumes() && env == d.part_poison) return;        // test hook: this env's first part publishes nothing
        const float tg = __uint_as_float(EMLOCO_PART_TAG(d.part_seq, part));
        float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if ((lane < NB)) { w[0] = qj[0]; w[1] = qj[1]; w[2] = qj[2]; w[3] = qj[3]; }
        else if (lane < NB + 32) {
            const int g = lane - NB;
            const float *src = g < 4 ? sh_root + 4 * g : g < 6 ? sh_P + 4 * (g - 4) : g < 22 ? sh_lam + 4 * (g - 6) : g < 30 ? (const float *)sh_slot + 4 * (g - 22) : sh_L;
            if (g != 30) { w[0] = src[0]; w[1] = src[1]; w[2] = src[2]; w[3] = src[3]; }
            else w[0] = __int_as_float(work);
        }
        float *pa = pst + lane * 4;
        part_st16(pa, w[0], tg, w[1], tg);
        part_st16(pa + PART_G1, w[2], tg, w[3], tg);
        if ((lane < NB)) {
            float *pb = pst + PART_GB + lane * 4;
            part_st16(pb, wj[0], tg, wj[1], tg);
            part_st16(pb + 4 * NB, wj[2], tg, edof[0], tg);
            part_st16(pb + 8 * NB, edof[1], tg, edof[2], tg);
        }
        return;
    }
    // ---------------------------------------------------------------- write back (state after the final kinematics pass)
    if ((lane < NB)) {
        float *o = d.rb_state + (size_t)env * NB * 13 + lane * 13;
        float t[3], V[6], r[3];
        for (int k = 0; k < 6; ++k) V[k] = sh_V[lane][k];
        for (int k = 0; k < 3; ++k) r[k] = sh_R[lane][9 + k];
        cross3(V, r, t);
        for (int k = 0; k < 3; ++k) { o[k] = sh_pq[lane][k]; o[7 + k] = V[3 + k] + t[k]; o[10 + k] = V[k]; }
        for (int k = 0; k < 4; ++k) o[3 + k] = sh_pq[lane][4 + k];
        if (lane >= 1) {
            float *ds = dofs_env + jdof * 2;
            for (int k = 0; k < 3; ++k) { ds[2 * k] = edof[k]; ds[2 * k + 1] = wj[k]; }
        }
    }
    if (lane == 0) {
        float *rs = d.root_state + (long)env * 13;
        for (int k = 0; k < 3; ++k) { rs[k] = sh_root[k]; rs[7 + k] = sh_root[10 + k]; rs[10 + k] = sh_root[7 + k]; }
        for (int k = 0; k < 4; ++k) rs[3 + k] = sh_root[3 + k];
    }
    for (int s = 0; s < 2; ++s) {      // warm-start multipliers per candidate for the next launch
        const int c = lane + 64 * s;
        if (c < MAXCAND) {
            const int os = sh_slot[c];
            for (int k = 0; k < 3; ++k) lws_env[c * 3 + k] = os != 255 ? sh_lam[3 * os + k] : 0.0f;
        }
    }
}
#undef o_dyn
#undef jdof
#undef o_drv

// The step of every env (one workgroup = one wave per env).  Subset launches (emloco_sim_step_subset): with skip flags the
// workgroups of the flagged envs leave at once; with a device-compacted id list (valid ids first, -1 after them) workgroup
// i steps list entry i.  Both are THIS kernel: a second instantiation of the 49 KB body for the list launch ran beside the
// big launch out of a different code object, the two thrashed the instruction cache the CUs share (measured: the big
// launch 0.58 -> 0.64 ms, the 25-env list launch 0.22 -> 0.44 ms).
// HF = 0: ground plane, HF = 1: height-field ground (d.hf).  Two instantiations, a simulator uses one of them for its lifetime: with the
// height-field branches compiled out the plane kernel is 0.9 % shorter (0.3507 -> 0.3477 ms at 4096 envs).
template <int HF>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, 64), amdgpu_waves_per_eu(EMLOCO_SIM_WAVES_PER_SIMD, EMLOCO_SIM_WAVES_PER_SIMD)))
sim_step_kernel(EmlocoSimParams prm, EmlocoSimDev d) {
    const int n_parts = d.n_parts > 1 ? d.n_parts : 1;
    // the uniform split (all first parts, then all second parts, ...) or this workgroup's word of the part plan (sim_plan.h)
    const SimPlanWork pw = sim_plan_decode(d.plan, d.plan_n, blockIdx.x, d.n_env, n_parts, prm.n_sub);
    const int part = pw.part(), slot = pw.slot;
    if (!pw.valid) return;
    int env = d.step_order ? d.step_order[slot] : slot;
    if (d.step_ids) { env = d.step_ids[slot]; if (env < 0) return; }   // list launch: workgroup i steps list entry i (-1: padding)
    if (d.step_skip && d.step_skip[env] != 0) return;            // flagged envs are stepped elsewhere
    env = __builtin_amdgcn_readfirstlane(env);                   // workgroup-uniform: the env's bases live in scalar registers
    const long long t0 = d.step_start ? (long long)wall_clock64() : 0ll;
    int work;
    sim_step_env<HF>(prm, d, env, work, pw);
    if (d.step_ticks && threadIdx.x == 0 && pw.final()) {
        // the key of the next launch's order: EMLOCO_COST_KEY_TICKS (diagnostic build) = measured duration in 5.12 us units
#ifdef EMLOCO_COST_KEY_TICKS
        d.step_ticks[env] = (unsigned)(((long long)wall_clock64() - t0) >> 9);
#else
        d.step_ticks[env] = (unsigned)work;
#endif
#ifndef EMLOCO_SIM_SCHED
        if (d.step_start) { d.step_start[env] = (unsigned long long)t0; d.step_start[d.n_env + env] = (unsigned long long)wall_clock64(); }
#endif
    }
#ifdef EMLOCO_SIM_SCHED
    if (d.step_start && threadIdx.x == 0) {
        unsigned long long *ss = d.step_start + ((size_t)part * d.n_env + env) * 4;
        ss[0] = (unsigned long long)t0; ss[2] = (unsigned long long)wall_clock64(); ss[3] = (unsigned long long)(part | slot << 8) | (unsigned long long)blockIdx.x << 32;
    }
#endif
}

// Dispatch order of the next full launch: env ids sorted by the contact work of their last step (sum over its substeps of
// 10 + number of contacts where there were any: the contact phases are ~45 % of a substep and grow with the contact count),
// most first (counting sort, one 1024-thread workgroup).  The measured duration of the last step is the worse key: it is
// dominated by what the env's wave shared its SIMD and CU with (correlation between consecutive steps 0.2).  Workgroups are
// handed to the CUs in index order.  The split launch (emloco_sim_set_split, 4 parts) is 16 384 one-wave workgroups for 4096
// envs -- all first parts in this order, then all second parts in the same order, and so on -- on 3072 wave slots (256 CUs x
// 12): the first 3072 first parts start at once, everything behind them takes a slot as one frees up.  A later part finds
// its predecessor's hand-over complete when it starts (it queued ~19 us for its slot, median; tools/exp/sim_sched.py,
// profiles/r09_sim_serial_path.txt): the launch is bound by the slots, 82 % of the slot-time is spent running and 15 % is the
// fill and drain at its two ends.  Its length is therefore set by what the LAST workgroups of each part cost: with the
// expensive envs (many contacts) first and the cheap ones (airborne) last, the slots that free up late receive short work.
// The order within a bucket is whatever the LDS atomics give -- envs are independent, results do not depend on it.
// Where that empty slot-time lies (profiles/r10_sim_launch_plan.txt): 0.1 % before the first slot turns over, 2 % in the
// middle, 15 % after the last workgroup has been dispatched -- 5.33 rounds of near-equal jobs leave the last round a third
// full, and its jobs were the longest of the launch (the last part carries the final pass and the write-back).  Under a part
// plan (emloco_sim_set_plan, sim_plan.h) the position in this order is a RANK and the plan's table says which workgroup
// runs which substeps of which rank: the default plan gives every env a fifth, short workgroup for the final pass and the
// write-back, and starts the cheaper half of this order one stage ahead of the other half, so that the stages of the two
// halves interleave instead of ending together.
__global__ void __launch_bounds__(1024)
sim_order_kernel(const unsigned *ticks, int n, int *order, unsigned char *bucket_ws) {
    order_sort(ticks, n, order, bucket_ws);             // order_device.h
}

// Forward kinematics only (used after state writes through the *_indexed setters): fills rb_state of
// the listed envs from root_state / dof_state.  One wave per env; lanes walk the tree level by level (fk_device.h).
__global__ void __launch_bounds__(64)
sim_fk_kernel(EmlocoSimDev d, const int *env_ids, int n_ids) {
    const int lane = threadIdx.x;
    // grid-stride over the id list (one pass when the grid covers it); a device-compacted list ends at its first -1
    for (int bi = blockIdx.x; bi < n_ids; bi += gridDim.x) {
        const int env = env_ids ? env_ids[bi] : bi;
        if (env < 0) break;
        __shared__ float sm[FK_SM_FLOATS];
        fk_env(d, env, lane, sm);
        __syncthreads();                              // LDS is reused by the next list entry
    }
}

// Rows of the listed envs from a caller's full tensor into the simulator's own (the *_indexed setters when `dev_full` is not the
// sim's alias): one workgroup per list entry.  Entries outside [0, n_env) are skipped -- the -1 padding of a device-compacted list
// (emloco_sim.h: valid ids first, -1 after them) and, since the check costs nothing, ids past the end -- so no entry can make a
// store land outside the destination.
__global__ void __launch_bounds__(64)
copy_rows_kernel(const float *src, float *dst, const int *ids, int n_ids, int row_len, int n_env) {
    const int i = blockIdx.x;
    if (i >= n_ids) return;
    const int env = ids[i];
    if (env < 0 || env >= n_env) return;
    const long base = (long)env * row_len;
    for (int k = threadIdx.x; k < row_len; k += blockDim.x) dst[base + k] = src[base + k];
}

}  // namespace emloco

#undef cross3
#undef dot3
#undef dot6
#undef qmul
#undef qnormalize
#undef q2mat
#undef matvec3
#undef rotvec2quat
#undef quat2rotvec
