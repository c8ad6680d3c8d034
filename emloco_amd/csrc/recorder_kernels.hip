// recorder_kernels.hip -- the flight recorder (include/emloco_task.h: emloco_recorder_record / emloco_recorder_check).  Included by
// recorder_capi.hip and, on the CPU, by tests/emu/emu_recorder.cpp.  The kernels copy 32-bit words and compare; the only arithmetic
// is the squared speed of the cause test, whose value is never stored (built without contraction, in the order the header states).
// No kernel hands anything to another workgroup of its launch: the claim is one workgroup, the launches around it own an env or a
// slot per workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/emloco_sim.h"
#include "../../include/emloco_task.h"

namespace emloco {

constexpr int kRecRoot = 13, kRecDof = EMLOCO_NDOF * 2, kRecWarm = EMLOCO_MAXCAND * 3, kRecDrive = EMLOCO_NDOF;
constexpr int kRecRb = EMLOCO_NB * 13, kRecCf = EMLOCO_NB * 3, kRecDf = EMLOCO_NDOF;
constexpr int kRecHeader = 4;
static_assert(kRecHeader + kRecRoot + kRecDof + kRecWarm + kRecDrive == EMLOCO_REC_WORDS, "record layout");
static_assert(kRecRoot + kRecDof + kRecWarm + kRecRb + kRecCf + kRecDf == EMLOCO_REC_POST_WORDS, "post-state layout");
static_assert(EMLOCO_REC_WORDS % 4 == 0 && EMLOCO_REC_POST_WORDS % 4 == 0, "16-byte rows");

constexpr int kRecThreads = EMLOCO_REC_WORDS / 4;        // record: one 16-byte store per thread and env
constexpr int kRecCauseWaves = 4;                        // cause bits: one wave per env
constexpr int kRecClaimThreads = 256;
constexpr int kRecCopyThreads = 256;
constexpr int kRecCauses = 5;

__device__ __forceinline__ uint32_t rec_bits(const float *p, long i) { return reinterpret_cast<const uint32_t *>(p)[i]; }

// word w of the record of (env, t)
__device__ __forceinline__ uint32_t rec_word(const EmlocoRecorderBufs &b, int env, int t, int w) {
    if (w < kRecHeader) return w == 0 ? (uint32_t)(int32_t)b.progress_buf[env] : w == 1 ? (uint32_t)t : w == 2 ? (uint32_t)b.drive_mode : 0u;
    w -= kRecHeader;
    if (w < kRecRoot) return rec_bits(b.root_state, (long)env * kRecRoot + w);
    w -= kRecRoot;
    if (w < kRecDof) return rec_bits(b.dof_state, (long)env * kRecDof + w);
    w -= kRecDof;
    if (w < kRecWarm) return rec_bits(b.warm_start, (long)env * kRecWarm + w);
    w -= kRecWarm;
    return rec_bits(b.drive, (long)env * kRecDrive + w);
}

// word w of the state after the step
__device__ __forceinline__ uint32_t rec_post_word(const EmlocoRecorderBufs &b, int env, int w) {
    if (w < kRecRoot) return rec_bits(b.root_state, (long)env * kRecRoot + w);
    w -= kRecRoot;
    if (w < kRecDof) return rec_bits(b.dof_state, (long)env * kRecDof + w);
    w -= kRecDof;
    if (w < kRecWarm) return rec_bits(b.warm_start, (long)env * kRecWarm + w);
    w -= kRecWarm;
    if (w < kRecRb) return rec_bits(b.rb_state, (long)env * kRecRb + w);
    w -= kRecRb;
    if (w < kRecCf) return rec_bits(b.contact_force, (long)env * kRecCf + w);
    w -= kRecCf;
    return rec_bits(b.dof_force, (long)env * kRecDf + w);
}

// record: grid-stride over the envs, thread i stores words 4 i .. 4 i + 3 of the env's record
__global__ void __launch_bounds__(kRecThreads)
recorder_record_kernel(EmlocoRecorderBufs b, int t) {
    const int row = t % b.depth;
    const int w = (int)threadIdx.x * 4;
    for (int env = (int)blockIdx.x; env < b.n_env; env += (int)gridDim.x) {
        uint4 v;
        v.x = rec_word(b, env, t, w); v.y = rec_word(b, env, t, w + 1); v.z = rec_word(b, env, t, w + 2); v.w = rec_word(b, env, t, w + 3);
        reinterpret_cast<uint4 *>(b.ring + ((long)env * b.depth + row) * EMLOCO_REC_WORDS)[threadIdx.x] = v;
    }
}

// stage 1: the cause bits of every env into cause_ws.  One wave per env, lanes 0..23 scan its bodies, lane 0 decides.
__global__ void __launch_bounds__(64 * kRecCauseWaves)
recorder_cause_kernel(EmlocoRecorderBufs b, int t) {
#ifndef EMLOCO_EMU
#pragma clang fp contract(off)
#endif
    const int lane = (int)threadIdx.x & 63;
    for (int env = (int)blockIdx.x * kRecCauseWaves + ((int)threadIdx.x >> 6); env < b.n_env; env += (int)gridDim.x * kRecCauseWaves) {   // wave-uniform
        bool bad = false, fast = false, spin = false;
        if (lane < EMLOCO_NB) {
            const float *s = b.rb_state + ((long)env * EMLOCO_NB + lane) * 13;
            float x[13];
            for (int k = 0; k < 13; ++k) x[k] = s[k];
            for (int k = 0; k < 13; ++k) bad |= !(fabsf(x[k]) <= 3.402823466e38f);      // NaN and +-Inf
            const float v2 = (x[7] * x[7] + x[8] * x[8]) + x[9] * x[9];
            const float w2 = (x[10] * x[10] + x[11] * x[11]) + x[12] * x[12];
            fast = v2 > b.speed2_limit;                                                 // (a NaN is not greater)
            spin = w2 > b.ang_speed2_limit;
        }
        const bool any_bad = __ballot(bad) != 0ull, any_fast = __ballot(fast) != 0ull, any_spin = __ballot(spin) != 0ull;
        if (lane == 0) {
            int c = (any_bad ? EMLOCO_REC_NONFINITE : 0) | (any_fast ? EMLOCO_REC_SPEED : 0) | (any_spin ? EMLOCO_REC_ANG_SPEED : 0);
            if (b.terminate_buf[env] != 0 && b.progress_buf[env] < (int64_t)b.early_fall_steps) c |= EMLOCO_REC_EARLY_FALL;
            if (b.request && b.request[env] != 0) c |= EMLOCO_REC_REQUEST;
            c &= b.cause_mask;
            if (c != 0 && (int64_t)t - (int64_t)b.last_capture_step[env] < (int64_t)b.depth) {      // its windows would overlap
                if (c & EMLOCO_REC_REQUEST) b.request[env] = 0;
                c = 0;
            }
            b.cause_ws[env] = c;
        }
    }
}

// stage 2: ONE workgroup hands the free slots to the step's triggered envs in ascending env index.  Thread i owns the contiguous
// envs [i c, (i + 1) c): it counts its triggered envs, an exclusive scan over the threads gives its first rank.  A claimed slot
// gets its four header words here; they tell the copy launch whose ring goes where.
__global__ void __launch_bounds__(kRecClaimThreads)
recorder_claim_kernel(EmlocoRecorderBufs b, int t) {
    __shared__ int scan[kRecClaimThreads];
    __shared__ int missed[kRecCauses];
    const int tid = (int)threadIdx.x;
    const int c = (b.n_env + kRecClaimThreads - 1) / kRecClaimThreads;
    const int lo = tid * c < b.n_env ? tid * c : b.n_env, hi = lo + c < b.n_env ? lo + c : b.n_env;
    int mine = 0;
    for (int e = lo; e < hi; ++e) mine += b.cause_ws[e] != 0;
    scan[tid] = mine;
    if (tid < kRecCauses) missed[tid] = 0;
    __syncthreads();
    for (int off = 1; off < kRecClaimThreads; off <<= 1) {       // inclusive scan
        const int add = tid >= off ? scan[tid - off] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    const int used = b.counters[0];
    const int total = scan[kRecClaimThreads - 1];
    int rank = scan[tid] - mine;
    const long slot_words = EMLOCO_REC_SLOT_WORDS((long)b.depth);
    const int64_t span = (int64_t)t - (int64_t)b.t0 + 1;
    const int n_valid = span < (int64_t)b.depth ? (int)span : b.depth;
    for (int e = lo; e < hi; ++e) {
        const int cause = b.cause_ws[e];
        if (cause == 0) continue;
        const int slot = used + rank++;
        if (slot < b.n_slots) {
            uint32_t *h = b.slots + slot * slot_words;
            h[0] = (uint32_t)e; h[1] = (uint32_t)t; h[2] = (uint32_t)cause; h[3] = (uint32_t)n_valid;
            b.last_capture_step[e] = t;
            if (cause & EMLOCO_REC_REQUEST) b.request[e] = 0;
        } else {
            for (int k = 0; k < kRecCauses; ++k)
                if (cause & (1 << k)) atomicAdd(&missed[k], 1);
        }
    }
    __syncthreads();
    if (tid == 0) b.counters[0] = used + total < b.n_slots ? used + total : b.n_slots;
    if (tid < kRecCauses && missed[tid] != 0) b.counters[1 + tid] += missed[tid];
}

// stage 3: grid-stride over the slots; a slot claimed at this step (in use, its header's t is this step's) takes its env's ring in
// chronological order and the state after the step
__global__ void __launch_bounds__(kRecCopyThreads)
recorder_copy_kernel(EmlocoRecorderBufs b, int t) {
    const long slot_words = EMLOCO_REC_SLOT_WORDS((long)b.depth);
    const int used = b.counters[0];
    for (int slot = (int)blockIdx.x; slot < used; slot += (int)gridDim.x) {       // block-uniform
        uint32_t *s = b.slots + slot * slot_words;
        if ((int)s[1] != t) continue;
        const int env = (int)s[0], n_valid = (int)s[3];
        const int first = t - n_valid + 1;
        uint4 *dst = reinterpret_cast<uint4 *>(s + kRecHeader);
        const uint4 *ring = reinterpret_cast<const uint4 *>(b.ring + (long)env * b.depth * EMLOCO_REC_WORDS);
        for (int i = (int)threadIdx.x; i < b.depth * kRecThreads; i += kRecCopyThreads) {
            const int j = i / kRecThreads, q = i % kRecThreads;
            uint4 v;
            v.x = v.y = v.z = v.w = 0u;
            if (j < n_valid) v = ring[(long)((first + j) % b.depth) * kRecThreads + q];
            dst[i] = v;
        }
        // the state after the step: as in the record its pieces lie back to back (none but the root starts on a 16-byte boundary of the
        // block, and a root row is 52 bytes), so words are gathered and the stores are wide
        uint4 *post = reinterpret_cast<uint4 *>(s + kRecHeader + (long)b.depth * EMLOCO_REC_WORDS);
        for (int q = (int)threadIdx.x; q < EMLOCO_REC_POST_WORDS / 4; q += kRecCopyThreads) {
            uint4 v;
            v.x = rec_post_word(b, env, 4 * q); v.y = rec_post_word(b, env, 4 * q + 1);
            v.z = rec_post_word(b, env, 4 * q + 2); v.w = rec_post_word(b, env, 4 * q + 3);
            post[q] = v;
        }
    }
}

}  // namespace emloco
