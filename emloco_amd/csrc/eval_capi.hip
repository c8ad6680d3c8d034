// eval_capi.hip -- C ABI of the LocoVal evaluation kernels (include/emloco_predictor.h: emloco_locoval_eval_*).
#include <hip/hip_runtime.h>
#include <cmath>
#include "eval_kernels.hip"
#include "capi_error.h"

using emloco::capi_fail;

static_assert(sizeof(EmlocoLocoValRecord) == 48, "EmlocoLocoValRecord is 48 bytes (the numpy dtype of learning/locoval_eval.py)");
static_assert(sizeof(EmlocoLocoValTrackRecord) == 32, "EmlocoLocoValTrackRecord is 32 bytes (TRACK_DTYPE of learning/locoval_eval.py)");

extern "C" {

int emloco_locoval_eval_step(const EmlocoLocoValEval *s, const float *reward_raw, const float *disc, const int64_t *dones,
                             const int64_t *terminate, const uint8_t *inverted, void *stream) {
    if (!s || s->n_env < 1 || s->games_per_env < 1 || !reward_raw || !dones || !s->coef || !s->c_disc || !s->tp_disc || !s->cr ||
        !s->c_loc || !s->c_pow || !s->tp_cr || !s->tp_loc || !s->tp_pow || !s->steps || !s->games || !s->done || !s->terminated ||
        !s->inverted || !s->waypoint_traj || !s->init_pose || !s->init_vel || !s->traj13 || !s->pose || !s->vel || !s->row_mask)
        return capi_fail(EMLOCO_E_ARG, "emloco_locoval_eval_step: bad argument");
    hipLaunchKernelGGL(emloco::locoval_eval_step_kernel, dim3((unsigned)((s->n_env + 3) / 4)), dim3(256), 0, (hipStream_t)stream, *s,
                       reward_raw, disc, dones, terminate, inverted);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_locoval_eval_finish(const EmlocoLocoValEval *s, const float *value, EmlocoLocoValRecord *records, void *stream) {
    if (!s || s->n_env < 1 || s->games_per_env < 1 || !value || !records || !s->n_full || !s->games || !s->done || !s->steps)
        return capi_fail(EMLOCO_E_ARG, "emloco_locoval_eval_finish: bad argument");
    hipLaunchKernelGGL(emloco::locoval_eval_finish_kernel, dim3((unsigned)((s->n_env + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *s,
                       value, records);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_locoval_eval_finish_multi(const EmlocoLocoValEval *s, const EmlocoLocoValNets *nets, EmlocoLocoValRecord *records, void *stream) {
    if (!s || s->n_env < 1 || s->games_per_env < 1 || !nets || !records || !s->n_full || !s->games || !s->done || !s->steps)
        return capi_fail(EMLOCO_E_ARG, "emloco_locoval_eval_finish_multi: bad argument");
    if (nets->n_nets < 1 || nets->n_nets > EMLOCO_EVAL_MAX_NETS)
        return capi_fail(EMLOCO_E_ARG, "emloco_locoval_eval_finish_multi: n_nets outside 1 .. EMLOCO_EVAL_MAX_NETS");
    for (int k = 0; k < nets->n_nets; ++k)
        if (nets->net[k].variant < 0 || nets->net[k].variant > 3 || !nets->net[k].value)
            return capi_fail(EMLOCO_E_ARG, "emloco_locoval_eval_finish_multi: a network with a bad variant or no value plane");
    hipLaunchKernelGGL(emloco::locoval_eval_finish_multi_kernel, dim3((unsigned)((s->n_env + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       *s, *nets, records);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_locoval_eval_reduce(int n_env, int games_per_env, const EmlocoLocoValRecord *records, const int32_t *games, double *moments,
                               void *stream) {
    if (n_env < 1 || games_per_env < 1 || !records || !games || !moments) return capi_fail(EMLOCO_E_ARG, "emloco_locoval_eval_reduce: bad argument");
    hipLaunchKernelGGL(emloco::locoval_eval_reduce_kernel, dim3(1), dim3(emloco::kEvalReduceThreads), 0, (hipStream_t)stream, n_env,
                       games_per_env, records, games, moments);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_locoval_eval_track(const EmlocoLocoValEval *s, const EmlocoLocoValTrack *t, EmlocoLocoValTrackRecord *records, float *samples,
                              void *stream) {
    if (!s || !t || !records || !samples || s->n_env < 1 || s->games_per_env < 1 || !s->steps || !s->games || !s->done)
        return capi_fail(EMLOCO_E_ARG, "emloco_locoval_eval_track: bad argument");
    if (t->stride < 1 || t->root_stride < 2 || !(t->dt > 0.0f) || !(t->traj_dur > 0.0f) || !std::isfinite(t->dt) || !std::isfinite(t->traj_dur))
        return capi_fail(EMLOCO_E_ARG, "emloco_locoval_eval_track: stride < 1, root_stride < 2, or dt / traj_dur not finite and positive");
    if (!t->root_pos || !t->traj_verts || !t->progress_buf || !t->sum_dev || !t->sum_sample_dev || !t->path_len || !t->max_dev || !t->prev_xy ||
        !t->last_sample_dev || !t->n_samples)
        return capi_fail(EMLOCO_E_ARG, "emloco_locoval_eval_track: a NULL tensor in EmlocoLocoValTrack");
    hipLaunchKernelGGL(emloco::locoval_eval_track_kernel, dim3((unsigned)((s->n_env + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *s, *t,
                       records, samples);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_locoval_track_reduce(int n_env, int games_per_env, const EmlocoLocoValTrackRecord *records, const int32_t *games, float fail_dist,
                                double *moments, void *stream) {
    if (n_env < 1 || games_per_env < 1 || !records || !games || !moments) return capi_fail(EMLOCO_E_ARG, "emloco_locoval_track_reduce: bad argument");
    hipLaunchKernelGGL(emloco::locoval_track_reduce_kernel, dim3(1), dim3(emloco::kEvalReduceThreads), 0, (hipStream_t)stream, n_env,
                       games_per_env, records, games, fail_dist, moments);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
