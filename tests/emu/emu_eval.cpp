// TEST INFRASTRUCTURE ONLY: runs emloco_amd/csrc/eval_kernels.hip on the CPU through tests/emu/hip/.  The launch geometry is the C ABI's
// (eval_capi.hip).
#include <stdint.h>
#include "hip/hip_runtime.h"
#include "../../emloco_amd/csrc/eval_kernels.hip"

using namespace emloco;

extern "C" int emu_locoval_eval_step(const EmlocoLocoValEval *s, const float *reward_raw, const float *disc, const int64_t *dones,
                                     const int64_t *terminate, const uint8_t *inverted) {
    const EmlocoLocoValEval t = *s;
    emu::launch((unsigned)((t.n_env + 3) / 4), 256, [&] { locoval_eval_step_kernel(t, reward_raw, disc, dones, terminate, inverted); });
    blockIdx.x = 0;
    return 0;
}

extern "C" int emu_locoval_eval_track(const EmlocoLocoValEval *s, const EmlocoLocoValTrack *t, EmlocoLocoValTrackRecord *records,
                                      float *samples) {
    const EmlocoLocoValEval a = *s;
    const EmlocoLocoValTrack b = *t;
    emu::launch((unsigned)((a.n_env + 255) / 256), 256, [&] { locoval_eval_track_kernel(a, b, records, samples); });
    blockIdx.x = 0;
    return 0;
}

extern "C" int emu_locoval_eval_finish(const EmlocoLocoValEval *s, const float *value, EmlocoLocoValRecord *records) {
    const EmlocoLocoValEval t = *s;
    emu::launch((unsigned)((t.n_env + 255) / 256), 256, [&] { locoval_eval_finish_kernel(t, value, records); });
    blockIdx.x = 0;
    return 0;
}

extern "C" int emu_locoval_eval_finish_multi(const EmlocoLocoValEval *s, const EmlocoLocoValNets *nets, EmlocoLocoValRecord *records) {
    const EmlocoLocoValEval t = *s;
    const EmlocoLocoValNets n = *nets;
    emu::launch((unsigned)((t.n_env + 255) / 256), 256, [&] { locoval_eval_finish_multi_kernel(t, n, records); });
    blockIdx.x = 0;
    return 0;
}

extern "C" int emu_locoval_eval_reduce(int n_env, int games_per_env, const EmlocoLocoValRecord *records, const int32_t *games,
                                       double *moments) {
    emu::launch(1, kEvalReduceThreads, [&] { locoval_eval_reduce_kernel(n_env, games_per_env, records, games, moments); });
    return 0;
}

extern "C" int emu_locoval_track_reduce(int n_env, int games_per_env, const EmlocoLocoValTrackRecord *records, const int32_t *games,
                                        float fail_dist, double *moments) {
    emu::launch(1, kEvalReduceThreads, [&] { locoval_track_reduce_kernel(n_env, games_per_env, records, games, fail_dist, moments); });
    return 0;
}

extern "C" int emu_locoval_record_size() { return (int)sizeof(EmlocoLocoValRecord); }
extern "C" int emu_locoval_track_record_size() { return (int)sizeof(EmlocoLocoValTrackRecord); }
