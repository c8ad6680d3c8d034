// TEST INFRASTRUCTURE ONLY: the evaluation of several LocoVal networks on the same games (emloco_amd/csrc/locoval_multi.h and the
// finish of eval_kernels.hip) on the CPU through tests/emu/hip/ (tests/test_locoval_eval_multi_cpu.py compiles it with
// emu/emu_runtime.cpp).  The single-network path it is compared with comes from the two glue files it includes, unchanged; the launch
// geometry of the two new entry points is the C ABI's (predictor_capi.hip, eval_capi.hip).
#include "emu_locoval_variants.cpp"
#include "emu_locoval_eval.cpp"

extern "C" int emu_locoval_eval_fwd_multi(const EmlocoLocoValEval *s, const EmlocoLocoValNets *nets) {
    const EmlocoLocoValEval t = *s;
    const EmlocoLocoValNets n = *nets;
    emu::launch((unsigned)t.n_env, 64, [&] {
        locoval_eval_fwd_multi_kernel(t.n_env, (const float *)t.traj13, (const float *)t.pose, (const float *)t.vel, (const float *)t.row_mask, n);
    });
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
