// TEST INFRASTRUCTURE ONLY: the flight recorder's kernels (emloco_amd/csrc/recorder_kernels.hip) on the CPU with the launch shapes of
// recorder_capi.hip, all arrays on the host.  Built into its own library by tests/emu_recorder.py together with emu_runtime.cpp.
#include "hip/hip_runtime.h"
#include "../../emloco_amd/csrc/recorder_kernels.hip"

static unsigned rec_grid(const EmlocoRecorderBufs &r, int jobs) {
    const int g = r.grid > 0 ? r.grid : jobs;
    return (unsigned)(g < 1024 ? g : 1024);
}

extern "C" int emu_recorder_record(const EmlocoRecorderBufs *rec, int t) {
    const EmlocoRecorderBufs r = *rec;
    emu::launch(rec_grid(r, r.n_env), emloco::kRecThreads, [&] { emloco::recorder_record_kernel(r, t); });
    blockIdx.x = 0;
    return 0;
}

extern "C" int emu_recorder_check(const EmlocoRecorderBufs *rec, int t) {
    const EmlocoRecorderBufs r = *rec;
    emu::launch(rec_grid(r, (r.n_env + emloco::kRecCauseWaves - 1) / emloco::kRecCauseWaves), 64 * emloco::kRecCauseWaves,
                [&] { emloco::recorder_cause_kernel(r, t); });
    emu::launch(1, emloco::kRecClaimThreads, [&] { emloco::recorder_claim_kernel(r, t); });
    emu::launch(rec_grid(r, r.n_slots), emloco::kRecCopyThreads, [&] { emloco::recorder_copy_kernel(r, t); });
    blockIdx.x = 0;
    return 0;
}
