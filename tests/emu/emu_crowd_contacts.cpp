// TEST INFRASTRUCTURE ONLY: the crowd contact audit's kernels (emloco_amd/csrc/crowd_contact_kernels.hip) on the CPU with the launch
// shapes of crowd_capi.hip, all arrays on the host.  Built into its own library by tests/emu_crowd_contacts.py together with
// emu_runtime.cpp.
#include "hip/hip_runtime.h"
#include "../../emloco_amd/csrc/crowd_contact_kernels.hip"

static const char *g_why = "";
static int refuse(const char *why) { g_why = why ? why : ""; return why ? -1 : 0; }

extern "C" const char *emu_crowd_contacts_error(void) { return g_why; }

// `grid` > 0: that many workgroups stride over the envs (the result does not depend on it)
extern "C" int emu_crowd_contacts(const EmlocoCrowdContacts *cc, EmlocoCrowdContactNow *now, int grid) {
    if (refuse(emloco::crowd_contacts_refusal(cc, now, false))) return -1;
    const EmlocoCrowdContacts c = *cc;
    const int blocks = (c.n_env + emloco::kContactWaves - 1) / emloco::kContactWaves;
    const unsigned g = (unsigned)(grid > 0 && grid < blocks ? grid : blocks);
    emu::launch(g, emloco::kContactThreads, [&] { emloco::crowd_contact_prep_kernel(c); });
    emu::launch(g, emloco::kContactThreads, [&] { emloco::crowd_contact_kernel(c, now); });
    blockIdx.x = 0;
    return 0;
}

extern "C" int emu_crowd_contacts_accumulate(const EmlocoCrowdContacts *cc, const EmlocoCrowdContactNow *now) {
    if (refuse(emloco::crowd_contacts_refusal(cc, now, true))) return -1;
    const EmlocoCrowdContacts c = *cc;
    emu::launch((unsigned)((c.n_env + 255) / 256), 256, [&] { emloco::crowd_contact_accumulate_kernel(c, now); });
    blockIdx.x = 0;
    return 0;
}

extern "C" int emu_crowd_contacts_reduce(int n_env, int games_per_env, const EmlocoCrowdContactRecord *records, const int32_t *games, double *moments) {
    if (refuse(emloco::crowd_contacts_reduce_refusal(n_env, games_per_env, records, games, moments))) return -1;
    emu::launch(1, emloco::kContactReduceThreads, [&] { emloco::crowd_contact_reduce_kernel(n_env, games_per_env, records, games, moments); });
    return 0;
}

extern "C" int emu_crowd_contacts_epoch_reduce(int n_env, double *totals, double *epoch) {
    if (refuse(n_env < 1 ? "n_env < 1" : !totals ? "null totals" : !epoch ? "null epoch" : nullptr)) return -1;
    emu::launch(1, emloco::kContactReduceThreads, [&] { emloco::crowd_contact_epoch_kernel(n_env, totals, epoch); });
    return 0;
}
