// crowd_capi.hip -- C ABI (include/emloco_task.h) over the crowd-aware terrain sensor's kernels, the crowd contact audit's and the
// group observation's and the crowd spawn's.
#include <hip/hip_runtime.h>
#include "crowd_kernels.hip"
#include "crowd_contact_kernels.hip"
#include "crowd_people_kernels.hip"
#include "crowd_spawn_kernels.hip"
#include "capi_error.h"

using emloco::capi_fail;

namespace {
constexpr int kCrowdMaxGrid = 4096;
unsigned crowd_grid(int jobs) { return (unsigned)(jobs < kCrowdMaxGrid ? jobs : kCrowdMaxGrid); }
}  // namespace

extern "C" {

int emloco_task_crowd_sensor(const EmlocoCrowdBufs *bufs, const int32_t *dev_env_ids, int n, void *stream) {
    const char *who = "emloco_task_crowd_sensor";
    if (const char *why = emloco::crowd_refusal(bufs, n)) return capi_fail(EMLOCO_E_ARG, who, why);
    hipStream_t st = (hipStream_t)stream;
    const int rows = dev_env_ids ? n : bufs->n_env;
    if (rows == 0) return 0;
    if (bufs->stamps) {
        hipLaunchKernelGGL(emloco::crowd_stamp_kernel, dim3(crowd_grid(bufs->n_env)), dim3(emloco::kCrowdThreads), 0, st, *bufs);
        EMLOCO_HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(emloco::crowd_gather_kernel, dim3(crowd_grid(rows)), dim3(emloco::kCrowdThreads), 0, st, *bufs, dev_env_ids, rows);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_crowd_contacts(const EmlocoCrowdContacts *c, EmlocoCrowdContactNow *now, void *stream) {
    const char *who = "emloco_crowd_contacts";
    if (const char *why = emloco::crowd_contacts_refusal(c, now, false)) return capi_fail(EMLOCO_E_ARG, who, why);
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = crowd_grid((c->n_env + emloco::kContactWaves - 1) / emloco::kContactWaves);
    hipLaunchKernelGGL(emloco::crowd_contact_prep_kernel, dim3(grid), dim3(emloco::kContactThreads), 0, st, *c);
    EMLOCO_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(emloco::crowd_contact_kernel, dim3(grid), dim3(emloco::kContactThreads), 0, st, *c, now);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_crowd_contacts_accumulate(const EmlocoCrowdContacts *c, const EmlocoCrowdContactNow *now, void *stream) {
    const char *who = "emloco_crowd_contacts_accumulate";
    if (const char *why = emloco::crowd_contacts_refusal(c, now, true)) return capi_fail(EMLOCO_E_ARG, who, why);
    hipLaunchKernelGGL(emloco::crowd_contact_accumulate_kernel, dim3((unsigned)((c->n_env + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *c, now);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_crowd_contacts_reduce(int n_env, int games_per_env, const EmlocoCrowdContactRecord *records, const int32_t *games,
                                 double *moments, void *stream) {
    const char *who = "emloco_crowd_contacts_reduce";
    if (const char *why = emloco::crowd_contacts_reduce_refusal(n_env, games_per_env, records, games, moments)) return capi_fail(EMLOCO_E_ARG, who, why);
    hipLaunchKernelGGL(emloco::crowd_contact_reduce_kernel, dim3(1), dim3(emloco::kContactReduceThreads), 0, (hipStream_t)stream, n_env,
                       games_per_env, records, games, moments);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_crowd_contacts_epoch_reduce(int n_env, double *totals, double *epoch, void *stream) {
    const char *who = "emloco_crowd_contacts_epoch_reduce";
    if (n_env < 1) return capi_fail(EMLOCO_E_ARG, who, "n_env < 1");
    if (!totals) return capi_fail(EMLOCO_E_ARG, who, "null totals");
    if (!epoch) return capi_fail(EMLOCO_E_ARG, who, "null epoch");
    hipLaunchKernelGGL(emloco::crowd_contact_epoch_kernel, dim3(1), dim3(emloco::kContactReduceThreads), 0, (hipStream_t)stream, n_env, totals, epoch);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_task_crowd_people(const EmlocoCrowdPeople *p, const int32_t *dev_env_ids, int n, void *stream) {
    const char *who = "emloco_task_crowd_people";
    if (const char *why = emloco::crowd_people_refusal(p, n)) return capi_fail(EMLOCO_E_ARG, who, why);
    hipStream_t st = (hipStream_t)stream;
    const int rows = dev_env_ids ? n : p->n_env;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(emloco::crowd_people_roots_kernel, dim3((unsigned)((p->n_env + 255) / 256)), dim3(256), 0, st, *p);
    EMLOCO_HIPCHK(hipGetLastError());
    const unsigned grid = crowd_grid((rows + emloco::kPeopleWaves - 1) / emloco::kPeopleWaves);
    hipLaunchKernelGGL(emloco::crowd_people_kernel, dim3(grid), dim3(emloco::kPeopleThreads), 0, st, *p, dev_env_ids, rows);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

int emloco_task_crowd_spawn(const EmlocoCrowdSpawn *s, const int32_t *dev_env_ids, int n, const float *u, void *stream) {
    const char *who = "emloco_task_crowd_spawn";
    if (const char *why = emloco::crowd_spawn_refusal(s, dev_env_ids, n, u)) return capi_fail(EMLOCO_E_ARG, who, why);
    hipStream_t st = (hipStream_t)stream;
    const int rows = dev_env_ids ? n : s->n_env;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(emloco::crowd_spawn_mark_kernel, dim3((unsigned)((rows + emloco::kSpawnMarkThreads - 1) / emloco::kSpawnMarkThreads)),
                       dim3(emloco::kSpawnMarkThreads), 0, st, *s, dev_env_ids, rows);
    EMLOCO_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(emloco::crowd_spawn_place_kernel, dim3((unsigned)(s->n_env / s->group_size)), dim3((unsigned)(s->tries * 64)), 0, st, *s, u, rows);
    EMLOCO_HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
