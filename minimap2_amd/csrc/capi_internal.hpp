// What the translation units behind the C ABI (include/mm2amd.h) share: the thread's last error, the exception boundary, and the functions one
// capi_*.cpp or the backend defines for another.  No HIP here: capi_map.cpp and capi_common.cpp are also built into the checker library, which has none
// (the scope object that makes a device current is DeviceScope, device_ctx.hpp).
#pragma once
#include <string>
#include <vector>
#include "../../include/mm2amd.h"

namespace mm2amd {

class Backend; struct DeviceCtx; struct FlatIndex; struct TxtJob; struct RecJob; struct RecHit;

// capi_common.cpp
void capi_set_error(const std::string &msg);               // what mm2amd_last_error() returns, without a code
int capi_fail(int code, const std::string &msg);           // ... with one; returns `code`
int effective_cpus();                                      // the CPUs this process can really use: hardware threads, capped by the container's CPU quota
void apply_hw_queue_default();                             // GPU_MAX_HW_QUEUES, before this process's first HIP call when that call is ours

// The exception boundary of an entry point: an IdxIoError is MM2AMD_EIO, a HipError MM2AMD_ENODEV ("no HIP device") or MM2AMD_EHIP, any other
// std::exception MM2AMD_EINVAL.  capi_fail_current (device_ctx.cpp) looks at the exception in flight.
int capi_fail_current();
template <typename F> int guarded(F &&f) { try { return f(); } catch (...) { return capi_fail_current(); } }

// backend_hip.cpp in the product: `device` < 0 = the process's default device; `replica` numbers the backends of one context;
// `tables_device` is where `device_tables` live (a backend on another device copies them)
Backend *make_backend(const FlatIndex &fi, void *device_tables, int n_threads, int device, int replica, int tables_device);
int backend_device_count();
// The minimizer tables of `fi` (sequence table and packed sequence set) built by the backend on `device` (< 0: the default one);
// returns the tables (for make_backend's device_tables; *on_device = their device) or nullptr when this backend wants host tables.
void *backend_build_index_tables(FlatIndex &fi, int device, int *on_device);
void backend_free_index_tables(void *tables);
const char *backend_name();

// capi_kernels.cpp.  The two passes of aln_text_kernel around the host's offsets; shared by mm2amd_aln_text_batch and mm2amd_hits_text_batch (capi_index.cpp).
// The caller holds dc.mu and has made the device current.  hq / ht: the jobs' byte pools (q_pos / t_pos of the kTxtQ* / kTxtTCodes sources
// index them); dS: a packed reference already on the device (kTxtTPacked*), or null.
int aln_text_run(DeviceCtx &dc, const std::vector<TxtJob> &jobs, int what, const std::vector<uint8_t> &hq, const std::vector<uint8_t> &ht, const uint32_t *dS,
                 const std::vector<uint32_t> &cig, mm2amd_txt_res_t *res, char *pool, size_t pool_cap);
// The two passes of junc_text_kernel for mm2amd_hits_junc_batch (capi_index.cpp); the caller holds dc.mu and has made the device current.
// jobs / hits: one of each per hit that can write, in hit order; slot[k]: the hit's place in res (n_res entries, the others get len 0, status 0);
// names / tnames: the read and target names the jobs and hits point into (hits[k].rid indexes tname_off); dS: the handle's packed sequence.
int junc_text_run(DeviceCtx &dc, const std::vector<RecJob> &jobs, const std::vector<RecHit> &hits, const std::vector<int> &slot, int n_res, const std::string &names,
                  const std::string &tnames, const std::vector<uint64_t> &tname_off, const uint32_t *dS, const std::vector<uint32_t> &cig, mm2amd_txt_res_t *res, char *pool,
                  size_t pool_cap);

} // namespace mm2amd
