// The host sequences around the device stages that more than one caller drives: the region finish, the =/X passes, the two-pass text kernels and
// the sdust launch classes.  Each exists once here; the mapper's lanes (backend_hip.cpp) and the C entry points (capi_*.cpp) call it over buffers
// they own, with their own stream, their own way of waiting and their own byte accounting.  Host code only: no .hip file includes this header.
#pragma once
#include <algorithm>
#include <cstring>
#include "hip_util.hpp"
#include "kernel_prof.hpp"
#include "region_finish.hpp"
#include "cigar_eqx.hpp"
#include "sdust.hpp"

namespace mm2amd {

// How a caller waits for its stream: a lane polls (stream_wait, hip_util.hpp), an entry point holds the device's shared stream and synchronises.
using StreamWait = void (*)(hipStream_t);
inline void stream_sync(hipStream_t s) { HIP_CHECK(hipStreamSynchronize(s)); }

// ---- region_finish_kernel (region_finish.hpp); prof null: the launch leaves no profile entry
// LDS slots per region for a launch whose longest stitched CIGAR has `longest` operations
inline int fin_cap_ops(uint32_t longest) { return (int)std::min<uint32_t>((std::max<uint32_t>(longest, 1u) + 63) & ~63u, (uint32_t)kFinMaxOps); }

inline void finish_run(const FinRegion *regions, int n, const FinPiece *pieces, const uint32_t *dp_pool, uint32_t *out_pool, FinResult *results, const uint8_t *qpool, const uint32_t *S,
                       const int8_t *mat25, int8_t q, int8_t e, bool log_gap, uint32_t longest, hipStream_t st, KernelProfiler *prof, double alg_bytes, double units)
{
	FinParams P;
	P.regions = regions, P.n_regions = n, P.pieces = pieces, P.cigar_pool = dp_pool, P.out_pool = out_pool, P.results = results;
	P.qpool = qpool, P.S = S;
	memcpy(P.mat, mat25, 25);
	P.q = q, P.e = e, P.log_gap = log_gap ? 1 : 0;
	P.cap_ops = fin_cap_ops(longest);
	if (prof) prof->begin(st);
	region_finish_launch(P, st);
	if (prof) prof->end(st, "region_finish_kernel", alg_bytes, units);
}

// ---- cigar_eqx_kernel (cigar_eqx.hpp) for regions region_finish_kernel has just finished on `st`: count, place, write
struct EqxBufs { DevBuf<uint32_t> d_n, d_out; DevBuf<uint64_t> d_off; PinBuf<uint32_t> h_n, h_out; PinBuf<uint64_t> h_off; }; // the regions' =/X lengths, their places, the pool
// Phase one: the counting pass, the wait for the counts, their exclusive sum (B.h_n, B.h_off; h_off[n] = the total, which is returned).
// P: regions, results, fin_pool, qpool and S are the caller's; the rest is filled here.
inline uint64_t eqx_count(EqxBufs &B, EqxParams &P, KernelProfiler &kp, double alg_bytes, hipStream_t st, StreamWait wait)
{
	const size_t n = (size_t)P.n_regions;
	P.n_ops = B.d_n.ensure(n), P.out_off = B.d_off.ensure(n);
	uint32_t *hn = B.h_n.ensure(n);
	uint64_t *ho = B.h_off.ensure(n + 1);
	kp.begin(st);
	cigar_eqx_launch(P, false, st);
	kp.end(st, "cigar_eqx_kernel[count]", alg_bytes, (double)n);
	HIP_CHECK(hipMemcpyAsync(hn, B.d_n.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	wait(st);
	uint64_t total = 0;
	for (size_t i = 0; i < n; ++i) ho[i] = total, total += hn[i];
	ho[n] = total;
	return total;
}
// Phase two: the places go up, the writing pass fills a pool of exactly `total` operations.  The copy of the pool is queued; the caller waits for the stream.
inline EqxOut eqx_write(EqxBufs &B, EqxParams &P, uint64_t total, KernelProfiler &kp, double alg_bytes, hipStream_t st)
{
	const size_t n = (size_t)P.n_regions;
	HIP_CHECK(hipMemcpyAsync(B.d_off.p, B.h_off.p, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
	P.out_pool = B.d_out.ensure(total + 1);
	uint32_t *hout = B.h_out.ensure(total + 1);
	kp.begin(st);
	cigar_eqx_launch(P, true, st);
	kp.end(st, "cigar_eqx_kernel[write]", alg_bytes, (double)n);
	if (total) HIP_CHECK(hipMemcpyAsync(hout, B.d_out.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	return EqxOut{ B.h_n.p, B.h_off.p, hout };
}

// ---- the text kernels (aln_text.hpp, rec_text.hpp, junc_text.hpp): a sizing pass, the host's offsets, a writing pass.  P is TxtParams or RecParams
// with jobs, n_jobs, res and the sources set; `launch` is the kernel's launcher.  Placing the jobs in the pool between the phases is the caller's:
// h_off are their places (n_jobs of them), d_out has room for `total` bytes, which come back into h_out.
template <typename P, typename Res>
void text_size_pass(P &prm, void (*launch)(const P &, bool, void *), Res *h_res, KernelProfiler &prof, const char *name, double alg_bytes, double units, hipStream_t st, StreamWait wait)
{
	prm.off = nullptr, prm.out = nullptr;
	prof.begin(st);
	launch(prm, false, st);
	prof.end(st, name, alg_bytes, units);
	HIP_CHECK(hipMemcpyAsync(h_res, prm.res, (size_t)prm.n_jobs * sizeof(Res), hipMemcpyDeviceToHost, st));
	wait(st);
}
template <typename P>
void text_write_pass(P &prm, void (*launch)(const P &, bool, void *), const uint64_t *h_off, uint64_t *d_off, char *d_out, char *h_out, uint64_t total, KernelProfiler &prof, const char *name,
                     double alg_bytes, double units, hipStream_t st, StreamWait wait)
{
	HIP_CHECK(hipMemcpyAsync(d_off, h_off, (size_t)prm.n_jobs * 8, hipMemcpyHostToDevice, st));
	prm.off = d_off, prm.out = d_out;
	prof.begin(st);
	launch(prm, true, st);
	prof.end(st, name, alg_bytes, units);
	HIP_CHECK(hipMemcpyAsync(h_out, d_out, total, hipMemcpyDeviceToHost, st));
	wait(st);
}

// ---- sdust_kernel's launch classes (sdust.hpp).  The switches are read at every call.
inline bool sdust_env_no_narrow() { const char *e = getenv("MM2AMD_SDUST_NO_NARROW"); return e && *e && strcmp(e, "0") != 0; }
inline int sdust_env_narrow_cap()
{
	const char *e = getenv("MM2AMD_SDUST_NARROW_CAP");
	const long v = e && *e ? strtol(e, nullptr, 10) : kSdustNarrowCap;
	return (int)(v < 1 ? 1 : v > kSdustWideCap ? kSdustWideCap : v);
}
// wide: SdustParams::wide (0: the narrow class; 1: the wide class over the list; 2: the wide class over every read); grid: as sdust_launch takes it
inline void sdust_run_class(SdustParams &P, int wide, int grid, KernelProfiler &prof, double units, hipStream_t st)
{
	P.cap = wide ? kSdustWideCap : sdust_env_narrow_cap(), P.wide = wide;
	prof.begin(st);
	sdust_launch(P, grid, st);
	prof.end(st, wide ? "sdust_kernel[wide]" : "sdust_kernel[narrow]", 0.0, units);
}

} // namespace mm2amd
