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
#include "pair.hpp"
#include "threads.hpp"

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

// ---- pair_kernel (pair.hpp): the fragments by class, one launch per class, the host class and the unmapped mates answered here.  hits, out, frag
// and res are the caller's (any host memory; a lane passes pinned buffers); arguments are checked by the caller.
struct PairBufs {
	DevBuf<mm2amd_pe_hit_t> d_hits; DevBuf<mm2amd_pe_out_t> d_out; DevBuf<mm2amd_pe_frag_t> d_frag; DevBuf<mm2amd_pe_res_t> d_res;
	DevBuf<uint32_t> d_list; PinBuf<uint32_t> h_list;
	DevBuf<float> d_logf; PinBuf<float> h_logf; bool logf_ready = false; // logf(1) .. logf(kPeLogTable) from the host's libm, filled when first needed
	std::vector<uint32_t> host_list;
};
// the hits the fragments span: [*first, *last)
inline void pair_span(int n_frag, const mm2amd_pe_frag_t *frag, uint64_t *first, uint64_t *last)
{
	uint64_t lo = ~(uint64_t)0, hi = 0;
	for (int f = 0; f < n_frag; ++f) {
		const uint64_t m = (uint64_t)frag[f].n[0] + (uint64_t)frag[f].n[1];
		if (m == 0) continue;
		lo = std::min(lo, frag[f].hit0), hi = std::max(hi, frag[f].hit0 + m);
	}
	*first = hi ? lo : 0, *last = hi;
}
inline void pair_run(PairBufs &B, int n_frag, const mm2amd_pe_frag_t *frag, const mm2amd_pe_hit_t *hits, const mm2amd_pe_opt_t &opt, mm2amd_pe_out_t *out, mm2amd_pe_res_t *res,
                     int n_threads, KernelProfiler &prof, hipStream_t st, StreamWait wait)
{
	const size_t n = (size_t)n_frag;
	if (n == 0) return;
	uint64_t first = 0, last = 0;
	pair_span(n_frag, frag, &first, &last);
	const uint64_t total = last - first;
	// the fragments by class: narrow ones from the front of the list, wide ones from its end; an unmapped mate is answered below, the rest is the host's
	uint32_t *const h_list = B.h_list.ensure(n);
	size_t n_narrow = 0, n_wide = 0;
	double narrow_ends = 0, wide_ends = 0;
	for (size_t f = 0; f < n; ++f) {
		const uint64_t m = (uint64_t)frag[f].n[0] + (uint64_t)frag[f].n[1];
		pe_res_none(res[f], MM2AMD_PE_PATH_HOST, MM2AMD_PE_OK);
		if (frag[f].n[0] == 0 || frag[f].n[1] == 0) res[f].path = MM2AMD_PE_PATH_NARROW;
		else if (m <= (uint64_t)kPeNarrowCap) h_list[n_narrow++] = (uint32_t)f, narrow_ends += (double)m;
		else if (m <= (uint64_t)kPeWideCap) h_list[n - 1 - n_wide++] = (uint32_t)f, wide_ends += (double)m;
	}
	if (n_narrow + n_wide > 0) {
		if (!B.logf_ready) {
			float *t = B.h_logf.ensure((size_t)kPeLogTable + 1, 1.0);
			t[0] = 0.0f;
			for (int k = 1; k <= kPeLogTable; ++k) t[k] = logf((float)k);
			B.d_logf.ensure((size_t)kPeLogTable + 1, 1.0);
			HIP_CHECK(hipMemcpyAsync(B.d_logf.p, t, ((size_t)kPeLogTable + 1) * sizeof(float), hipMemcpyHostToDevice, st));
			B.logf_ready = true;
		}
		B.d_hits.ensure(total + 1), B.d_out.ensure(total + 1), B.d_frag.ensure(n), B.d_res.ensure(n), B.d_list.ensure(n);
		prof.begin(st); // (the copies have rows of their own in the profile: the call is bound by them)
		HIP_CHECK(hipMemcpyAsync(B.d_hits.p, hits + first, total * sizeof(mm2amd_pe_hit_t), hipMemcpyHostToDevice, st));
		HIP_CHECK(hipMemcpyAsync(B.d_frag.p, frag, n * sizeof(mm2amd_pe_frag_t), hipMemcpyHostToDevice, st));
		HIP_CHECK(hipMemcpyAsync(B.d_list.p, h_list, n * 4, hipMemcpyHostToDevice, st));
		HIP_CHECK(hipMemcpyAsync(B.d_res.p, res, n * sizeof(mm2amd_pe_res_t), hipMemcpyHostToDevice, st));
		prof.end(st, "pair_copy[up]", (double)total * sizeof(mm2amd_pe_hit_t) + (double)n * (sizeof(mm2amd_pe_frag_t) + 4 + sizeof(mm2amd_pe_res_t)));
		PairParams P;
		P.hits = B.d_hits.p, P.first = first, P.frag = B.d_frag.p, P.out = B.d_out.p, P.res = B.d_res.p, P.opt = opt, P.logf_tab = B.d_logf.p;
		if (n_narrow) {
			P.list = B.d_list.p, P.n_list = (int)n_narrow, P.cap = kPeNarrowCap, P.path = MM2AMD_PE_PATH_NARROW;
			prof.begin(st);
			pair_launch(P, st);
			prof.end(st, "pair_kernel[narrow]", 0.0, narrow_ends);
		}
		if (n_wide) {
			P.list = B.d_list.p + (n - n_wide), P.n_list = (int)n_wide, P.cap = kPeWideCap, P.path = MM2AMD_PE_PATH_WIDE;
			prof.begin(st);
			pair_launch(P, st);
			prof.end(st, "pair_kernel[wide]", 0.0, wide_ends);
		}
		prof.begin(st);
		HIP_CHECK(hipMemcpyAsync(res, B.d_res.p, n * sizeof(mm2amd_pe_res_t), hipMemcpyDeviceToHost, st));
		HIP_CHECK(hipMemcpyAsync(out + first, B.d_out.p, total * sizeof(mm2amd_pe_out_t), hipMemcpyDeviceToHost, st));
		prof.end(st, "pair_copy[down]", (double)total * sizeof(mm2amd_pe_out_t) + (double)n * sizeof(mm2amd_pe_res_t));
		wait(st);
		prof.collect();
	}
	// what no launch answered: an unmapped mate (nothing changes), and the host class -- by size, or because the kernel met equal keys among more
	// than 64 ends
	B.host_list.clear();
	for (size_t f = 0; f < n; ++f) {
		if (frag[f].n[0] == 0 || frag[f].n[1] == 0 || res[f].path == MM2AMD_PE_PATH_HOST) B.host_list.push_back((uint32_t)f);
		else if (res[f].best[0] >= frag[f].n[0] || res[f].best[1] >= frag[f].n[1]) throw HipError("[mm2amd] pair_kernel: a pair outside its fragment");
	}
	parallel_for(n_threads, (long)B.host_list.size(), [&](long k, int) {
		const uint32_t f = B.host_list[(size_t)k];
		pe_host_fragment(frag[f], hits + frag[f].hit0, opt, out + frag[f].hit0, res + f, res[f].path);
	}, 64);
}

} // namespace mm2amd
