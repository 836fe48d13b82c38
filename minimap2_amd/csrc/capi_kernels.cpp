// C ABI of libmm2amd.so (declared in include/mm2amd.h): the kernel-level entry points.
#include <map>
#include <algorithm>
#include <cstring>
#include "capi_internal.hpp"
#include "device_ctx.hpp"
#include "ksw_host.hpp"
#include "stage_run.hpp"
#include "ksw_ll.hpp"
#include "aln_text.hpp"
#include "junc_text.hpp"
#include "sdust_core.hpp"
#include "fastx.hpp"
#include "tables.hpp"
#include "threads.hpp"
#include "trace.hpp"
#include "device_sort.hpp"
#include "seed_chain_dev.hpp"
#include "kernel_prof.hpp"
#include "hits_merge.hpp"
#include "split_merge.hpp"
#include "index_handle.hpp"

using namespace mm2amd;

namespace {

struct KernelApiState { // buffers of the kernel-level entry points
	KswRunner ksw;
	DevBuf<uint8_t> d_qpool, d_tpool;
};
KernelApiState &kstate() { static KernelApiState s; return s; }

struct LlApiState { // mm2amd_ksw_ll_batch: kept between calls
	DevBuf<uint8_t> d_q, d_t;
	DevBuf<LlJob> d_jobs;
	DevBuf<LlRes> d_res;
	DevBuf<uint32_t> d_bnd;
	PinBuf<uint8_t> h_q, h_t; // the pools are gathered in pinned memory: the uploads are then asynchronous copies in stream order
	PinBuf<LlJob> h_jobs;
	PinBuf<LlRes> h_res;
};
LlApiState &ll_state() { static LlApiState s; return s; }
constexpr size_t kLlBndBudget = (size_t)1 << 26; // words of boundary columns per launch (256 MB): a batch that needs more is launched in parts

bool ll_no_wg() { const char *e = getenv("MM2AMD_LL_NO_WG"); return e && *e && strcmp(e, "0") != 0; }
int64_t ll_wg_min_cells() { const char *e = getenv("MM2AMD_LL_WG_MIN_CELLS"); return e && *e ? (int64_t)strtoll(e, nullptr, 10) : kLlWgMinCells; }

struct SdustApiState { // mm2amd_sdust_batch: kept between calls
	DevBuf<uint8_t> d_codes;
	DevBuf<uint64_t> d_off, d_out_off, d_out;
	DevBuf<uint32_t> d_reg_n, d_reg_s, d_reg_e, d_list, d_cnt_out;
	DevBuf<SdustCounters> d_cnt;
	PinBuf<uint8_t> h_codes;
	PinBuf<uint64_t> h_off;
	PinBuf<uint32_t> h_list;
};
SdustApiState &sdust_state() { static SdustApiState s; return s; }

int sdust_check_args(const char *who, int n_jobs, const mm2amd_sdust_job_t *jobs, int T, const mm2amd_sdust_res_t *res)
{
	if (n_jobs < 0 || T <= 0 || (n_jobs > 0 && (!jobs || !res))) return capi_fail(MM2AMD_EINVAL, std::string("[mm2amd] ") + who + ": bad arguments (T must be positive)");
	for (int i = 0; i < n_jobs; ++i)
		if (jobs[i].len < 0 || jobs[i].len > kSdustMaxLen || (jobs[i].len > 0 && !jobs[i].seq)) return capi_fail(MM2AMD_EINVAL, std::string("[mm2amd] ") + who + ": bad job (negative or excessive length, or null sequence)");
	return 0;
}

struct HitsMergeApiState { // mm2amd_hits_merge_batch: kept between calls
	DevBuf<mm2amd_hm_hit_t> d_hits;
	DevBuf<mm2amd_hm_out_t> d_out;
	DevBuf<mm2amd_hm_seg_t> d_seg;
	DevBuf<uint64_t> d_off;
	DevBuf<uint32_t> d_list;
	PinBuf<uint32_t> h_list;
};
HitsMergeApiState &hm_state() { static HitsMergeApiState s; return s; }

int hm_check_args(const char *who, int n_seg, const uint64_t *seg_off, const mm2amd_hm_hit_t *hits, const mm2amd_hm_opt_t *opt, const mm2amd_hm_out_t *out,
                  const mm2amd_hm_seg_t *seg)
{
	if (n_seg < 0 || (n_seg > 0 && (!seg_off || !opt || !seg))) return capi_fail(MM2AMD_EINVAL, std::string("[mm2amd] ") + who + ": bad arguments");
	for (int s = 0; s < n_seg; ++s)
		if (seg_off[s + 1] < seg_off[s] || seg_off[s + 1] - seg_off[s] > (uint64_t)kHmMaxHits)
			return capi_fail(MM2AMD_EINVAL, std::string("[mm2amd] ") + who + ": bad offsets (descending, or a segment above the hit limit)");
	if (n_seg > 0 && seg_off[n_seg] > seg_off[0] && (!hits || !out)) return capi_fail(MM2AMD_EINVAL, std::string("[mm2amd] ") + who + ": hits without arrays");
	return 0;
}

struct PairApiState { PairBufs bufs; }; // mm2amd_pair_batch: kept between calls
PairApiState &pe_state() { static PairApiState s; return s; }

int pe_check_args(const char *who, int n_frag, const mm2amd_pe_frag_t *frag, const mm2amd_pe_hit_t *hits, const mm2amd_pe_opt_t *opt, const mm2amd_pe_out_t *out,
                  const mm2amd_pe_res_t *res, std::vector<uint32_t> &order)
{
	if (n_frag < 0 || (n_frag > 0 && (!frag || !opt || !res))) return capi_fail(MM2AMD_EINVAL, std::string("[mm2amd] ") + who + ": bad arguments");
	if (n_frag > 0 && opt->match_sc <= 0) return capi_fail(MM2AMD_EINVAL, std::string("[mm2amd] ") + who + ": match_sc must be positive");
	bool ascending = true;
	uint64_t end = 0, lo = ~(uint64_t)0, hi = 0;
	for (int f = 0; f < n_frag; ++f) {
		const mm2amd_pe_frag_t &F = frag[f];
		if (F.n[0] < 0 || F.n[1] < 0 || F.n[0] > kPeMaxHits || F.n[1] > kPeMaxHits || F.hit0 > (uint64_t)1 << 48)
			return capi_fail(MM2AMD_EINVAL, std::string("[mm2amd] ") + who + ": bad fragment (a negative count, or a segment above the hit limit)");
		const uint64_t m = (uint64_t)F.n[0] + (uint64_t)F.n[1];
		if (m == 0) continue;
		ascending = ascending && F.hit0 >= end;
		end = F.hit0 + m, lo = std::min(lo, F.hit0), hi = std::max(hi, end);
	}
	if (hi == 0) return 0;
	if (!hits || !out) return capi_fail(MM2AMD_EINVAL, std::string("[mm2amd] ") + who + ": hits without arrays");
	if (hi - lo > (uint64_t)1 << 31) return capi_fail(MM2AMD_EINVAL, std::string("[mm2amd] ") + who + ": the fragments span more than 2^31 hits");
	if (!ascending) { // (the usual batch lists its fragments in the order of their hits: one pass above; otherwise by start)
		order.clear();
		for (int f = 0; f < n_frag; ++f) if (frag[f].n[0] + frag[f].n[1] > 0) order.push_back((uint32_t)f);
		std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return frag[a].hit0 < frag[b].hit0; });
		for (size_t k = 1; k < order.size(); ++k) {
			const mm2amd_pe_frag_t &A = frag[order[k - 1]];
			if (A.hit0 + (uint64_t)A.n[0] + (uint64_t)A.n[1] > frag[order[k]].hit0) return capi_fail(MM2AMD_EINVAL, std::string("[mm2amd] ") + who + ": the fragments' hit ranges overlap");
		}
	}
	return 0;
}

struct FastxApiState { // mm2amd_fastx_parse: kept between calls; one call at a time on a stream of its own
	std::mutex mu;
	hipStream_t stream = nullptr;
	DevBuf<uint8_t> d_text, d_pool;
	DevBuf<uint32_t> d_tile, d_line, d_dst, d_ridx, d_name, d_state;
	DevBuf<uint2> d_work;
	DevBuf<FastxDevRec> d_recs;
	PinBuf<uint32_t> h_word;
	PinBuf<FastxDevRec> h_recs;
	double times[6] = { 0, 0, 0, 0, 0, 0 }; // upload, device work up to the sizes, copy kernels, download, the host's table, the host's parser
};
FastxApiState &fastx_state() { static FastxApiState *s = new FastxApiState; return *s; } // (never destroyed: the stream belongs to a runtime that may be gone first)
KernelProfiler &fastx_prof() { return kernel_profiler(kMaxProfLanes - 2, kMaxReplicas - 1); } // (a slot no mapper lane and no record formatter of fewer than 16 replicas uses)

uint32_t fastx_long_line()
{
	const char *e = getenv("MM2AMD_FASTX_LONG_LINE");
	const long v = e && *e ? strtol(e, nullptr, 10) : (long)kFastxLongLine;
	return (uint32_t)(v < 16 ? 16 : v > (long)kFastxMaxText ? (long)kFastxMaxText : v);
}

int fastx_check_args(const char *who, const char *text, size_t len, size_t *n_recs, size_t *pool_len, size_t *consumed, int *path, size_t max_len)
{
	if (!n_recs || !pool_len || !consumed || !path || (len > 0 && !text) || len > max_len)
		return capi_fail(MM2AMD_EINVAL, std::string("[mm2amd] ") + who + ": bad arguments (a null pointer, or a text above the length limit)");
	*n_recs = 0, *pool_len = 0, *consumed = 0, *path = MM2AMD_FASTX_PATH_HOST;
	return 0;
}

// the host's parser behind both entry points
int fastx_host(const char *who, const char *text, size_t len, int is_final, int flags, mm2amd_fastx_rec_t *recs, size_t recs_cap, char *pool, size_t pool_cap,
               size_t *n_recs, size_t *pool_len, size_t *consumed)
{
	const bool sizing = !recs || !pool;
	FastxSink out(sizing ? nullptr : recs, recs_cap, sizing ? nullptr : pool, pool_cap);
	const size_t used = fastx_parse_host(text, len, is_final != 0, flags, out);
	*n_recs = out.n_recs, *pool_len = out.pool_len, *consumed = !is_final && out.n_recs == 0 ? 0 : used;
	if (!sizing && (out.n_recs > recs_cap || out.pool_len > pool_cap)) return capi_fail(MM2AMD_ENOMEM, std::string("[mm2amd] ") + who + ": table or pool too small (a call with recs == NULL gives the sizes)");
	return 0;
}

} // namespace

namespace mm2amd {

int aln_text_run(DeviceCtx &dc, const std::vector<TxtJob> &jobs, int what, const std::vector<uint8_t> &hq, const std::vector<uint8_t> &ht, const uint32_t *dS,
                 const std::vector<uint32_t> &cig, mm2amd_txt_res_t *res, char *pool, size_t pool_cap)
{
	const int n_jobs = (int)jobs.size();
	DevBuf<uint8_t> d_q, d_t;
	DevBuf<uint32_t> d_cig;
	DevBuf<TxtJob> d_jobs;
	DevBuf<TxtRes> d_res;
	DevBuf<uint64_t> d_off;
	DevBuf<char> d_out;
	d_q.ensure(hq.size() + 1), d_t.ensure(ht.size() + 1), d_cig.ensure(cig.size() + 1), d_jobs.ensure(n_jobs), d_res.ensure(n_jobs), d_off.ensure(n_jobs);
	if (!hq.empty()) HIP_CHECK(hipMemcpyAsync(d_q.p, hq.data(), hq.size(), hipMemcpyHostToDevice, dc.stream));
	if (!ht.empty()) HIP_CHECK(hipMemcpyAsync(d_t.p, ht.data(), ht.size(), hipMemcpyHostToDevice, dc.stream));
	if (!cig.empty()) HIP_CHECK(hipMemcpyAsync(d_cig.p, cig.data(), cig.size() * 4, hipMemcpyHostToDevice, dc.stream));
	HIP_CHECK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)n_jobs * sizeof(TxtJob), hipMemcpyHostToDevice, dc.stream));
	TxtParams P;
	P.jobs = d_jobs.p, P.n_jobs = n_jobs, P.what = what, P.qpool = d_q.p, P.tpool = d_t.p, P.S = dS, P.cigar = d_cig.p, P.res = d_res.p;
	KernelProfiler &prof = kernel_profiler(0);
	std::vector<TxtRes> hr(n_jobs);
	text_size_pass(P, aln_text_launch, hr.data(), prof, "aln_text_kernel[size]", 0.0, 0.0, dc.stream, stream_sync);
	std::vector<uint64_t> off(n_jobs);
	uint64_t total = 0;
	double cols = 0;
	for (int i = 0; i < n_jobs; ++i) {
		off[i] = total;
		res[i].off = total, res[i].len = hr[i].len, res[i].status = hr[i].status;
		total += hr[i].len, cols += (double)hr[i].cols;
	}
	prof.add_units("aln_text_kernel[size]", cols);
	if (pool && total > pool_cap) { prof.collect(); return capi_fail(MM2AMD_ENOMEM, "[mm2amd] alignment text: pool too small (a call with pool == NULL gives the lengths)"); }
	if (pool && total) text_write_pass(P, aln_text_launch, off.data(), d_off.p, d_out.ensure(total, 1.0), pool, total, prof, "aln_text_kernel[write]", (double)total, cols, dc.stream, stream_sync);
	prof.collect();
	return 0;
}

int junc_text_run(DeviceCtx &dc, const std::vector<RecJob> &jobs, const std::vector<RecHit> &hits, const std::vector<int> &slot, int n_res, const std::string &names,
                  const std::string &tnames, const std::vector<uint64_t> &tname_off, const uint32_t *dS, const std::vector<uint32_t> &cig, mm2amd_txt_res_t *res, char *pool,
                  size_t pool_cap)
{
	const int n_jobs = (int)jobs.size();
	for (int i = 0; i < n_res; ++i) res[i].off = 0, res[i].len = 0, res[i].status = 0;
	if (n_jobs == 0) return 0;
	DevBuf<RecJob> d_jobs;
	DevBuf<RecHit> d_hits;
	DevBuf<char> d_names, d_tnames, d_out;
	DevBuf<uint64_t> d_tname_off, d_off;
	DevBuf<uint32_t> d_cig;
	DevBuf<RecRes> d_res;
	d_jobs.ensure(n_jobs), d_hits.ensure(n_jobs), d_names.ensure(names.size() + 1), d_tnames.ensure(tnames.size() + 1), d_tname_off.ensure(tname_off.size()), d_cig.ensure(cig.size() + 1);
	d_res.ensure(n_jobs), d_off.ensure(n_jobs);
	HIP_CHECK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)n_jobs * sizeof(RecJob), hipMemcpyHostToDevice, dc.stream));
	HIP_CHECK(hipMemcpyAsync(d_hits.p, hits.data(), (size_t)n_jobs * sizeof(RecHit), hipMemcpyHostToDevice, dc.stream));
	if (!names.empty()) HIP_CHECK(hipMemcpyAsync(d_names.p, names.data(), names.size(), hipMemcpyHostToDevice, dc.stream));
	if (!tnames.empty()) HIP_CHECK(hipMemcpyAsync(d_tnames.p, tnames.data(), tnames.size(), hipMemcpyHostToDevice, dc.stream));
	HIP_CHECK(hipMemcpyAsync(d_tname_off.p, tname_off.data(), tname_off.size() * 8, hipMemcpyHostToDevice, dc.stream));
	if (!cig.empty()) HIP_CHECK(hipMemcpyAsync(d_cig.p, cig.data(), cig.size() * 4, hipMemcpyHostToDevice, dc.stream));
	RecParams P{};
	P.jobs = d_jobs.p, P.n_jobs = n_jobs, P.hits = d_hits.p, P.flag = 0, P.names = d_names.p, P.qpool = nullptr, P.S = dS, P.cigar = d_cig.p;
	P.tnames = d_tnames.p, P.tname_off = d_tname_off.p, P.tlen = nullptr, P.res = d_res.p;
	KernelProfiler &prof = kernel_profiler(0);
	std::vector<RecRes> hr(n_jobs);
	text_size_pass(P, junc_text_launch, hr.data(), prof, "junc_text_kernel[size]", (double)cig.size() * 4.0, (double)n_jobs, dc.stream, stream_sync);
	std::vector<uint64_t> off(n_jobs);
	uint64_t total = 0;
	for (int k = 0, i = 0; i < n_res; ++i) {
		res[i].off = total;
		if (k < n_jobs && slot[k] == i) {
			off[k] = total, res[i].len = hr[k].len, res[i].status = hr[k].status == kRecOk ? 0 : -1;
			total += hr[k].len, ++k;
		}
	}
	if (pool && total > pool_cap) { prof.collect(); return capi_fail(MM2AMD_ENOMEM, "[mm2amd] junction text: pool too small (a call with pool == NULL gives the lengths)"); }
	if (pool && total)
		text_write_pass(P, junc_text_launch, off.data(), d_off.p, d_out.ensure(total, 1.0), pool, total, prof, "junc_text_kernel[write]", (double)total + (double)cig.size() * 4.0, (double)n_jobs, dc.stream, stream_sync);
	prof.collect();
	return 0;
}

} // namespace mm2amd

extern "C" {

int mm2amd_device_count(void)
{
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess) return capi_fail(MM2AMD_ENODEV, std::string("[mm2amd] hipGetDeviceCount: ") + hipGetErrorString(e));
	return n;
}

static int ksw_batch(int mode, int8_t noncan, int n_jobs, const mm2amd_ksw_job_t *jobs, int8_t m, const int8_t *mat,
                     int8_t gapo, int8_t gape, int8_t gapo2, int8_t gape2,
                     mm2amd_ksw_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_cap)
{
	if (n_jobs < 0 || (n_jobs > 0 && (!jobs || !res)) || !mat || m != 5) return capi_fail(MM2AMD_EINVAL, "[mm2amd] ksw_extd2_batch: bad arguments (m must be 5)");
	if (n_jobs == 0) return 0;
	return guarded([&]() -> int {
		DeviceScope dev; DeviceCtx &dc = dev.dc;
		KernelApiState &d = kstate();
		d.ksw.n_cu = dc.n_cu;
		std::vector<KswJob> dj(n_jobs);
		size_t qtot = 0, ttot = 0;
		for (int i = 0; i < n_jobs; ++i) {
			const mm2amd_ksw_job_t &j = jobs[i];
			KswJob &o = dj[i];
			o.q_off = qtot, o.t_off = ttot, o.qlen = j.qlen, o.tlen = j.tlen, o.w = j.w, o.zdrop = j.zdrop, o.end_bonus = j.end_bonus;
			o.flag = j.flag & 0x1fff;
			o.tag = (uint32_t)i, o.reserved = 0;
			qtot += j.qlen > 0 ? j.qlen : 0, ttot += j.tlen > 0 ? j.tlen : 0;
		}
		std::vector<uint8_t> hq(qtot + 1), ht(ttot + 1);
		for (int i = 0; i < n_jobs; ++i) {
			if (jobs[i].qlen > 0) memcpy(&hq[dj[i].q_off], jobs[i].query, jobs[i].qlen);
			if (jobs[i].tlen > 0) memcpy(&ht[dj[i].t_off], jobs[i].target, jobs[i].tlen);
		}
		d.d_qpool.ensure(qtot + 1), d.d_tpool.ensure(ttot + 1);
		HIP_CHECK(hipMemcpyAsync(d.d_qpool.p, hq.data(), qtot + 1, hipMemcpyHostToDevice, dc.stream));
		HIP_CHECK(hipMemcpyAsync(d.d_tpool.p, ht.data(), ttot + 1, hipMemcpyHostToDevice, dc.stream));
		KswScoring sc;
		memcpy(sc.mat, mat, 25);
		sc.m = m, sc.q = gapo, sc.e = gape, sc.q2 = gapo2, sc.e2 = gape2, sc.single = (int8_t)mode, sc.noncan = noncan;
		std::vector<KswRes> r(n_jobs);
		const uint32_t *cig = nullptr;
		size_t n_cig = 0;
		d.ksw.prof = &kernel_profiler(0);
		d.ksw.disable_fast = getenv("MM2AMD_KSW_EXACT_ONLY") != nullptr;
		d.ksw.run(dj, d.d_qpool.p, d.d_tpool.p, nullptr, sc, r.data(), &cig, &n_cig, dc.stream);
		kernel_profiler().collect();
		if (n_cig > cigar_pool_cap) return capi_fail(MM2AMD_ENOMEM, "[mm2amd] ksw_extd2_batch: cigar_pool too small (sum(qlen+tlen) always suffices)");
		if (n_cig) memcpy(cigar_pool, cig, n_cig * sizeof(uint32_t));
		for (int i = 0; i < n_jobs; ++i) {
			mm2amd_ksw_res_t &o = res[i];
			o.max = r[i].max, o.zdropped = r[i].zdropped, o.max_q = r[i].max_q, o.max_t = r[i].max_t;
			o.mqe = r[i].mqe, o.mqe_t = r[i].mqe_t, o.mte = r[i].mte, o.mte_q = r[i].mte_q;
			o.score = r[i].score, o.n_cigar = r[i].n_cigar, o.reach_end = r[i].reach_end, o.cigar_off = r[i].cigar_off;
		}
		return 0;
	});
}

int mm2amd_ksw_extd2_batch(int n_jobs, const mm2amd_ksw_job_t *jobs, int8_t m, const int8_t *mat,
                           int8_t gapo, int8_t gape, int8_t gapo2, int8_t gape2,
                           mm2amd_ksw_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_cap)
{
	return ksw_batch(0, 0, n_jobs, jobs, m, mat, gapo, gape, gapo2, gape2, res, cigar_pool, cigar_pool_cap);
}

int mm2amd_ksw_extz2_batch(int n_jobs, const mm2amd_ksw_job_t *jobs, int8_t m, const int8_t *mat, int8_t gapo, int8_t gape,
                           mm2amd_ksw_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_cap)
{
	return ksw_batch(1, 0, n_jobs, jobs, m, mat, gapo, gape, gapo, gape, res, cigar_pool, cigar_pool_cap);
}

int mm2amd_ksw_exts2_batch(int n_jobs, const mm2amd_ksw_job_t *jobs, int8_t m, const int8_t *mat, int8_t gapo, int8_t gape, int8_t gapo2, int8_t noncan,
                           mm2amd_ksw_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_cap)
{
	return ksw_batch(2, noncan, n_jobs, jobs, m, mat, gapo, gape, gapo2, 0, res, cigar_pool, cigar_pool_cap);
}

// mm2amd_update_extra_batch, and with eqx mm2amd_update_extra_eqx_batch: cigar_eqx_kernel on top, its pool sized by a first call without one
static int update_extra_impl(bool eqx, int n_jobs, const mm2amd_fin_job_t *jobs, const int8_t *mat25, int8_t q, int8_t e, int log_gap,
                             mm2amd_fin_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_cap)
{
	if (n_jobs < 0 || (n_jobs > 0 && (!jobs || !res)) || !mat25) return capi_fail(MM2AMD_EINVAL, "[mm2amd] update_extra_batch: bad arguments");
	if (n_jobs == 0) return 0;
	return guarded([&]() -> int {
		DeviceScope dev; DeviceCtx &dc = dev.dc;
		std::vector<FinRegion> regs(n_jobs);
		std::vector<FinPiece> pieces;
		std::vector<uint32_t> cig;
		size_t qtot = 0, ttot = 0, out_words = 0;
		uint32_t longest = 1;
		for (int i = 0; i < n_jobs; ++i) {
			const mm2amd_fin_job_t &j = jobs[i];
			if (j.qlen < 0 || j.tlen < 0 || j.n_pieces < 0 || (j.n_pieces > 0 && (!j.piece || !j.piece_len))) return capi_fail(MM2AMD_EINVAL, "[mm2amd] update_extra_batch: bad job");
			FinRegion &r = regs[i];
			r.q_pos = qtot, r.t_pos = ttot, r.piece0 = (uint32_t)pieces.size(), r.n_pieces = (uint32_t)j.n_pieces, r.out_off = (uint32_t)out_words;
			r.q_len = j.qlen, r.t_len = j.tlen;
			uint32_t sum = 0;
			for (int k = 0; k < j.n_pieces; ++k) {
				if (j.piece_len[k] < 0) return capi_fail(MM2AMD_EINVAL, "[mm2amd] update_extra_batch: negative piece length");
				pieces.push_back(FinPiece{ (uint32_t)cig.size(), (uint32_t)j.piece_len[k] });
				cig.insert(cig.end(), j.piece[k], j.piece[k] + j.piece_len[k]);
				sum += (uint32_t)j.piece_len[k];
			}
			if (sum > (uint32_t)kFinMaxOps) return capi_fail(MM2AMD_EINVAL, "[mm2amd] update_extra_batch: a region has more CIGAR operations than the kernel stages in LDS");
			longest = std::max(longest, sum);
			out_words += sum;
			qtot += ((size_t)j.qlen + 15) & ~(size_t)7, ttot += ((size_t)j.tlen + 15) & ~(size_t)7; // (the kernel reads aligned 8-byte / 8-code blocks)
		}
		if (!eqx && out_words > cigar_pool_cap) return capi_fail(MM2AMD_ENOMEM, "[mm2amd] update_extra_batch: cigar_pool too small (the sum of the piece lengths suffices)");
		std::vector<uint8_t> hq(qtot + 16, 0);
		std::vector<uint32_t> hS(ttot / 8 + 4, 0);
		for (int i = 0; i < n_jobs; ++i) {
			const mm2amd_fin_job_t &j = jobs[i];
			if (j.qlen) memcpy(&hq[regs[i].q_pos], j.query, (size_t)j.qlen);
			for (int32_t t = 0; t < j.tlen; ++t) { const uint64_t o = regs[i].t_pos + (uint64_t)t; hS[o >> 3] |= (uint32_t)(j.target[t] & 0xf) << ((o & 7) << 2); }
		}
		DevBuf<uint8_t> d_q;
		DevBuf<uint32_t> d_S, d_cig, d_out;
		DevBuf<FinRegion> d_regs;
		DevBuf<FinPiece> d_pieces;
		DevBuf<FinResult> d_res;
		d_q.ensure(hq.size()), d_S.ensure(hS.size()), d_cig.ensure(cig.size() + 1), d_out.ensure(out_words + 1), d_regs.ensure(n_jobs), d_pieces.ensure(pieces.size() + 1), d_res.ensure(n_jobs);
		HIP_CHECK(hipMemcpyAsync(d_q.p, hq.data(), hq.size(), hipMemcpyHostToDevice, dc.stream));
		HIP_CHECK(hipMemcpyAsync(d_S.p, hS.data(), hS.size() * 4, hipMemcpyHostToDevice, dc.stream));
		if (!cig.empty()) HIP_CHECK(hipMemcpyAsync(d_cig.p, cig.data(), cig.size() * 4, hipMemcpyHostToDevice, dc.stream));
		HIP_CHECK(hipMemcpyAsync(d_regs.p, regs.data(), (size_t)n_jobs * sizeof(FinRegion), hipMemcpyHostToDevice, dc.stream));
		if (!pieces.empty()) HIP_CHECK(hipMemcpyAsync(d_pieces.p, pieces.data(), pieces.size() * sizeof(FinPiece), hipMemcpyHostToDevice, dc.stream));
		finish_run(d_regs.p, n_jobs, d_pieces.p, d_cig.p, d_out.p, d_res.p, d_q.p, d_S.p, mat25, q, e, log_gap != 0, longest, dc.stream, nullptr, 0.0, 0.0); // (no profile entry)
		std::vector<FinResult> hr(n_jobs);
		const auto put = [&](int i, int32_t n_cigar, uint32_t off) { // the public record from the kernel's
			const FinResult &f = hr[i];
			mm2amd_fin_res_t &o = res[i];
			o.n_cigar = n_cigar, o.blen = f.blen, o.mlen = f.mlen, o.n_ambi = f.n_ambi, o.dp_max = f.dp_max, o.qshift = f.qshift, o.tshift = f.tshift, o.is_spliced = f.is_spliced, o.cigar_off = off;
		};
		if (eqx) { // count, place, write (cigar_eqx.hpp); cigar_pool null: the counts alone
			EqxBufs B;
			EqxParams X{};
			X.regions = d_regs.p, X.n_regions = n_jobs, X.results = d_res.p, X.fin_pool = d_out.p, X.qpool = d_q.p, X.S = d_S.p;
			KernelProfiler &prof = kernel_profiler();
			HIP_CHECK(hipMemcpyAsync(hr.data(), d_res.p, (size_t)n_jobs * sizeof(FinResult), hipMemcpyDeviceToHost, dc.stream));
			const uint64_t total = eqx_count(B, X, prof, (double)out_words * 4.0 + (double)qtot + (double)ttot / 2 + (double)n_jobs * (sizeof(FinRegion) + sizeof(FinResult) + 4), dc.stream, stream_sync);
			for (int i = 0; i < n_jobs; ++i) put(i, hr[i].n_cigar < 0 ? hr[i].n_cigar : (int32_t)B.h_n.p[i], (uint32_t)B.h_off.p[i]);
			if (total >= (1ull << 32)) { prof.collect(); return capi_fail(MM2AMD_EINVAL, "[mm2amd] update_extra_eqx_batch: the batch's =/X CIGARs exceed 32-bit offsets"); }
			if (!cigar_pool) { prof.collect(); return 0; }
			if (total > cigar_pool_cap) { prof.collect(); return capi_fail(MM2AMD_ENOMEM, "[mm2amd] update_extra_eqx_batch: cigar_pool too small (a call with cigar_pool == NULL gives every res[i].n_cigar)"); }
			const EqxOut x = eqx_write(B, X, total, prof, ((double)out_words + (double)total) * 4.0 + 2.0 * ((double)qtot + (double)ttot / 2) + (double)n_jobs * (sizeof(FinRegion) + sizeof(FinResult) + 12), dc.stream);
			stream_sync(dc.stream);
			prof.collect();
			if (total) memcpy(cigar_pool, x.cigars, total * 4);
			return 0;
		}
		std::vector<uint32_t> ho(out_words + 1);
		HIP_CHECK(hipMemcpyAsync(hr.data(), d_res.p, (size_t)n_jobs * sizeof(FinResult), hipMemcpyDeviceToHost, dc.stream));
		if (out_words) HIP_CHECK(hipMemcpyAsync(ho.data(), d_out.p, out_words * 4, hipMemcpyDeviceToHost, dc.stream));
		HIP_CHECK(hipStreamSynchronize(dc.stream));
		for (int i = 0; i < n_jobs; ++i) put(i, hr[i].n_cigar, regs[i].out_off);
		if (out_words) memcpy(cigar_pool, ho.data(), out_words * 4);
		return 0;
	});
}

int mm2amd_update_extra_batch(int n_jobs, const mm2amd_fin_job_t *jobs, const int8_t *mat25, int8_t q, int8_t e, int log_gap,
                              mm2amd_fin_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_cap)
{
	return update_extra_impl(false, n_jobs, jobs, mat25, q, e, log_gap, res, cigar_pool, cigar_pool_cap);
}

int mm2amd_update_extra_eqx_batch(int n_jobs, const mm2amd_fin_job_t *jobs, const int8_t *mat25, int8_t q, int8_t e, int log_gap,
                                  mm2amd_fin_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_cap)
{
	return update_extra_impl(true, n_jobs, jobs, mat25, q, e, log_gap, res, cigar_pool, cigar_pool_cap);
}

int mm2amd_aln_text_batch(int n_jobs, const mm2amd_txt_job_t *jobs, int what, mm2amd_txt_res_t *res, char *pool, size_t pool_cap)
{
	if (n_jobs < 0 || (n_jobs > 0 && (!jobs || !res)) || what < MM2AMD_TXT_CIGAR || what > MM2AMD_TXT_DS_LONG) return capi_fail(MM2AMD_EINVAL, "[mm2amd] aln_text_batch: bad arguments");
	if (n_jobs == 0) return 0;
	return guarded([&]() -> int {
		const bool seqs = what != MM2AMD_TXT_CIGAR;
		std::vector<TxtJob> tj(n_jobs);
		size_t qtot = 0, ttot = 0, ctot = 0;
		for (int i = 0; i < n_jobs; ++i) {
			const mm2amd_txt_job_t &j = jobs[i];
			if (j.n_cigar < 0 || (j.n_cigar > 0 && !j.cigar)) return capi_fail(MM2AMD_EINVAL, "[mm2amd] aln_text_batch: bad job");
			if (seqs && (j.qlen < 0 || j.tlen < 0 || (j.qlen > 0 && !j.query) || (j.tlen > 0 && !j.target))) return capi_fail(MM2AMD_EINVAL, "[mm2amd] aln_text_batch: bad job");
			TxtJob &o = tj[i];
			o.q_pos = qtot, o.t_pos = ttot, o.cig_off = ctot, o.n_cigar = (uint32_t)j.n_cigar, o.qlen = seqs ? j.qlen : 0, o.tlen = seqs ? j.tlen : 0;
			o.qsrc = (uint8_t)kTxtQCodes, o.tsrc = (uint8_t)kTxtTCodes, o.reserved = 0;
			ctot += (size_t)j.n_cigar;
			if (seqs) qtot += (size_t)j.qlen, ttot += (size_t)j.tlen;
		}
		std::vector<uint8_t> hq(qtot), ht(ttot);
		std::vector<uint32_t> cig(ctot);
		for (int i = 0; i < n_jobs; ++i) {
			const mm2amd_txt_job_t &j = jobs[i];
			if (j.n_cigar) memcpy(&cig[tj[i].cig_off], j.cigar, (size_t)j.n_cigar * 4);
			if (seqs && j.qlen) memcpy(&hq[tj[i].q_pos], j.query, (size_t)j.qlen);
			if (seqs && j.tlen) memcpy(&ht[tj[i].t_pos], j.target, (size_t)j.tlen);
		}
		DeviceScope dev;
		return aln_text_run(dev.dc, tj, what, hq, ht, nullptr, cig, res, pool, pool_cap);
	});
}

int mm2amd_ksw_ll_limits(int *strip_cols, int *wg_waves, int64_t *wg_min_cells, int *max_len)
{
	if (strip_cols) *strip_cols = kLlStrip;
	if (wg_waves) *wg_waves = kLlWgWaves;
	if (wg_min_cells) *wg_min_cells = ll_wg_min_cells();
	if (max_len) *max_len = kLlMaxLen;
	return 0;
}

int mm2amd_ksw_ll_batch(int n_jobs, const mm2amd_ll_job_t *jobs, int8_t m, const int8_t *mat, int gapo, int gape, mm2amd_ll_res_t *res)
{
	if (n_jobs < 0 || (n_jobs > 0 && (!jobs || !res)) || !mat || m != 5) return capi_fail(MM2AMD_EINVAL, "[mm2amd] ksw_ll_batch: bad arguments (m must be 5)");
	if (n_jobs == 0) return 0;
	for (int i = 0; i < n_jobs; ++i) {
		const mm2amd_ll_job_t &j = jobs[i];
		if (j.qlen < 0 || j.tlen < 0 || (j.qlen > 0 && !j.query) || (j.tlen > 0 && !j.target)) return capi_fail(MM2AMD_EINVAL, "[mm2amd] ksw_ll_batch: bad job (negative length or null sequence)");
		uint8_t top = 0;
		for (int32_t k = 0; k < j.qlen; ++k) top |= (uint8_t)(j.query[k] > 4);
		for (int32_t k = 0; k < j.tlen; ++k) top |= (uint8_t)(j.target[k] > 4);
		if (top) return capi_fail(MM2AMD_EINVAL, "[mm2amd] ksw_ll_batch: a sequence holds a code above 4");
	}
	return guarded([&]() -> int {
		DeviceScope dev; DeviceCtx &dc = dev.dc;
		LlApiState &d = ll_state();
		const bool no_wg = ll_no_wg();
		const int64_t wg_min = ll_wg_min_cells();
		// routing: HOST, or one of the two launch classes; each class longest job first, so that a launch's tail is short
		std::vector<int> cls[2], host;
		for (int i = 0; i < n_jobs; ++i) {
			const mm2amd_ll_job_t &j = jobs[i];
			const int64_t cells = (int64_t)j.qlen * j.tlen;
			if (cells == 0 || j.qlen > kLlMaxLen || j.tlen > kLlMaxLen || !ll_plain_class(j.qlen, j.tlen, mat, gapo, gape)) host.push_back(i), res[i].path = MM2AMD_LL_PATH_HOST;
			else if (!no_wg && j.qlen > kLlStrip && cells >= wg_min) cls[1].push_back(i), res[i].path = MM2AMD_LL_PATH_WG;
			else cls[0].push_back(i), res[i].path = MM2AMD_LL_PATH_WAVE;
		}
		std::vector<LlJob> dj;
		struct Launch { size_t first; int n, waves; double cells; };
		std::vector<Launch> launches;
		size_t qtot = 0, ttot = 0, bnd_max = 1;
		for (int c = 0; c < 2; ++c) {
			std::vector<int> &v = cls[c];
			std::stable_sort(v.begin(), v.end(), [&](int a, int b) { return (int64_t)jobs[a].qlen * jobs[a].tlen > (int64_t)jobs[b].qlen * jobs[b].tlen; });
			const int waves = c ? kLlWgWaves : 1;
			size_t bnd = 0;
			Launch cur{ dj.size(), 0, waves, 0.0 };
			for (int i : v) {
				const mm2amd_ll_job_t &j = jobs[i];
				const size_t need = j.qlen > kLlStrip ? (size_t)waves * ll_bnd_words(j.tlen) : 0;
				if (cur.n > 0 && bnd + need > kLlBndBudget) { launches.push_back(cur); cur = Launch{ dj.size(), 0, waves, 0.0 }; bnd = 0; }
				LlJob o;
				o.q_off = qtot, o.t_off = ttot, o.bnd_off = bnd, o.qlen = j.qlen, o.tlen = j.tlen, o.flag = (uint32_t)j.flag & 7u, o.out = (uint32_t)i;
				dj.push_back(o);
				qtot += (size_t)j.qlen, ttot += (size_t)j.tlen, bnd += need;
				bnd_max = std::max(bnd_max, bnd);
				++cur.n, cur.cells += (double)j.qlen * j.tlen;
			}
			if (cur.n > 0) launches.push_back(cur);
		}
		if (!dj.empty()) {
			uint8_t *const hq = d.h_q.ensure(qtot + 1), *const ht = d.h_t.ensure(ttot + 1);
			LlJob *const hj = d.h_jobs.ensure(dj.size());
			d.h_res.ensure((size_t)n_jobs);
			for (size_t k = 0; k < dj.size(); ++k) {
				const LlJob &o = dj[k];
				memcpy(hq + o.q_off, jobs[o.out].query, (size_t)o.qlen);
				memcpy(ht + o.t_off, jobs[o.out].target, (size_t)o.tlen);
				hj[k] = o;
			}
			d.d_q.ensure(qtot + 1), d.d_t.ensure(ttot + 1), d.d_jobs.ensure(dj.size()), d.d_res.ensure((size_t)n_jobs), d.d_bnd.ensure(bnd_max);
			HIP_CHECK(hipMemcpyAsync(d.d_q.p, hq, qtot + 1, hipMemcpyHostToDevice, dc.stream));
			HIP_CHECK(hipMemcpyAsync(d.d_t.p, ht, ttot + 1, hipMemcpyHostToDevice, dc.stream));
			HIP_CHECK(hipMemcpyAsync(d.d_jobs.p, hj, dj.size() * sizeof(LlJob), hipMemcpyHostToDevice, dc.stream));
			LlParams P;
			P.qpool = d.d_q.p, P.tpool = d.d_t.p, P.bnd = d.d_bnd.p, P.res = d.d_res.p, P.goe = gapo + gape, P.ge = gape;
			for (int qc = 0; qc < 5; ++qc) { // ksw_ll_qinit's profile: target code a against query code qc scores mat[a * m + qc] (ksw2_ll_sse.c:63-71)
				P.sc_lo[qc] = 0;
				for (int a = 0; a < 4; ++a) P.sc_lo[qc] |= (uint32_t)(uint8_t)mat[a * 5 + qc] << (8 * a);
				P.sc_hi[qc] = mat[20 + qc];
			}
			KernelProfiler &prof = kernel_profiler(0);
			for (const Launch &l : launches) {
				P.jobs = d.d_jobs.p + l.first, P.n_jobs = l.n, P.n_waves = l.waves;
				prof.begin(dc.stream);
				ksw_ll_launch(P, dc.stream);
				prof.end(dc.stream, l.waves == 1 ? "ksw_ll_kernel[wave]" : "ksw_ll_kernel[wg]", 0.0, l.cells);
			}
		}
		// the host's share while the device works: the sequences as the flags say, then the scalar routine
		std::vector<uint8_t> hq1, ht1;
		for (int i : host) {
			const mm2amd_ll_job_t &j = jobs[i];
			if (j.qlen == 0 || j.tlen == 0) { res[i].score = 0, res[i].qe = res[i].te = -1; continue; } // (nothing to align: the contract's answer)
			hq1.assign(j.query, j.query + j.qlen), ht1.assign(j.target, j.target + j.tlen);
			if (j.flag & MM2AMD_LL_QREV) std::reverse(hq1.begin(), hq1.end());
			if (j.flag & MM2AMD_LL_QCOMP) for (uint8_t &c : hq1) c = c < 4 ? 3 - c : 4;
			if (j.flag & MM2AMD_LL_TREV) std::reverse(ht1.begin(), ht1.end());
			int qe = -1, te = -1;
			res[i].score = ll_local_score(j.qlen, hq1.data(), j.tlen, ht1.data(), mat, gapo, gape, &qe, &te);
			res[i].qe = qe, res[i].te = te;
		}
		if (!dj.empty()) {
			const LlRes *const hr = d.h_res.p;
			HIP_CHECK(hipMemcpyAsync(d.h_res.p, d.d_res.p, (size_t)n_jobs * sizeof(LlRes), hipMemcpyDeviceToHost, dc.stream));
			HIP_CHECK(hipStreamSynchronize(dc.stream));
			kernel_profiler(0).collect();
			for (const LlJob &o : dj) res[o.out].score = hr[o.out].score, res[o.out].qe = hr[o.out].qe, res[o.out].te = hr[o.out].te;
		}
		return 0;
	});
}

int mm2amd_sdust_limits(int *narrow_cap, int *wide_cap, int *max_len)
{
	if (narrow_cap) *narrow_cap = sdust_env_narrow_cap();
	if (wide_cap) *wide_cap = kSdustWideCap;
	if (max_len) *max_len = kSdustMaxLen;
	return 0;
}

int mm2amd_sdust_batch(int n_jobs, const mm2amd_sdust_job_t *jobs, int T, mm2amd_sdust_res_t *res, uint64_t *pool, size_t pool_cap)
{
	if (const int rc = sdust_check_args("sdust_batch", n_jobs, jobs, T, res)) return rc;
	if (n_jobs == 0) return 0;
	return guarded([&]() -> int {
		DeviceScope dev; DeviceCtx &dc = dev.dc;
		SdustApiState &d = sdust_state();
		const size_t n = (size_t)n_jobs;
		uint64_t *const h_off = d.h_off.ensure(2 * (n + 1)); // the jobs' base offsets, then their offsets in the pool
		h_off[0] = 0;
		for (size_t i = 0; i < n; ++i) h_off[i + 1] = h_off[i] + (uint64_t)jobs[i].len;
		const uint64_t total = h_off[n];
		uint8_t *const h_codes = d.h_codes.ensure(total + 1);
		for (size_t i = 0; i < n; ++i) for (int32_t k = 0; k < jobs[i].len; ++k) h_codes[h_off[i] + k] = kNt4Table[(uint8_t)jobs[i].seq[k]];
		d.d_codes.ensure(total + 1), d.d_off.ensure(n + 1), d.d_out_off.ensure(n + 1), d.d_reg_n.ensure(total + 1), d.d_reg_s.ensure(total + 1), d.d_reg_e.ensure(total + 1);
		d.d_list.ensure(n), d.d_cnt_out.ensure(n), d.d_cnt.ensure(1);
		HIP_CHECK(hipMemcpyAsync(d.d_codes.p, h_codes, total + 1, hipMemcpyHostToDevice, dc.stream));
		HIP_CHECK(hipMemcpyAsync(d.d_off.p, h_off, (n + 1) * 8, hipMemcpyHostToDevice, dc.stream));
		HIP_CHECK(hipMemsetAsync(d.d_cnt.p, 0, sizeof(SdustCounters), dc.stream));
		SdustParams P;
		P.codes = d.d_codes.p, P.off = d.d_off.p, P.code_mul = 1, P.n_reads = n_jobs, P.T = T < kSdustMaxT ? T : kSdustMaxT;
		P.reg_n = d.d_reg_n.p, P.reg_s = d.d_reg_s.p, P.reg_e = d.d_reg_e.p, P.wide_list = d.d_list.p, P.cnt = d.d_cnt.p;
		KernelProfiler &prof = kernel_profiler(0);
		SdustCounters hc;
		memset(&hc, 0, sizeof hc);
		uint32_t *const h_list = d.h_list.ensure(2 * n); // the listed jobs, then every job's number of regions
		for (size_t i = 0; i < n; ++i) res[i].path = MM2AMD_SDUST_PATH_NARROW;
		if (sdust_env_no_narrow()) {
			sdust_run_class(P, 2, 0, prof, (double)total, dc.stream);
			for (size_t i = 0; i < n; ++i) res[i].path = MM2AMD_SDUST_PATH_WIDE;
		} else {
			sdust_run_class(P, 0, 0, prof, 0.0, dc.stream);
			HIP_CHECK(hipMemcpyAsync(&hc, d.d_cnt.p, sizeof hc, hipMemcpyDeviceToHost, dc.stream));
			HIP_CHECK(hipStreamSynchronize(dc.stream));
			if (hc.n_wide > (uint32_t)n_jobs) return capi_fail(MM2AMD_EHIP, "[mm2amd] sdust_batch: the device's list of wide jobs is longer than the batch");
			double wide_bases = 0;
			if (hc.n_wide) { // the jobs that stopped, scanned again with the full list: a launch of exactly that many wavefronts
				HIP_CHECK(hipMemcpyAsync(h_list, d.d_list.p, (size_t)hc.n_wide * 4, hipMemcpyDeviceToHost, dc.stream));
				sdust_run_class(P, 1, (int)std::min<uint32_t>(hc.n_wide, (uint32_t)kSdustWideGrid), prof, 0.0, dc.stream);
				HIP_CHECK(hipStreamSynchronize(dc.stream));
				for (uint32_t k = 0; k < hc.n_wide; ++k) {
					if (h_list[k] >= (uint32_t)n_jobs) return capi_fail(MM2AMD_EHIP, "[mm2amd] sdust_batch: the device listed a job outside the batch");
					res[h_list[k]].path = MM2AMD_SDUST_PATH_WIDE, wide_bases += (double)jobs[h_list[k]].len;
				}
				prof.add_units("sdust_kernel[wide]", wide_bases);
			}
			prof.add_units("sdust_kernel[narrow]", (double)total - wide_bases + (double)hc.narrow_partial);
		}
		// every job's number of regions, the offsets they give, then the regions themselves
		sdust_count_launch(P, d.d_cnt_out.p, dc.stream);
		uint32_t *const h_n = h_list + n;
		HIP_CHECK(hipMemcpyAsync(h_n, d.d_cnt_out.p, n * 4, hipMemcpyDeviceToHost, dc.stream));
		HIP_CHECK(hipMemcpyAsync(&hc, d.d_cnt.p, sizeof hc, hipMemcpyDeviceToHost, dc.stream));
		HIP_CHECK(hipStreamSynchronize(dc.stream));
		prof.collect();
		if (hc.err) return capi_fail(MM2AMD_EHIP, "[mm2amd] sdust_batch: a list of perfect intervals outgrew the wide capacity");
		uint64_t *const out_off = h_off + n + 1;
		uint64_t n_out = 0;
		for (size_t i = 0; i < n; ++i) {
			if (h_n[i] > (uint32_t)jobs[i].len) return capi_fail(MM2AMD_EHIP, "[mm2amd] sdust_batch: more regions than bases");
			out_off[i] = n_out, res[i].off = n_out, res[i].n = h_n[i];
			n_out += h_n[i];
		}
		if (!pool || n_out == 0) return 0;
		if (n_out > pool_cap) return capi_fail(MM2AMD_ENOMEM, "[mm2amd] sdust_batch: pool too small (a call with pool == NULL gives the counts)");
		d.d_out.ensure(n_out);
		HIP_CHECK(hipMemcpyAsync(d.d_out_off.p, out_off, n * 8, hipMemcpyHostToDevice, dc.stream));
		sdust_pack_launch(P, d.d_out_off.p, d.d_out.p, dc.stream);
		HIP_CHECK(hipMemcpyAsync(pool, d.d_out.p, n_out * 8, hipMemcpyDeviceToHost, dc.stream));
		HIP_CHECK(hipStreamSynchronize(dc.stream));
		return 0;
	});
}

int mm2amd_sdust_host_batch(int n_jobs, const mm2amd_sdust_job_t *jobs, int T, int n_threads, mm2amd_sdust_res_t *res, uint64_t *pool, size_t pool_cap,
                            double *core_seconds)
{
	if (const int rc = sdust_check_args("sdust_host_batch", n_jobs, jobs, T, res)) return rc;
	if (core_seconds) *core_seconds = 0;
	if (n_jobs == 0) return 0;
	return guarded([&]() -> int {
		std::vector<std::vector<uint64_t>> regs((size_t)n_jobs);
		std::vector<double> busy((size_t)std::max(n_threads, 1), 0.0);
		parallel_for(n_threads, (long)n_jobs, [&](long i, int tid) {
			const double t0 = Trace::now();
			thread_local std::vector<SdustState::Perf> perf(SdustState::PCAP);
			std::vector<uint8_t> codes((size_t)jobs[i].len + 1);
			for (int32_t k = 0; k < jobs[i].len; ++k) codes[k] = kNt4Table[(uint8_t)jobs[i].seq[k]];
			SdustState S;
			S.P = perf.data();
			sdust_scan(codes.data(), jobs[i].len, T, S, [&](int s0, int e0) { regs[i].push_back((uint64_t)(uint32_t)s0 << 32 | (uint32_t)e0); });
			busy[tid] += Trace::now() - t0;
		}, 1);
		uint64_t n_out = 0;
		for (int i = 0; i < n_jobs; ++i) res[i].off = n_out, res[i].n = (uint32_t)regs[i].size(), res[i].path = -1, n_out += regs[i].size();
		if (core_seconds) for (double b : busy) *core_seconds += b;
		if (!pool || n_out == 0) return 0;
		if (n_out > pool_cap) return capi_fail(MM2AMD_ENOMEM, "[mm2amd] sdust_host_batch: pool too small (a call with pool == NULL gives the counts)");
		for (int i = 0; i < n_jobs; ++i) if (!regs[i].empty()) memcpy(pool + res[i].off, regs[i].data(), regs[i].size() * 8);
		return 0;
	});
}

int mm2amd_hits_merge_limits(int *narrow_cap, int *wide_cap, int *max_hits)
{
	if (narrow_cap) *narrow_cap = kHmNarrowCap;
	if (wide_cap) *wide_cap = kHmWideCap;
	if (max_hits) *max_hits = kHmMaxHits;
	return 0;
}

int mm2amd_hits_merge_batch(int n_seg, const uint64_t *seg_off, const mm2amd_hm_hit_t *hits, const mm2amd_hm_opt_t *opt, mm2amd_hm_out_t *out,
                            mm2amd_hm_seg_t *seg)
{
	if (const int rc = hm_check_args("hits_merge_batch", n_seg, seg_off, hits, opt, out, seg)) return rc;
	if (n_seg == 0) return 0;
	return guarded([&]() -> int {
		DeviceScope dev; DeviceCtx &dc = dev.dc;
		HitsMergeApiState &d = hm_state();
		const size_t n = (size_t)n_seg;
		const uint64_t first = seg_off[0], total = seg_off[n] - first;
		// the segments by class: narrow ones from the front of the list, wide ones from its end; the rest is the host's
		uint32_t *const h_list = d.h_list.ensure(n);
		size_t n_narrow = 0, n_wide = 0;
		double narrow_hits = 0, wide_hits = 0;
		for (size_t s = 0; s < n; ++s) {
			const uint64_t m = seg_off[s + 1] - seg_off[s];
			seg[s].n_kept = -1, seg[s].path = MM2AMD_HM_PATH_HOST;
			if (m <= (uint64_t)kHmNarrowCap) h_list[n_narrow++] = (uint32_t)s, narrow_hits += (double)m;
			else if (m <= (uint64_t)kHmWideCap) h_list[n - 1 - n_wide++] = (uint32_t)s, wide_hits += (double)m;
		}
		if (n_narrow + n_wide > 0) {
			d.d_hits.ensure(total + 1), d.d_out.ensure(total + 1), d.d_seg.ensure(n), d.d_off.ensure(n + 1), d.d_list.ensure(n);
			if (total) HIP_CHECK(hipMemcpyAsync(d.d_hits.p, hits + first, total * sizeof(mm2amd_hm_hit_t), hipMemcpyHostToDevice, dc.stream));
			HIP_CHECK(hipMemcpyAsync(d.d_off.p, seg_off, (n + 1) * 8, hipMemcpyHostToDevice, dc.stream));
			HIP_CHECK(hipMemcpyAsync(d.d_list.p, h_list, n * 4, hipMemcpyHostToDevice, dc.stream));
			HIP_CHECK(hipMemcpyAsync(d.d_seg.p, seg, n * sizeof(mm2amd_hm_seg_t), hipMemcpyHostToDevice, dc.stream));
			HitsMergeParams P;
			P.hits = d.d_hits.p, P.seg_off = d.d_off.p, P.first = first, P.out = d.d_out.p, P.seg = d.d_seg.p, P.opt = *opt;
			KernelProfiler &prof = kernel_profiler(0);
			if (n_narrow) {
				P.list = d.d_list.p, P.n_list = (int)n_narrow, P.cap = kHmNarrowCap, P.path = MM2AMD_HM_PATH_NARROW;
				prof.begin(dc.stream);
				hits_merge_launch(P, dc.stream);
				prof.end(dc.stream, "hits_merge_kernel[narrow]", 0.0, narrow_hits);
			}
			if (n_wide) {
				P.list = d.d_list.p + (n - n_wide), P.n_list = (int)n_wide, P.cap = kHmWideCap, P.path = MM2AMD_HM_PATH_WIDE;
				prof.begin(dc.stream);
				hits_merge_launch(P, dc.stream);
				prof.end(dc.stream, "hits_merge_kernel[wide]", 0.0, wide_hits);
			}
			HIP_CHECK(hipMemcpyAsync(seg, d.d_seg.p, n * sizeof(mm2amd_hm_seg_t), hipMemcpyDeviceToHost, dc.stream));
			if (total) HIP_CHECK(hipMemcpyAsync(out + first, d.d_out.p, total * sizeof(mm2amd_hm_out_t), hipMemcpyDeviceToHost, dc.stream));
			HIP_CHECK(hipStreamSynchronize(dc.stream));
			prof.collect();
		}
		// the host class: by size, or because the kernel met equal keys among more than 64 live hits -- the longest lists of the batch, on the pool's threads
		std::vector<uint32_t> host_list;
		for (size_t s = 0; s < n; ++s) {
			if (seg[s].path == MM2AMD_HM_PATH_HOST) { host_list.push_back((uint32_t)s); continue; }
			if (seg[s].n_kept < 0 || (uint64_t)seg[s].n_kept > seg_off[s + 1] - seg_off[s]) return capi_fail(MM2AMD_EHIP, "[mm2amd] hits_merge_batch: the device kept more hits than the segment has");
		}
		parallel_for(effective_cpus(), (long)host_list.size(), [&](long k, int) {
			const uint32_t s = host_list[(size_t)k];
			hm_host_segment(hits + seg_off[s], (int)(seg_off[s + 1] - seg_off[s]), *opt, out + seg_off[s], seg + s);
		}, 1);
		return 0;
	});
}

int mm2amd_hits_merge_host_batch(int n_seg, const uint64_t *seg_off, const mm2amd_hm_hit_t *hits, const mm2amd_hm_opt_t *opt, int n_threads,
                                 mm2amd_hm_out_t *out, mm2amd_hm_seg_t *seg, double *core_seconds)
{
	if (const int rc = hm_check_args("hits_merge_host_batch", n_seg, seg_off, hits, opt, out, seg)) return rc;
	if (core_seconds) *core_seconds = 0;
	if (n_seg == 0) return 0;
	return guarded([&]() -> int {
		std::vector<double> busy((size_t)std::max(n_threads, 1), 0.0);
		parallel_for(n_threads, (long)n_seg, [&](long s, int tid) {
			const double t0 = Trace::now();
			hm_host_segment(hits + seg_off[s], (int)(seg_off[s + 1] - seg_off[s]), *opt, out + seg_off[s], seg + s);
			busy[tid] += Trace::now() - t0;
		}, 16);
		if (core_seconds) for (double b : busy) *core_seconds += b;
		return 0;
	});
}

int mm2amd_pair_limits(int *narrow_cap, int *wide_cap, int *max_hits)
{
	if (narrow_cap) *narrow_cap = kPeNarrowCap;
	if (wide_cap) *wide_cap = kPeWideCap;
	if (max_hits) *max_hits = kPeMaxHits;
	return 0;
}

int mm2amd_pair_batch(int n_frag, const mm2amd_pe_frag_t *frag, const mm2amd_pe_hit_t *hits, const mm2amd_pe_opt_t *opt, mm2amd_pe_out_t *out,
                      mm2amd_pe_res_t *res)
{
	std::vector<uint32_t> order;
	if (const int rc = pe_check_args("pair_batch", n_frag, frag, hits, opt, out, res, order)) return rc;
	if (n_frag == 0) return 0;
	return guarded([&]() -> int {
		DeviceScope dev; DeviceCtx &dc = dev.dc;
		pair_run(pe_state().bufs, n_frag, frag, hits, *opt, out, res, effective_cpus(), kernel_profiler(0), dc.stream, stream_sync);
		return 0;
	});
}

int mm2amd_pair_host_batch(int n_frag, const mm2amd_pe_frag_t *frag, const mm2amd_pe_hit_t *hits, const mm2amd_pe_opt_t *opt, int n_threads,
                           mm2amd_pe_out_t *out, mm2amd_pe_res_t *res, double *core_seconds)
{
	std::vector<uint32_t> order;
	if (const int rc = pe_check_args("pair_host_batch", n_frag, frag, hits, opt, out, res, order)) return rc;
	if (core_seconds) *core_seconds = 0;
	if (n_frag == 0) return 0;
	return guarded([&]() -> int {
		std::vector<double> busy((size_t)std::max(n_threads, 1), 0.0);
		parallel_for(n_threads, (long)n_frag, [&](long f, int tid) {
			const double t0 = Trace::now();
			pe_host_fragment(frag[f], hits + frag[f].hit0, *opt, out + frag[f].hit0, res + f, MM2AMD_PE_PATH_HOST);
			busy[tid] += Trace::now() - t0;
		}, 64);
		if (core_seconds) for (double b : busy) *core_seconds += b;
		return 0;
	});
}

void *mm2amd_split_open(const char *prefix, const mm2amd_index_t *idx, int part_no)
{
	void *h = nullptr;
	if (!prefix || !idx || part_no < 0 || part_no > 9999) { capi_fail(MM2AMD_EINVAL, "[mm2amd] split_open: bad arguments"); return nullptr; }
	guarded([&]() -> int { h = split_open(prefix, index_flat((const IndexHandle *)idx), part_no); return 0; });
	return h;
}

int mm2amd_split_write(void *w, const void *opt, int n_seq, const int *n_reg, void *const *reg, const int *rep_len, const int *frag_gap)
{
	if (!w || !opt || n_seq < 0 || (n_seq > 0 && (!n_reg || !reg || !rep_len || !frag_gap))) return capi_fail(MM2AMD_EINVAL, "[mm2amd] split_write: bad arguments");
	return guarded([&]() -> int {
		SplitWriter &sw = *(SplitWriter *)w;
		sw.cigar = (((const ref::MapOpt *)opt)->flag & ref::F_CIGAR) != 0;
		split_write(sw, n_seq, n_reg, reg, rep_len, frag_gap);
		return 0;
	});
}

int mm2amd_split_close(void *w)
{
	SplitWriter *sw = (SplitWriter *)w;
	if (!sw) return 0;
	const bool ok = !sw->fp || fclose(sw->fp) == 0;
	sw->fp = nullptr;
	const std::string fn = sw->fn;
	delete sw;
	return ok ? 0 : capi_fail(MM2AMD_EIO, "[mm2amd] split_close: cannot finish " + fn);
}

void *mm2amd_split_merge_open(const char *prefix, int n_parts, const void *opt)
{
	void *h = nullptr;
	if (!prefix || !opt) { capi_fail(MM2AMD_EINVAL, "[mm2amd] split_merge_open: bad arguments"); return nullptr; }
	guarded([&]() -> int {
		SplitMerger *m = split_merge_open(prefix, n_parts, *(const ref::MapOpt *)opt);
		m->device = split_device_route();
		m->device_pair = pair_device_env();
		h = m;
		return 0;
	});
	return h;
}

int mm2amd_split_merge_batch(void *h, int n_frag, const int *seg_off, const int *n_seg, const void *seq, int *n_reg, void **reg, int *rep_len, int *frag_gap)
{
	if (!h || n_frag < 0 || (n_frag > 0 && (!seq || !n_reg || !reg || !rep_len || !frag_gap))) return capi_fail(MM2AMD_EINVAL, "[mm2amd] split_merge_batch: bad arguments");
	return guarded([&]() -> int { split_merge_batch(*(SplitMerger *)h, n_frag, seg_off, n_seg, (const ref::Bseq1 *)seq, n_reg, reg, rep_len, frag_gap); return 0; });
}

int mm2amd_split_merge_format(void *h, int n_frag, const int *seg_off, const int *n_seg, const void *seq, const int *n_reg, void *const *reg, const int *rep_len, char **out,
                              size_t *out_len)
{
	if (!h || !out || !out_len || n_frag < 0 || (n_frag > 0 && (!seq || !n_reg || !reg))) return capi_fail(MM2AMD_EINVAL, "[mm2amd] split_merge_format: bad arguments");
	return guarded([&]() -> int {
		SplitMerger &m = *(SplitMerger *)h;
		*out = format_batch(m.fi, m.opt, effective_cpus(), n_frag, seg_off, n_seg, (const ref::Bseq1 *)seq, n_reg, reg, rep_len, out_len);
		return *out ? 0 : capi_fail(MM2AMD_ENOMEM, "[mm2amd] split_merge_format: out of memory");
	});
}

int mm2amd_split_merge_sq(void *h, char **out, size_t *out_len)
{
	if (!h || !out || !out_len) return capi_fail(MM2AMD_EINVAL, "[mm2amd] split_merge_sq: bad arguments");
	return guarded([&]() -> int {
		const std::string s = split_sq_lines(*(SplitMerger *)h);
		if (!(*out = (char *)malloc(s.size() + 1))) return capi_fail(MM2AMD_ENOMEM, "[mm2amd] split_merge_sq: out of memory");
		memcpy(*out, s.c_str(), s.size() + 1);
		*out_len = s.size();
		return 0;
	});
}

int mm2amd_split_merge_close(void *h, int remove_tmp)
{
	SplitMerger *m = (SplitMerger *)h;
	if (!m) return 0;
	const std::string prefix = m->prefix;
	const int n = (int)m->fp.size();
	delete m;
	if (remove_tmp) for (int j = 0; j < n; ++j) remove(split_tmp_name(prefix, j).c_str()); // mm_split_rm_tmp (splitidx.c:74-84)
	return 0;
}

int mm2amd_fastx_limits(size_t *max_text, int *long_line)
{
	if (max_text) *max_text = kFastxMaxText;
	if (long_line) *long_line = (int)fastx_long_line();
	return 0;
}

int mm2amd_fastx_last_times(double *out, int cap)
{
	FastxApiState &d = fastx_state();
	std::lock_guard<std::mutex> lk(d.mu);
	int n = 0;
	for (; n < cap && n < 6; ++n) out[n] = d.times[n];
	return n;
}

int mm2amd_fastx_parse_host(const char *text, size_t len, int is_final, int flags, mm2amd_fastx_rec_t *recs, size_t recs_cap, char *pool, size_t pool_cap,
                            size_t *n_recs, size_t *pool_len, size_t *consumed, int *path)
{
	if (const int rc = fastx_check_args("fastx_parse_host", text, len, n_recs, pool_len, consumed, path, SIZE_MAX)) return rc;
	if (len == 0) return 0;
	return guarded([&]() -> int { return fastx_host("fastx_parse_host", text, len, is_final, flags, recs, recs_cap, pool, pool_cap, n_recs, pool_len, consumed); });
}

int mm2amd_fastx_parse(const char *text, size_t len, int is_final, int flags, mm2amd_fastx_rec_t *recs, size_t recs_cap, char *pool, size_t pool_cap,
                       size_t *n_recs, size_t *pool_len, size_t *consumed, int *path)
{
	if (const int rc = fastx_check_args("fastx_parse", text, len, n_recs, pool_len, consumed, path, kFastxMaxText)) return rc;
	return guarded([&]() -> int {
		DeviceCtx &dc = device_ctx();
		FastxApiState &d = fastx_state();
		std::lock_guard<std::mutex> lk(d.mu);
		{ std::lock_guard<std::mutex> lk2(dc.mu); ensure_device(dc); } // (no device: MM2AMD_ENODEV, also for an empty text's caller who asked for the device)
		if (len == 0) return 0;
		HIP_CHECK(hipSetDevice(dc.device_id));
		if (!d.stream) HIP_CHECK(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
		for (double &t : d.times) t = 0;
		const auto to_host = [&]() -> int {
			*path = MM2AMD_FASTX_PATH_HOST;
			const double t0 = Trace::now();
			const int rc = fastx_host("fastx_parse", text, len, is_final, flags, recs, recs_cap, pool, pool_cap, n_recs, pool_len, consumed);
			d.times[5] = Trace::now() - t0;
			return rc;
		};
		const bool fin = is_final != 0, fq = text[0] == '@';
		if (!fq && text[0] != '>') return to_host();
		if (!fq && fin && text[len - 1] == '>' && (len == 1 || text[len - 2] == '\n')) return to_host(); // a file that ends in a lone marker holds no record there
		const bool profiling = KernelProfiler::enabled_flag();
		KernelProfiler &prof = fastx_prof();
		hipStream_t st = d.stream;
		double t0 = Trace::now();
		FastxParams P;
		memset(&P, 0, sizeof P);
		const uint32_t mis = (uint32_t)((uintptr_t)text & 15u);
		P.text = d.d_text.ensure(len + 64) + 16 + mis; // (the buffers come aligned to 256 bytes: the text keeps the caller's alignment modulo 16)
		P.len = (uint32_t)len, P.flags = (uint32_t)flags, P.cls = fq ? MM2AMD_FASTX_PATH_FASTQ4 : MM2AMD_FASTX_PATH_FASTA, P.long_line = fastx_long_line();
		P.n_tiles = (uint32_t)((mis + len + kFastxTile - 1) / kFastxTile);
		P.tile_cnt = d.d_tile.ensure((size_t)P.n_tiles + 1);
		P.state = d.d_state.ensure(4);
		uint32_t *const hw = d.h_word.ensure(8);
		HIP_CHECK(hipMemcpyAsync((void *)P.text, text, len, hipMemcpyHostToDevice, st));
		HIP_CHECK(hipMemsetAsync(P.state, 0, 16, st));
		if (profiling) { stream_wait(st); d.times[0] = Trace::now() - t0; t0 = Trace::now(); }
		// the '\n' of every tile, their running sum, the number of lines
		prof.begin(st); fastx_lines_launch(P, false, st); prof.end(st, "fastx_lines_kernel[count]", (double)len, (double)len);
		device_exclusive_sum_u32(P.tile_cnt, P.tile_cnt, P.n_tiles, st);
		HIP_CHECK(hipMemcpyAsync(hw, P.tile_cnt + P.n_tiles, 4, hipMemcpyDeviceToHost, st));
		stream_wait(st);
		prof.collect();
		if (!profiling) d.times[0] = Trace::now() - t0, t0 = Trace::now(); // (the upload is not timed apart then: it ends within this wait)
		P.n_nl = hw[0];
		if (P.n_nl > len) return capi_fail(MM2AMD_EHIP, "[mm2amd] fastx_parse: the device counted more lines than bytes");
		const uint32_t n_all = P.n_nl + (text[len - 1] != '\n' ? 1u : 0u);
		if (fq) {
			if (fin && (n_all & 3u)) return to_host(); // the file ends inside a record: what the reference makes of the rest is the host's business
			P.n_lines = fin ? n_all : (P.n_nl & ~3u);
			if (P.n_lines == 0) { *path = P.cls; return 0; }
		} else P.n_lines = n_all;
		P.line_off = d.d_line.ensure((size_t)P.n_nl + 2);
		P.dst = d.d_dst.ensure((size_t)P.n_lines + 1), P.name_len = d.d_name.ensure(P.n_lines);
		if (!fq) P.ridx = d.d_ridx.ensure((size_t)P.n_lines + 1);
		P.work_cap = (uint32_t)(2 * (len / P.long_line) + len / kFastxLongChunk + 4);
		P.work = d.d_work.ensure(P.work_cap);
		prof.begin(st); fastx_lines_launch(P, true, st); prof.end(st, "fastx_lines_kernel[write]", (double)len + 4.0 * P.n_nl, (double)len);
		prof.begin(st); fastx_classify_launch(P, st); prof.end(st, "fastx_classify_kernel", 16.0 * P.n_lines, (double)P.n_lines);
		device_exclusive_sum_u32(P.dst, P.dst, P.n_lines, st);
		if (!fq) device_exclusive_sum_u32(P.ridx, P.ridx, P.n_lines, st);
		HIP_CHECK(hipMemcpyAsync(hw, P.state, 12, hipMemcpyDeviceToHost, st));
		HIP_CHECK(hipMemcpyAsync(hw + 3, P.dst + P.n_lines, 4, hipMemcpyDeviceToHost, st));
		if (!fq) HIP_CHECK(hipMemcpyAsync(hw + 4, P.ridx + P.n_lines, 4, hipMemcpyDeviceToHost, st));
		if (fq && !fin) HIP_CHECK(hipMemcpyAsync(hw + 5, P.line_off + P.n_lines, 4, hipMemcpyDeviceToHost, st));
		stream_wait(st);
		prof.collect();
		if (hw[0]) return to_host(); // the buffer is not what its first byte promised
		const uint32_t n_work = hw[1], total = hw[3];
		if (n_work > P.work_cap) return capi_fail(MM2AMD_EHIP, "[mm2amd] fastx_parse: more long-line work items than the text can hold");
		size_t used = len;
		if (fq) {
			P.n_rec = P.n_lines / 4, P.pool_len = total;
			if (!fin) used = hw[5];
		} else if (fin) {
			P.n_rec = hw[4], P.pool_len = total + 1;
		} else { // the last header opens the record the buffer does not complete
			P.n_rec = hw[4] - 1;
			const uint32_t last = hw[2];
			if (last >= P.n_lines) return capi_fail(MM2AMD_EHIP, "[mm2amd] fastx_parse: the device's last header lies outside the line table");
			HIP_CHECK(hipMemcpyAsync(hw + 6, P.dst + last, 4, hipMemcpyDeviceToHost, st));
			HIP_CHECK(hipMemcpyAsync(hw + 7, P.line_off + last, 4, hipMemcpyDeviceToHost, st));
			stream_wait(st);
			P.pool_len = P.n_rec ? hw[6] + 1 : 0, used = P.n_rec ? hw[7] : 0;
		}
		if (used > len || P.pool_len > len + 1 || (size_t)P.n_rec > len) return capi_fail(MM2AMD_EHIP, "[mm2amd] fastx_parse: sizes from the device exceed the text");
		d.times[1] = Trace::now() - t0, t0 = Trace::now();
		*path = P.cls, *n_recs = P.n_rec, *pool_len = P.pool_len, *consumed = used;
		if (!recs || !pool || P.n_rec == 0) return 0;
		if (P.n_rec > recs_cap || P.pool_len > pool_cap) return capi_fail(MM2AMD_ENOMEM, "[mm2amd] fastx_parse: table or pool too small (a call with recs == NULL gives the sizes)");
		P.pool = d.d_pool.ensure((size_t)total + 16), P.recs = d.d_recs.ensure(P.n_rec);
		FastxDevRec *const hr = d.h_recs.ensure(P.n_rec);
		prof.begin(st); fastx_copy_launch(P, false, 0, st); prof.end(st, "fastx_copy_kernel[short]", (double)len + (double)P.pool_len, (double)P.n_lines);
		if (n_work) { prof.begin(st); fastx_copy_launch(P, true, n_work, st); prof.end(st, "fastx_copy_kernel[long]", 0.0, (double)n_work); }
		if (profiling) { stream_wait(st); d.times[2] = Trace::now() - t0; t0 = Trace::now(); }
		HIP_CHECK(hipMemcpyAsync(hr, P.recs, (size_t)P.n_rec * sizeof(FastxDevRec), hipMemcpyDeviceToHost, st));
		HIP_CHECK(hipMemcpyAsync(pool, P.pool, P.pool_len, hipMemcpyDeviceToHost, st));
		stream_wait(st);
		prof.collect();
		d.times[3] = Trace::now() - t0, t0 = Trace::now();
		const bool with_qual = (flags & MM2AMD_FASTX_WITH_QUAL) != 0;
		for (uint32_t r = 0; r < P.n_rec; ++r) { // the public table from the kernels' compact one
			const FastxDevRec &s = hr[r];
			mm2amd_fastx_rec_t &o = recs[r];
			const uint32_t l_seq = fq ? s.l_seq : (r + 1 < P.n_rec ? hr[r + 1].name : P.pool_len) - 1u - s.seq;
			if (s.name >= P.pool_len || s.seq >= P.pool_len || (uint64_t)s.seq + l_seq >= P.pool_len) return capi_fail(MM2AMD_EHIP, "[mm2amd] fastx_parse: a record from the device lies outside the pool");
			o.name = s.name, o.name_len = s.name_len, o.comment_len = s.comment_len, o.comment = s.comment_len ? (uint64_t)s.name + s.name_len + 1 : UINT64_MAX;
			o.seq = s.seq, o.l_seq = (int32_t)l_seq, o.qual = fq && with_qual ? (uint64_t)s.seq + l_seq + 1 : UINT64_MAX, o.reserved = 0;
		}
		d.times[4] = Trace::now() - t0;
		return 0;
	});
}

int mm2amd_sort_pairs_u64(uint64_t *keys, uint64_t *vals, uint64_t n, int bits)
{
	if ((n > 0 && (!keys || !vals)) || bits < 0 || bits > 64 || n >= (1ull << 32)) return capi_fail(MM2AMD_EINVAL, "[mm2amd] sort_pairs_u64: bad arguments (n < 2^32, 0 <= bits <= 64)");
	if (n == 0) return 0;
	return guarded([&]() -> int {
		DeviceScope dev; DeviceCtx &dc = dev.dc;
		DevBuf<uint64_t> k0, v0, k1, v1;
		k0.ensure(n, 1.0), v0.ensure(n, 1.0), k1.ensure(n, 1.0), v1.ensure(n, 1.0);
		HIP_CHECK(hipMemcpyAsync(k0.p, keys, n * 8, hipMemcpyHostToDevice, dc.stream));
		HIP_CHECK(hipMemcpyAsync(v0.p, vals, n * 8, hipMemcpyHostToDevice, dc.stream));
		const int where = device_sort_pairs_u64(k0.p, v0.p, k1.p, v1.p, n, bits, dc.stream);
		HIP_CHECK(hipMemcpyAsync(keys, where ? k1.p : k0.p, n * 8, hipMemcpyDeviceToHost, dc.stream));
		HIP_CHECK(hipMemcpyAsync(vals, where ? v1.p : v0.p, n * 8, hipMemcpyDeviceToHost, dc.stream));
		HIP_CHECK(hipStreamSynchronize(dc.stream));
		return 0;
	});
}

int mm2amd_exclusive_sum_u32(const uint32_t *in, uint32_t *out, uint64_t n)
{
	if (!out || (n > 0 && !in) || n >= (1ull << 32)) return capi_fail(MM2AMD_EINVAL, "[mm2amd] exclusive_sum_u32: bad arguments (n < 2^32)");
	return guarded([&]() -> int {
		DeviceScope dev; DeviceCtx &dc = dev.dc;
		DevBuf<uint32_t> d;
		d.ensure(n + 1, 1.0);
		if (n) HIP_CHECK(hipMemcpyAsync(d.p, in, n * 4, hipMemcpyHostToDevice, dc.stream));
		device_exclusive_sum_u32(d.p, d.p, n, dc.stream);
		HIP_CHECK(hipMemcpyAsync(out, d.p, (n + 1) * 4, hipMemcpyDeviceToHost, dc.stream));
		HIP_CHECK(hipStreamSynchronize(dc.stream));
		return 0;
	});
}

int mm2amd_encode_batch(int n, const char *const *seqs, const int32_t *lens, const int32_t *lens2, uint8_t *out) { return mm2amd_encode_range(n, seqs, lens, lens2, 0, n, out); }

int mm2amd_encode_range(int n, const char *const *seqs, const int32_t *lens, const int32_t *lens2, int lo, int hi, uint8_t *out)
{
	if (n < 0 || !out || (n > 0 && (!seqs || !lens)) || lo < 0 || hi < lo || hi > n) return capi_fail(MM2AMD_EINVAL, "[mm2amd] encode_batch: bad arguments");
	std::vector<uint64_t> unit_off(1, 0); // as begin_batch lays a batch out: units back to back, a pair's mate right after its first read
	std::vector<size_t> frag_unit(1, 0);  // fragment i's first unit
	for (int i = 0; i < n; ++i) {
		const int32_t l2 = lens2 ? lens2[i] : 0;
		if (lens[i] < 0 || l2 < 0 || (lens[i] + (int64_t)l2 > 0 && !seqs[i])) return capi_fail(MM2AMD_EINVAL, "[mm2amd] encode_batch: bad read (negative length or null sequence)");
		unit_off.push_back(unit_off.back() + (uint64_t)lens[i]);
		if (l2 > 0) unit_off.push_back(unit_off.back() + (uint64_t)l2);
		frag_unit.push_back(unit_off.size() - 1);
	}
	const uint64_t total = unit_off.back();
	const size_t n_units = unit_off.size() - 1;
	return guarded([&]() -> int {
		DeviceScope dev; DeviceCtx &dc = dev.dc;
		PinBuf<char> h_ascii;
		DevBuf<uint8_t> d_pool;
		DevBuf<uint64_t> d_off;
		char *h = h_ascii.ensure(total + 32, 1.0); // (the kernel reads whole aligned 16-byte words)
		uint64_t o = 0;
		for (int i = 0; i < n; ++i) {
			const uint64_t l = (uint64_t)lens[i] + (uint64_t)(lens2 ? lens2[i] : 0);
			if (l) memcpy(h + o, seqs[i], l);
			o += l;
		}
		d_pool.ensure(2 * total + 32, 1.0), d_off.ensure(n_units + 1, 1.0);
		HIP_CHECK(hipMemsetAsync(d_pool.p, 0xff, 2 * total + 32, dc.stream));
		HIP_CHECK(hipMemcpyAsync(d_off.p, unit_off.data(), (n_units + 1) * 8, hipMemcpyHostToDevice, dc.stream));
		SeedChainBuffers B;
		B.n_reads = (int)(frag_unit[hi] - frag_unit[lo]), B.seq_off = d_off.p + frag_unit[lo], B.ascii = h, B.qpool = d_pool.p + 16; // (a sub-batch, as the mapper's lanes launch it: the offsets stay the batch's)
		launch_encode(B, dc.stream);
		HIP_CHECK(hipMemcpyAsync(out, d_pool.p, 2 * total + 32, hipMemcpyDeviceToHost, dc.stream));
		HIP_CHECK(hipStreamSynchronize(dc.stream));
		return 0;
	});
}

long long mm2amd_alloc_counter(int which)
{
	AllocStats &a = alloc_stats();
	BandCounters &b = band_counters();
	return which == 0 ? a.dev_allocs.load() : which == 1 ? a.pin_allocs.load() : which == 2 ? a.ns.load() : which == 3 ? (long long)b.n_band1.load() : which == 4 ? (long long)b.n_band2.load() :
	       which == 5 ? (long long)b.n_widened.load() : which == 6 ? (long long)b.n_retried.load() :
	       which == 7 ? (long long)dev_arena().held_bytes() : which == 8 ? (long long)pin_arena().held_bytes() : which == 9 ? (long long)dev_arena().used_bytes() : which == 10 ? (long long)pin_arena().used_bytes() :
	       which == 11 ? (long long)b.n_band4.load() : which == 12 ? (long long)b.n_retried_big.load() :
	       which == 13 ? (long long)prune_counters().n_in.load() : which == 14 ? (long long)prune_counters().n_kept.load() : (long long)prune_counters().n_redo.load();
}

void mm2amd_profile_enable(int on)
{
	for (int r = 0; r < kMaxReplicas; ++r) for (int l = 0; l < kMaxProfLanes; ++l) kernel_profiler(l, r).reset();
	KernelProfiler::enabled_flag() = on != 0;
}

int mm2amd_profile_get(mm2amd_kernel_stat_t *out, int cap)
{
	std::map<std::string, KernelStat> all;
	for (int r = 0; r < kMaxReplicas; ++r) for (int l = 0; l < kMaxProfLanes; ++l)
		for (const auto &kv : kernel_profiler(l, r).stats()) {
			KernelStat &k = all[kv.first];
			k.ms += kv.second.ms, k.alg_bytes += kv.second.alg_bytes, k.units += kv.second.units, k.launches += kv.second.launches;
		}
	int n = 0;
	for (const auto &kv : all) {
		if (n >= cap) break;
		mm2amd_kernel_stat_t &o = out[n++];
		memset(&o, 0, sizeof o);
		strncpy(o.name, kv.first.c_str(), sizeof o.name - 1);
		o.ms = kv.second.ms, o.alg_bytes = kv.second.alg_bytes, o.launches = kv.second.launches, o.units = kv.second.units;
	}
	return n;
}

} // extern "C"
