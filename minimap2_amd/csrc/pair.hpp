// pair_kernel (pair_dev.hpp, compiled with region_finish.hip): mm_pair and mm_set_pe_thru (pe.c:50-68, :81-182) for a batch of two-segment
// fragments, one wavefront per fragment.  DESIGN.md section 3j has the formulation.  Host-side declarations, and the same rules on the host
// (pe_host_fragment: the host class and mm2amd_pair_host_batch).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/mm2amd.h"
#include "pair_rules.hpp"
#include "abi_ref.hpp"

namespace mm2amd {

// A fragment's working set in LDS, per end: its key as the input has it (8), and at its rank the key (8), rs and re (4 + 4), dp_max (4), hash (4)
// and the input position (4).
constexpr int kPeBytesPerEnd = 8 + 8 + 4 + 4 + 4 + 4 + 4;
constexpr int kPeNarrowCap = 64;   // 2.3 KB per wavefront: the workgroups of a CU are bounded by its wave slots, not by LDS
constexpr int kPeWideCap = 1024;   // 36 KB: four workgroups in a CU's 160 KB
constexpr int kPeMaxHits = 1 << 20; // of one segment
constexpr int kPeExactSortMax = 64; // RS_MIN_SIZE (ksort.h:98): up to here radix_sort_pair is a stable insertion sort, and equal keys keep the input's order
constexpr int kPeLogTable = (kPeWideCap / 2) * (kPeWideCap / 2); // the most candidates a fragment of the wide class has: logf(1) .. logf(this) on the device

struct PairParams {
	const mm2amd_pe_hit_t *hits; // hits and out start at offset `first`
	uint64_t first;
	const mm2amd_pe_frag_t *frag;
	const uint32_t *list;        // the fragments of this launch: block b runs fragment list[b]
	int n_list;
	mm2amd_pe_out_t *out;        // per hit
	mm2amd_pe_res_t *res;        // per fragment
	mm2amd_pe_opt_t opt;
	const float *logf_tab;       // [n] = logf((float)n), n = 0 .. kPeLogTable ([0] is never read)
	int cap, path;               // ends the launch's LDS holds; what res[].path says
};

void pair_launch(const PairParams &P, void *stream);

// do the parents of a fragment's hits index their own segment?  (regs[s][r->parent], pe.c:146, reads there)
MM2_HD inline bool pe_parent_ok(const mm2amd_pe_hit_t &h, int32_t n_seg_hits) { return h.parent >= 0 && h.parent < n_seg_hits; }

MM2_HD inline void pe_res_none(mm2amd_pe_res_t &r, int path, int status) { r.path = path, r.status = status, r.n_pairs = 0, r.best[0] = r.best[1] = -1, r.reserved = 0; }

// MM2AMD_DEVICE_PAIR=1: the places that pair today -- the mapper's finish step and the split-index merge -- send their fragments through
// mm_pair's device form; unset or 0 is the host routine (hits.cpp: pair_hits).  Read where the context or the merger is created.
inline bool pair_device_env() { const char *e = getenv("MM2AMD_DEVICE_PAIR"); return e && *e && strcmp(e, "0") != 0; }

// a hit record as the entry points take it (r.p is not null), and an answer put back into the record
inline void pe_flat_hit(mm2amd_pe_hit_t &h, const ref::Reg1 &r)
{
	h.rid = r.rid, h.rs = r.rs, h.re = r.re, h.qs = r.qs, h.qe = r.qe, h.dp_max = r.p->dp_max, h.id = r.id, h.parent = r.parent, h.mapq = (int32_t)r.mapq, h.hash = r.hash;
	h.flags = (r.rev ? MM2AMD_PE_REV : 0u) | (r.sam_pri ? MM2AMD_PE_SAM_PRI : 0u), h.reserved = 0;
}
inline void pe_apply(ref::Reg1 &r, const mm2amd_pe_out_t &o)
{
	r.parent = o.parent, r.mapq = (uint32_t)o.mapq, r.sam_pri = o.flags & MM2AMD_PE_SAM_PRI ? 1 : 0;
	if (o.flags & MM2AMD_PE_PROPER_FRAG) r.proper_frag = 1;
	if (o.flags & MM2AMD_PE_THRU) r.pe_thru = 1;
}

// one fragment on the host: hits[0, n0 + n1) -> out[0, n0 + n1), *res
inline void pe_host_fragment(const mm2amd_pe_frag_t &F, const mm2amd_pe_hit_t *hits, const mm2amd_pe_opt_t &opt, mm2amd_pe_out_t *out, mm2amd_pe_res_t *res, int path)
{
	struct End { uint64_t key; int32_t src; };
	thread_local std::vector<End> a;
	const int n0 = F.n[0], n1 = F.n[1], n = n0 + n1;
	const PeLift none;
	pe_res_none(*res, path, MM2AMD_PE_OK);
	for (int i = 0; i < n; ++i) out[i] = pe_hit_out(hits[i], 0, none);
	if (n0 <= 0 || n1 <= 0) return; // only one end is mapped: pe.c:102-105 returns before mm_set_pe_thru
	for (int i = 0; i < n; ++i)
		if (!pe_parent_ok(hits[i], i < n0 ? n0 : n1)) { res->status = MM2AMD_PE_BAD_PARENT; return; }
	a.resize((size_t)n);
	int32_t top[2] = { 0, 0 };
	for (int i = 0; i < n; ++i) {
		const int s = i >= n0;
		a[(size_t)i] = End{ pe_key(hits[i].rid, hits[i].rs, s, hits[i].flags & MM2AMD_PE_REV ? 1 : 0), i };
		top[s] = top[s] > hits[i].dp_max ? top[s] : hits[i].dp_max;
	}
	const int32_t bar = pe_dp_thres(top[0], top[1], opt.pe_bonus);
	{ RsortScratch scratch; exact_radix_sort(a.data(), a.data() + n, [](const End &e) { return e.key; }, scratch); } // radix_sort_pair: the unstable sort, replayed exactly
	const auto seg_of = [&](int k) { return a[(size_t)k].src >= n0 ? 1 : 0; };
	const auto rev_of = [&](int k) { return (int)(a[(size_t)k].key & 1) ^ seg_of(k); };
	const auto walk = [&](int i, int from, auto &&take) { // pe.c:121-131
		const mm2amd_pe_hit_t &c = hits[a[(size_t)i].src];
		for (int j = from; j >= 0; --j) {
			if (rev_of(j) != rev_of(i) || seg_of(j) == seg_of(i)) continue;
			const mm2amd_pe_hit_t &o = hits[a[(size_t)j].src];
			if (!pe_in_reach(c.rid, c.rs, o.rid, o.re, F.max_gap_ref)) break;
			if (c.dp_max + o.dp_max < bar) continue;
			take(pe_score(c.dp_max, o.dp_max, c.hash, o.hash), j);
		}
	};
	const auto scan = [&](auto &&take) { // pe.c:114-135
		int last[2] = { -1, -1 };
		for (int i = 0; i < n; ++i) {
			if (!pe_closes(a[(size_t)i].key)) { last[rev_of(i)] = i; continue; }
			const int from = last[rev_of(i)];
			if (from < 0) continue;
			const mm2amd_pe_hit_t &c = hits[a[(size_t)i].src], &o = hits[a[(size_t)from].src];
			if (!pe_in_reach(c.rid, c.rs, o.rid, o.re, F.max_gap_ref)) continue;
			walk(i, from, [&](int64_t v, int j) { take(v, i, j); });
		}
	};
	PeBest B;
	scan([&](int64_t v, int i, int j) { pe_take(B, v, i, j); });
	res->n_pairs = B.n;
	PeLift L[2];
	if (B.n > 0 && B.m1 > 0) { // found at least one pair
		int32_t n_sub = 0;
		scan([&](int64_t v, int, int) { n_sub += pe_near(v, B.m1, opt.sub_diff) ? 1 : 0; });
		const int src_c = a[(size_t)B.at].src, src_o = a[(size_t)B.at_o].src;
		const int at[2] = { src_c < n0 ? src_c : src_o, src_c < n0 ? src_o - n0 : src_c - n0 };
		L[0] = pe_lift(hits, at[0]), L[1] = pe_lift(hits + n0, at[1]);
		pe_pair_mapq(L[0].b_mapq, L[1].b_mapq, B.m1, B.m2, B.n, n_sub, opt.match_sc, logf((float)n_sub), &L[0].b_mapq, &L[1].b_mapq);
		res->best[0] = at[0], res->best[1] = at[1];
		for (int i = 0; i < n; ++i) out[i] = i < n0 ? pe_hit_out(hits[i], i, L[0]) : pe_hit_out(hits[i], i - n0, L[1]);
	}
	// mm_set_pe_thru
	int n_pri[2] = { 0, 0 }, pri[2] = { -1, -1 };
	for (int i = 0; i < n; ++i) if (hits[i].id == out[i].parent) ++n_pri[i >= n0], pri[i >= n0] = i;
	if (n_pri[0] == 1 && n_pri[1] == 1 && pe_thru(hits[pri[0]], hits[pri[1]], F.qlen[0], F.qlen[1])) out[pri[0]].flags |= MM2AMD_PE_THRU, out[pri[1]].flags |= MM2AMD_PE_THRU;
}

} // namespace mm2amd
