// hits_merge_kernel (hits_merge_dev.hpp, compiled with region_finish.hip): what merge_hits (map.c:520-531) does to a read segment's hits once the
// records of all index parts are in one list -- sort, parents, secondaries, SAM primary -- one wavefront per segment.  DESIGN.md section 3i has
// the formulation.  Host-side declarations, and the same rules on the host (hm_host_segment: the host class and mm2amd_hits_merge_host_batch).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../include/mm2amd.h"
#include "hit_rules.hpp"

namespace mm2amd {

// A segment's working set in LDS, per hit: the record (80), an mm_extra_t header for its p to point at (28 in a 32-byte slot), the sort key -- later
// the clipped interval of mm_set_parent -- (8), the primaries' list, hr_renumber's table, the input position (4 each), a keep flag (1).
constexpr int kHmBytesPerHit = 80 + 32 + 8 + 4 + 4 + 4 + 1;
constexpr int kHmNarrowCap = 64;   // 8.5 KB per wavefront: 18 workgroups per CU by LDS
constexpr int kHmWideCap = 448;    // 58.2 KB: two workgroups in a CU's 160 KB
constexpr int kHmMaxHits = 1 << 20;
constexpr int kHmExactSortMax = 64; // RS_MIN_SIZE (ksort.h:98): up to here radix_sort_128x is a stable insertion sort, and equal keys keep a fixed order

struct HitsMergeParams {
	const mm2amd_hm_hit_t *hits;
	const uint64_t *seg_off; // as the caller gave them; hits and out start at offset `first`
	uint64_t first;
	const uint32_t *list;   // the segments of this launch: block b runs segment list[b]
	int n_list;
	mm2amd_hm_out_t *out;   // per hit
	mm2amd_hm_seg_t *seg;   // per segment
	mm2amd_hm_opt_t opt;
	int cap, path;          // hits the launch's LDS holds; what seg[].path says
};

void hits_merge_launch(const HitsMergeParams &P, void *stream);

// a record of the list from its flat form; ex: the header its p points at
MM2_HD inline void hm_make_reg(ref::Reg1 &r, ref::Extra *ex, const mm2amd_hm_hit_t &h)
{
	__builtin_memset(&r, 0, sizeof r);
	r.cnt = h.cnt, r.rid = h.rid, r.score = h.score, r.qs = h.qs, r.qe = h.qe, r.rs = h.rs, r.re = h.re, r.hash = h.hash;
	r.rev = h.flags & MM2AMD_HM_REV ? 1 : 0, r.inv = h.flags & MM2AMD_HM_INV ? 1 : 0, r.is_alt = h.flags & MM2AMD_HM_ALT ? 1 : 0;
	r.sam_pri = h.flags & MM2AMD_HM_SAM_PRI ? 1 : 0, r.strand_retained = h.flags & MM2AMD_HM_STRAND_RETAINED ? 1 : 0;
	r.parent = ref::PARENT_UNSET;
	if (h.flags & MM2AMD_HM_ALIGNED) {
		__builtin_memset(ex, 0, sizeof(ref::Extra));
		ex->dp_max = h.dp_max;
		r.p = ex;
	}
}
MM2_HD inline uint64_t hm_key(const mm2amd_hm_hit_t &h, float alt_drop)
{
	return hr_sort_key(h.flags & MM2AMD_HM_ALIGNED ? h.dp_max : h.score, h.hash, (h.flags & MM2AMD_HM_ALT) != 0, alt_drop);
}
MM2_HD inline bool hm_live(const mm2amd_hm_hit_t &h) { return (h.flags & MM2AMD_HM_INV) || h.cnt > 0; }
MM2_HD inline void hm_make_out(mm2amd_hm_out_t &o, const ref::Reg1 &r, int pos)
{
	o.pos = pos, o.id = r.id, o.parent = r.parent, o.subsc = r.subsc, o.n_sub = r.n_sub, o.dp_max2 = r.p ? r.p->dp_max2 : 0;
	o.flags = (r.sam_pri ? MM2AMD_HM_SAM_PRI : 0u) | (r.strand_retained ? MM2AMD_HM_STRAND_RETAINED : 0u);
	o.reserved = 0;
}

// one segment on the host: hits[0, n) -> out[0, n), *seg
inline void hm_host_segment(const mm2amd_hm_hit_t *hits, int n, const mm2amd_hm_opt_t &opt, mm2amd_hm_out_t *out, mm2amd_hm_seg_t *seg)
{
	thread_local std::vector<ref::Reg1> r;
	thread_local std::vector<uint64_t> exw; // 32 bytes per hit: the header its p points at
	thread_local std::vector<Anchor> ranked;
	thread_local std::vector<uint64_t> cov;
	thread_local std::vector<int32_t> prim, where, src;
	thread_local std::vector<uint8_t> keep;
	r.resize((size_t)n), exw.resize((size_t)n * 4), cov.resize((size_t)n), prim.resize((size_t)n), where.resize((size_t)n), src.resize((size_t)n), keep.resize((size_t)n);
	const auto ex = [&](int k) { return (ref::Extra *)(exw.data() + (size_t)k * 4); };
	memset(out, 0, sizeof(mm2amd_hm_out_t) * (size_t)n);
	for (int i = 0; i < n; ++i) out[i].pos = -1;
	int m = 0; // the sorted list
	if (n <= 1) { // (hit.c:194)
		for (int i = 0; i < n; ++i) hm_make_reg(r[i], ex(i), hits[i]), src[i] = i;
		m = n;
	} else {
		ranked.clear();
		for (int i = 0; i < n; ++i) if (hm_live(hits[i])) ranked.push_back(Anchor{hm_key(hits[i], opt.alt_drop), (uint64_t)i});
		thread_local RsortScratch sc;
		exact_radix_sort(ranked.data(), ranked.data() + ranked.size(), [](const Anchor &a) { return a.x; }, sc);
		m = (int)ranked.size();
		for (int k = 0; k < m; ++k) { const int i = (int)ranked[(size_t)(m - 1 - k)].y; hm_make_reg(r[k], ex(k), hits[i]), src[k] = i; }
	}
	const bool hard = (opt.flags & MM2AMD_HM_HARD_MLEVEL) != 0;
	if (opt.flags & MM2AMD_HM_WAVE_PARENTS) hr_mark_parents_lanes(r.data(), m, cov.data(), prim.data(), opt.mask_level, opt.mask_len, opt.sub_diff, hard, opt.alt_drop, 64);
	else hr_mark_parents(r.data(), m, cov.data(), prim.data(), opt.mask_level, opt.mask_len, opt.sub_diff, hard, opt.alt_drop);
	int kept = m;
	if (!(opt.flags & MM2AMD_HM_ALL_CHAINS)) {
		if (opt.pri_ratio > 0.0f && m > 0) { // (hit.c:257)
			hr_select_secondaries(r.data(), m, keep.data(), opt.pri_ratio, opt.min_diff, opt.best_n, (opt.flags & MM2AMD_HM_CHECK_STRAND) != 0, opt.min_strand_sc);
			kept = 0;
			for (int i = 0; i < m; ++i) if (keep[i]) r[kept] = r[i], src[kept] = src[i], ++kept;
			if (kept != m) hr_renumber(r.data(), kept, where.data(), m);
		}
		hr_mark_sam_primary(r.data(), kept);
	}
	for (int k = 0; k < kept; ++k) hm_make_out(out[src[k]], r[k], k);
	seg->n_kept = kept, seg->path = MM2AMD_HM_PATH_HOST;
}

} // namespace mm2amd
