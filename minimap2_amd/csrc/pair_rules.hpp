// The rules of mm_pair and mm_set_pe_thru (pe.c:50-68, :81-182), written once for pair_kernel (pair_dev.hpp) and for the host (pair.hpp: pe_host_fragment):
// the pieces that do not depend on how the lanes are used.  Single precision where the reference has it, the operations in its order; the
// library is compiled with -ffp-contract=off, and the one transcendental -- logf of a count -- is handed in by the caller (the host's libm, or a
// table the host's libm filled).
#pragma once
#include <cstdint>
#include "../../include/mm2amd.h"
#include "exact_rsort.hpp" // MM2_HD

namespace mm2amd {

// the sort key of an end (pe.c:95): sequence, start, and in the lowest bit whether the hit CLOSES a pair (reverse hit of read 1 / forward hit of
// read 2) or opens one.  rs << 1 | (seg ^ rev) is an int there, widened into the key.
MM2_HD inline uint64_t pe_key(int32_t rid, int32_t rs, int seg, int rev) { return (uint64_t)rid << 32 | (uint64_t)(int64_t)(int32_t)((uint32_t)rs << 1 | (uint32_t)(seg ^ rev)); }
MM2_HD inline bool pe_closes(uint64_t key) { return (key & 1) != 0; }
// a closing end at rs on rid against an earlier end that stops at re on rid_o (pe.c:120, :125)
MM2_HD inline bool pe_in_reach(int32_t rid, int32_t rs, int32_t rid_o, int32_t re_o, int32_t max_gap_ref) { return rid == rid_o && rs - re_o <= max_gap_ref; }
// pe.c:127
MM2_HD inline int64_t pe_score(int32_t dp, int32_t dp_o, uint32_t hash, uint32_t hash_o) { return (int64_t)(dp + dp_o) << 32 | (uint32_t)(hash + hash_o); }
// the bar a pair's dp sum has to reach (pe.c:100, :106-107)
MM2_HD inline int32_t pe_dp_thres(int32_t top0, int32_t top1, int32_t pe_bonus) { const int32_t t = top0 + top1 - pe_bonus; return t < 0 ? 0 : t; }

// What mm_pair needs of its candidate list `sc`: the count, the largest value, sc.a[sc.n - 2] of the sorted list (the second largest counted
// with multiplicity), and who scored the largest first.  at / at_o: where the winning closing end and its partner stand in the sorted list.
struct PeBest { int64_t m1 = -1, m2 = -1; int32_t n = 0, at = -1, at_o = -1; };
MM2_HD inline void pe_take(PeBest &b, int64_t v, int32_t at, int32_t at_o)
{
	++b.n;
	if (v > b.m1) b.m2 = b.m1, b.m1 = v, b.at = at, b.at_o = at_o; // strict: among equal scores the first one met stays (pe.c:128)
	else if (v > b.m2) b.m2 = v;
}
// two parts of one scan; closing ends ascend within a part, and of two equal maxima the one with the smaller closing end was met first
MM2_HD inline PeBest pe_merge(const PeBest &x, const PeBest &y)
{
	const bool x_first = x.m1 > y.m1 || (x.m1 == y.m1 && x.at <= y.at);
	const PeBest &hi = x_first ? x : y, &lo = x_first ? y : x;
	PeBest r = hi;
	r.n = x.n + y.n;
	r.m2 = lo.m1 > hi.m2 ? lo.m1 : hi.m2;
	return r;
}
// pe.c:160: does a candidate count towards n_sub?  Unsigned 64-bit, as there.
MM2_HD inline bool pe_near(int64_t v, int64_t best, int32_t sub_diff) { return ((uint64_t)v >> 32) + (uint64_t)(int64_t)sub_diff >= (uint64_t)best >> 32; }

// The MAPQ tail (pe.c:158-175): the two hits' MAPQ after pairing.  runner_up: sc.a[sc.n - 2], read only when n_pairs > 1; logf_n_sub: logf((float)n_sub).
// The results are what the 8-bit field mm_reg1_t::mapq keeps of them.
MM2_HD inline void pe_pair_mapq(int32_t mapq0, int32_t mapq1, int64_t best, int64_t runner_up, int32_t n_pairs, int32_t n_sub, int32_t match_sc, float logf_n_sub, int32_t *out0, int32_t *out1)
{
	(void)n_sub;
	int mapq_pe = mapq0 > mapq1 ? mapq0 : mapq1;
	if (n_pairs > 1) {
		const uint64_t lead = (uint64_t)(best >> 32) - ((uint64_t)runner_up >> 32); // pe.c:164: int64 minus uint64
		const float by_lead = 6.02f * (float)lead;
		const float per_match = by_lead / (float)match_sc;
		const float crowd = 4.343f * logf_n_sub;
		const int mapq_pe_alt = (int)(per_match - crowd);
		mapq_pe = mapq_pe < mapq_pe_alt ? mapq_pe : mapq_pe_alt;
	}
	int32_t m[2] = { mapq0, mapq1 };
	for (int s = 0; s < 2; ++s) {
		if (m[s] < mapq_pe) {
			const float own = .2f * (float)m[s], pair = .8f * (float)mapq_pe;
			const float sum = own + pair;
			m[s] = (int32_t)(uint8_t)(int)(sum + .499f);
		}
		if (n_pairs == 1) { if (m[s] < 2) m[s] = 2; }
		else if ((uint64_t)best >> 32 > (uint64_t)runner_up >> 32) { if (m[s] < 1) m[s] = 1; }
	}
	*out0 = m[0], *out1 = m[1];
}

// mm_set_pe_thru's test of the two segments' only primaries (pe.c:62-63)
MM2_HD inline int32_t pe_abs(int32_t x) { return x < 0 ? -x : x; }
MM2_HD inline bool pe_thru(const mm2amd_pe_hit_t &p, const mm2amd_pe_hit_t &q, int32_t qlen0, int32_t qlen1)
{
	return p.rid == q.rid && (p.flags & MM2AMD_PE_REV) == (q.flags & MM2AMD_PE_REV) && pe_abs(p.rs - q.rs) < 3 && pe_abs(p.re - q.re) < 3 &&
	       ((p.qs == 0 && qlen1 - q.qe == 0) || (q.qs == 0 && qlen0 - p.qe == 0));
}

// What the found pair does to the hits of one segment (pe.c:143-157), as a function of each hit: `b` is the segment's hit of the pair at position
// b_pos, b_mapq its MAPQ from pe_pair_mapq.  old_pos: the position of the primary it replaces, -1 when it was a primary already.
struct PeLift { int32_t b_pos = -1, b_id = 0, b_mapq = 0, old_pos = -1, old_id = 0, moves_sam_pri = 0; };
MM2_HD inline PeLift pe_lift(const mm2amd_pe_hit_t *seg_hits, int32_t b_pos)
{
	PeLift L;
	const mm2amd_pe_hit_t &b = seg_hits[b_pos];
	L.b_pos = b_pos, L.b_id = b.id, L.b_mapq = b.mapq;
	if (b.id != b.parent) { // (parent indexes the segment: checked before)
		L.old_pos = b.parent, L.old_id = seg_hits[b.parent].id;
		if (L.old_pos == b_pos) L.b_mapq = 0; // p->mapq = 0 comes before the pair's MAPQ is read
	}
	L.moves_sam_pri = b.flags & MM2AMD_PE_SAM_PRI ? 0 : 1;
	return L;
}
// the hit at position pos of a segment after mm_pair, before mm_set_pe_thru; L.b_pos < 0: no pair was found
MM2_HD inline mm2amd_pe_out_t pe_hit_out(const mm2amd_pe_hit_t &h, int32_t pos, const PeLift &L)
{
	mm2amd_pe_out_t o;
	o.parent = h.parent, o.mapq = h.mapq, o.flags = h.flags & MM2AMD_PE_SAM_PRI, o.reserved = 0;
	if (L.b_pos < 0) return o;
	if (L.old_pos >= 0) {
		if (h.parent == L.old_id) o.parent = L.b_id;
		if (pos == L.old_pos) o.mapq = 0;
	}
	if (L.moves_sam_pri) o.flags = 0;
	if (pos == L.b_pos) o.mapq = L.b_mapq, o.flags = MM2AMD_PE_SAM_PRI | MM2AMD_PE_PROPER_FRAG;
	return o;
}

} // namespace mm2amd
