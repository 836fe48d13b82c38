// pair_kernel: see pair.hpp.  Included by region_finish.hip.
//
// One wavefront (a workgroup of 64) per fragment; the fragment's ends -- the hits of segment 0, then those of segment 1 -- live in LDS.
//   [order]   every lane takes ends lane, lane + 64, ...: the key of pe.c:95, then the end's rank -- the ends with a smaller key, plus those with an
//             equal key that come EARLIER in the input.  That is radix_sort_pair's order for up to 64 ends (a stable insertion sort).  Beyond 64 the
//             order among equal keys is the cycle walk's: a fragment with more than 64 ends and a tie says MM2AMD_PE_PATH_HOST and stops; without
//             a tie the ranks are the order whatever the sort.  An end's fields are stored at its rank: nothing is moved.
//   [scan]    closing ends are independent (pe.c:114-135 reads last[] and writes only max and sc): a lane per closing end, lanes striding.  The
//             lane looks back for the nearest earlier opening end of its strand (last[rev]), tests the reach against it, and walks from there to 0.
//             sc is never built: a lane keeps the count, the two largest scores and who scored the largest first (pair_rules.hpp: PeBest); the lanes'
//             closing ends ascend, so a butterfly of pe_merge gives the reference's argmax.  n_sub is a second pass of the same walks.
//   [outcome] wave-uniform: the two hits of the pair, the lift, the pair's MAPQ (logf from the host's table); then every hit's answer is a function
//             of its own record (pe_hit_out), and mm_set_pe_thru's primaries are counted across the lanes.
// Every loop is bounded by n <= P.cap, every index into LDS is below n (the ranks of n ends are a permutation of 0 .. n - 1: the order is total),
// every index into hits and out is below the fragment's end, and parent is checked before it is used as an index.
#pragma once
#include <hip/hip_runtime.h>
#include "hip_util.hpp"
#include "pair.hpp"

namespace mm2amd {

namespace {
__device__ __forceinline__ int pe_wave_sum(int v)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
	return v;
}
__device__ __forceinline__ int pe_wave_max(int v)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
	return v;
}
__device__ __forceinline__ PeBest pe_wave_best(PeBest b)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		PeBest o;
		o.m1 = (int64_t)__shfl_xor((long long)b.m1, d, 64), o.m2 = (int64_t)__shfl_xor((long long)b.m2, d, 64);
		o.n = __shfl_xor(b.n, d, 64), o.at = __shfl_xor(b.at, d, 64), o.at_o = __shfl_xor(b.at_o, d, 64);
		b = pe_merge(b, o); // (symmetric: both partners of an exchange arrive at the same record)
	}
	return b;
}
} // namespace

__global__ void __launch_bounds__(64) pair_kernel(PairParams P)
{
	MM2_DYN_LDS(unsigned char, lds);
	const int lane = (int)threadIdx.x;
	const uint32_t f = P.list[blockIdx.x];
	const mm2amd_pe_frag_t F = P.frag[f];
	const int n0 = F.n[0], n1 = F.n[1];
	mm2amd_pe_res_t *const res = P.res + f;
	if (n0 < 0 || n1 < 0 || (int64_t)n0 + n1 > (int64_t)P.cap) { // (the host sorts the fragments into the launches by this very number)
		if (lane == 0) pe_res_none(*res, MM2AMD_PE_PATH_HOST, MM2AMD_PE_OK);
		return;
	}
	const int n = n0 + n1, C = P.cap;
	const mm2amd_pe_hit_t *const hits = P.hits + (F.hit0 - P.first);
	mm2amd_pe_out_t *const out = P.out + (F.hit0 - P.first);
	uint64_t *const key_in = (uint64_t *)lds;
	uint64_t *const key = (uint64_t *)(lds + (size_t)8 * C);
	int32_t *const rs = (int32_t *)(lds + (size_t)16 * C);
	int32_t *const re = (int32_t *)(lds + (size_t)20 * C);
	int32_t *const dp = (int32_t *)(lds + (size_t)24 * C);
	uint32_t *const hash = (uint32_t *)(lds + (size_t)28 * C);
	int32_t *const src = (int32_t *)(lds + (size_t)32 * C);
	const PeLift none;

	// ---- an unmapped mate (pe.c:102-105), or a parent that does not index its segment: every hit as it came
	bool bad = false;
	for (int i = lane; i < n; i += 64) bad |= !pe_parent_ok(hits[i], i < n0 ? n0 : n1);
	const bool refused = __ballot(bad) != 0;
	if (n0 == 0 || n1 == 0 || refused) {
		for (int i = lane; i < n; i += 64) out[i] = pe_hit_out(hits[i], 0, none);
		if (lane == 0) pe_res_none(*res, P.path, n0 > 0 && n1 > 0 ? MM2AMD_PE_BAD_PARENT : MM2AMD_PE_OK);
		return;
	}

	// ---- order
	int top0 = 0, top1 = 0;
	for (int i = lane; i < n; i += 64) {
		const mm2amd_pe_hit_t h = hits[i];
		const int s = i >= n0;
		key_in[i] = pe_key(h.rid, h.rs, s, h.flags & MM2AMD_PE_REV ? 1 : 0);
		if (s) top1 = top1 > h.dp_max ? top1 : h.dp_max;
		else top0 = top0 > h.dp_max ? top0 : h.dp_max;
	}
	const int32_t bar = pe_dp_thres(pe_wave_max(top0), pe_wave_max(top1), P.opt.pe_bonus);
	__syncthreads();
	bool tie = false;
	for (int i = lane; i < n; i += 64) {
		const uint64_t k = key_in[i];
		int rank = 0;
		for (int j = 0; j < n; ++j) {
			const uint64_t kj = key_in[j];
			rank += kj < k || (kj == k && j < i) ? 1 : 0;
			tie |= kj == k && j != i;
		}
		const mm2amd_pe_hit_t h = hits[i];
		key[rank] = k, rs[rank] = h.rs, re[rank] = h.re, dp[rank] = h.dp_max, hash[rank] = h.hash, src[rank] = i;
	}
	if (__ballot(tie) != 0 && n > kPeExactSortMax) {
		if (lane == 0) pe_res_none(*res, MM2AMD_PE_PATH_HOST, MM2AMD_PE_OK);
		return;
	}
	__syncthreads();

	// ---- scan.  seg and rev of the end at rank k: seg = src[k] >= n0, and the key's lowest bit is seg ^ rev
	const auto seg_of = [&](int k) { return src[k] >= n0 ? 1 : 0; };
	const auto rev_of = [&](int k) { return (int)(key[k] & 1) ^ seg_of(k); };
	const auto scan = [&](auto &&take) {
		for (int i = lane; i < n; i += 64) {
			const uint64_t ki = key[i];
			if (!pe_closes(ki)) continue;
			const int seg_i = seg_of(i), rev_i = rev_of(i), rid_i = (int32_t)(ki >> 32);
			int from = -1; // last[rev] when the reference's loop stands at i
			for (int j = i - 1; j >= 0; --j)
				if (!pe_closes(key[j]) && rev_of(j) == rev_i) { from = j; break; }
			if (from < 0 || !pe_in_reach(rid_i, rs[i], (int32_t)(key[from] >> 32), re[from], F.max_gap_ref)) continue;
			for (int j = from; j >= 0; --j) {
				if (rev_of(j) != rev_i || seg_of(j) == seg_i) continue;
				if (!pe_in_reach(rid_i, rs[i], (int32_t)(key[j] >> 32), re[j], F.max_gap_ref)) break;
				if (dp[i] + dp[j] < bar) continue;
				take(pe_score(dp[i], dp[j], hash[i], hash[j]), i, j);
			}
		}
	};
	PeBest B;
	scan([&](int64_t v, int i, int j) { pe_take(B, v, i, j); });
	B = pe_wave_best(B);

	// ---- outcome
	PeLift L0, L1;
	int best0 = -1, best1 = -1;
	if (B.n > 0 && B.m1 > 0) {
		int n_sub = 0;
		scan([&](int64_t v, int, int) { n_sub += pe_near(v, B.m1, P.opt.sub_diff) ? 1 : 0; });
		n_sub = pe_wave_sum(n_sub);
		const int src_c = src[B.at], src_o = src[B.at_o];
		best0 = src_c < n0 ? src_c : src_o, best1 = src_c < n0 ? src_o - n0 : src_c - n0;
		L0 = pe_lift(hits, best0), L1 = pe_lift(hits + n0, best1);
		const int at_tab = n_sub < 1 ? 1 : n_sub > kPeLogTable ? kPeLogTable : n_sub; // (1 <= n_sub <= n0 * n1 <= kPeLogTable: the clamp is never taken)
		pe_pair_mapq(L0.b_mapq, L1.b_mapq, B.m1, B.m2, B.n, n_sub, P.opt.match_sc, P.logf_tab[at_tab], &L0.b_mapq, &L1.b_mapq);
	}
	// mm_set_pe_thru: the primaries after the lift, counted across the lanes; then every hit is written once, by its own lane
	int n_pri0 = 0, n_pri1 = 0, pri0 = -1, pri1 = -1;
	for (int i = lane; i < n; i += 64) {
		const mm2amd_pe_hit_t h = hits[i];
		const mm2amd_pe_out_t o = i < n0 ? pe_hit_out(h, i, L0) : pe_hit_out(h, i - n0, L1);
		if (h.id == o.parent) {
			if (i < n0) ++n_pri0, pri0 = i;
			else ++n_pri1, pri1 = i;
		}
	}
	n_pri0 = pe_wave_sum(n_pri0), n_pri1 = pe_wave_sum(n_pri1), pri0 = pe_wave_max(pri0), pri1 = pe_wave_max(pri1);
	const bool thru = n_pri0 == 1 && n_pri1 == 1 && pe_thru(hits[pri0], hits[pri1], F.qlen[0], F.qlen[1]); // (pri0 < n0 <= pri1 < n when the counts are 1)
	for (int i = lane; i < n; i += 64) {
		mm2amd_pe_out_t o = i < n0 ? pe_hit_out(hits[i], i, L0) : pe_hit_out(hits[i], i - n0, L1);
		if (thru && (i == pri0 || i == pri1)) o.flags |= MM2AMD_PE_THRU;
		out[i] = o;
	}
	if (lane == 0) res->path = P.path, res->status = MM2AMD_PE_OK, res->n_pairs = B.n, res->best[0] = best0, res->best[1] = best1, res->reserved = 0;
}

void pair_launch(const PairParams &P, void *stream)
{
	if (P.n_list <= 0) return;
	hipLaunchKernelGGL(pair_kernel, dim3(P.n_list), dim3(64), (size_t)kPeBytesPerEnd * (size_t)P.cap, (hipStream_t)stream, P);
	HIP_CHECK(hipGetLastError());
}

} // namespace mm2amd
