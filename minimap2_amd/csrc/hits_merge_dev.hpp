// hits_merge_kernel: see hits_merge.hpp.  Included by region_finish.hip.
//
// One wavefront (a workgroup of 64) per read segment; the segment's records live in LDS from the sort to the last rule.
//   [sort]     every lane takes hits lane, lane + 64, ...: the key of mm_hit_sort, then the hit's rank -- the live hits with a larger key, plus those
//              with an equal key that come LATER in the list.  That is the reference's order for up to 64 live hits (radix_sort_128x is then a stable
//              insertion sort, and mm_hit_sort reads its result backwards).  Beyond 64 the order among equal keys is the cycle walk's: a segment with
//              more than 64 live hits and a tie says MM2AMD_HM_PATH_HOST and stops; without a tie the ranks are the order whatever the sort.
//              The record is built at its rank: nothing is moved.
//   [parents]  hit i against the primaries so far, which are spread over the lanes (hit_rules.hpp: hr_wave_clip / hr_wave_cov_part, a wave sum;
//              hr_wave_owns, a ballot per 64 primaries); lane 0 commits.  Everything that decides the control flow is wave-uniform.
//   [select]   hr_select_secondaries counts as it goes: lane 0.  The compaction is the wave's (64 records at a time, a ballot gives the places);
//              hr_renumber and hr_mark_sam_primary are lane 0's again.
//   [out]      the place of every input hit through a table in LDS, then one store per hit.
// Every index into LDS is below n <= P.cap (the ranks of n_live hits are a permutation of 0 .. n_live - 1: the order is total), every index into
// out is below the segment's end.
#pragma once
#include <hip/hip_runtime.h>
#include "hip_util.hpp"
#include "hits_merge.hpp"

namespace mm2amd {

namespace {
__device__ __forceinline__ int hm_wave_sum(int v)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
	return v;
}
} // namespace

__global__ void __launch_bounds__(64) hits_merge_kernel(HitsMergeParams P)
{
	MM2_DYN_LDS(unsigned char, lds);
	const int lane = (int)threadIdx.x;
	const uint32_t s = P.list[blockIdx.x];
	const uint64_t base = P.seg_off[s] - P.first;
	const uint64_t n64 = P.seg_off[s + 1] - P.seg_off[s];
	if (n64 > (uint64_t)P.cap) { // (the host sorts the segments into the launches by this very number)
		if (lane == 0) P.seg[s].n_kept = -1, P.seg[s].path = MM2AMD_HM_PATH_HOST;
		return;
	}
	const int n_in = (int)n64, C = P.cap;
	ref::Reg1 *const r = (ref::Reg1 *)lds;
	unsigned char *const exb = lds + (size_t)80 * C;
	uint64_t *const keys = (uint64_t *)(lds + (size_t)112 * C); // the sort keys, then mm_set_parent's clipped intervals
	int32_t *const prim = (int32_t *)(lds + (size_t)120 * C);
	int32_t *const where = (int32_t *)(lds + (size_t)124 * C);
	int32_t *const src = (int32_t *)(lds + (size_t)128 * C);
	uint8_t *const keep = lds + (size_t)132 * C;
	const mm2amd_hm_hit_t *const hits = P.hits + base;
	const mm2amd_hm_opt_t &O = P.opt;

	// ---- sort
	int n = n_in;
	if (n_in <= 1) {
		if (lane < n_in) hm_make_reg(r[lane], (ref::Extra *)(exb + 32 * lane), hits[lane]), src[lane] = lane;
	} else {
		int live_cnt = 0;
		for (int i0 = 0; i0 < n_in; i0 += 64) {
			const int i = i0 + lane;
			bool live = false;
			if (i < n_in) { const mm2amd_hm_hit_t h = hits[i]; live = hm_live(h), keys[i] = hm_key(h, O.alt_drop), keep[i] = live ? 1 : 0; }
			live_cnt += __popcll(__ballot(live));
		}
		__syncthreads();
		bool tie = false;
		for (int i = lane; i < n_in; i += 64) {
			if (!keep[i]) continue;
			const uint64_t k = keys[i];
			int rank = 0;
			for (int j = 0; j < n_in; ++j) {
				if (!keep[j]) continue;
				const uint64_t kj = keys[j];
				rank += kj > k || (kj == k && j > i) ? 1 : 0;
				tie |= kj == k && j != i;
			}
			hm_make_reg(r[rank], (ref::Extra *)(exb + 32 * rank), hits[i]), src[rank] = i;
		}
		if (__ballot(tie) != 0 && live_cnt > kHmExactSortMax) {
			if (lane == 0) P.seg[s].n_kept = -1, P.seg[s].path = MM2AMD_HM_PATH_HOST;
			return;
		}
		n = live_cnt;
	}
	__syncthreads();

	// ---- parents (mm_set_parent)
	if (n > 0) {
		uint64_t *const cov = keys;
		const bool hard = (O.flags & MM2AMD_HM_HARD_MLEVEL) != 0;
		for (int i = lane; i < n; i += 64) r[i].id = i;
		if (lane == 0) prim[0] = 0, r[0].parent = 0;
		__syncthreads();
		int n_prim = 1;
		for (int i = 1; i < n; ++i) {
			const int si = r[i].qs, ei = r[i].qe;
			int uncov = 0;
			bool touches = hard;
			if (!hard) {
				for (int j = lane; j < n_prim; j += 64) cov[j] = hr_wave_clip(r[prim[j]], si, ei);
				__syncthreads();
				bool any = false;
				const int covered = hm_wave_sum(hr_wave_cov_part(cov, n_prim, lane, 64, &any));
				if (__ballot(any) != 0) touches = true, uncov = (ei - si) - covered;
			}
			int owner = -1;
			if (touches)
				for (int j0 = 0; j0 < n_prim; j0 += 64) {
					const int j = j0 + lane;
					const unsigned long long m = __ballot(j < n_prim && hr_wave_owns(r[prim[j < n_prim ? j : 0]], r[i], uncov, O.mask_level, O.mask_len));
					if (m) { owner = j0 + __ffsll((long long)m) - 1; break; }
				}
			if (lane == 0) {
				if (owner < 0) prim[n_prim] = i, r[i].parent = i, r[i].n_sub = 0;
				else hr_wave_commit(r[prim[owner]], r[i], O.sub_diff, O.alt_drop);
			}
			if (owner < 0) ++n_prim;
			__syncthreads();
		}
	}

	// ---- secondaries, compaction, renumbering, SAM primary (mm_select_sub, mm_set_sam_pri)
	int kept = n;
	if (!(O.flags & MM2AMD_HM_ALL_CHAINS)) {
		const bool select = O.pri_ratio > 0.0f && n > 0;
		if (select) {
			if (lane == 0) hr_select_secondaries(r, n, keep, O.pri_ratio, O.min_diff, O.best_n, (O.flags & MM2AMD_HM_CHECK_STRAND) != 0, O.min_strand_sc);
			__syncthreads();
			int w = 0;
			for (int i0 = 0; i0 < n; i0 += 64) {
				const int i = i0 + lane;
				uint4 t[5]; // a record is five 16-byte words, in registers
				int sv = 0;
				bool k = false;
				if (i < n) {
					const uint4 *const from = (const uint4 *)&r[i];
#pragma unroll
					for (int q = 0; q < 5; ++q) t[q] = from[q];
					sv = src[i], k = keep[i] != 0;
				}
				const unsigned long long m = __ballot(k);
				__syncthreads(); // (every lane has read its record before any lane writes one: the places are at or below the records read)
				if (k) {
					const int d = w + __popcll(m & ((1ull << lane) - 1));
					uint4 *const to = (uint4 *)&r[d];
#pragma unroll
					for (int q = 0; q < 5; ++q) to[q] = t[q];
					src[d] = sv;
				}
				w += __popcll(m);
				__syncthreads();
			}
			kept = w;
		}
		if (lane == 0) {
			if (kept != n) hr_renumber(r, kept, where, n);
			hr_mark_sam_primary(r, kept);
		}
		__syncthreads();
	}

	// ---- out
	for (int i = lane; i < n_in; i += 64) where[i] = -1;
	__syncthreads();
	for (int k = lane; k < kept; k += 64) where[src[k]] = k;
	__syncthreads();
	for (int i = lane; i < n_in; i += 64) {
		mm2amd_hm_out_t o;
		const int k = where[i];
		if (k >= 0) hm_make_out(o, r[k], k);
		else o.pos = -1, o.id = o.parent = o.subsc = o.n_sub = o.dp_max2 = 0, o.flags = 0, o.reserved = 0;
		P.out[base + (uint64_t)i] = o;
	}
	if (lane == 0) P.seg[s].n_kept = kept, P.seg[s].path = P.path;
}

void hits_merge_launch(const HitsMergeParams &P, void *stream)
{
	if (P.n_list <= 0) return;
	hipLaunchKernelGGL(hits_merge_kernel, dim3(P.n_list), dim3(64), (size_t)kHmBytesPerHit * (size_t)P.cap, (hipStream_t)stream, P);
	HIP_CHECK(hipGetLastError());
}

} // namespace mm2amd
