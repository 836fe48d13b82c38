// sdust_kernel: sdust() (sdust.h / sdust.c:134-175 with W = 64, as mm_dust_minier passes it, map.c:41) for a batch of reads, one wavefront per
// read.  Compiled with seed_chain.hip; DESIGN.md section 3e derives the formulation from the reference's automaton and lists every loop's bound.
//
// The window is a FIFO of at most 62 3-mer codes: lane k holds w[k] and e[k], the number of later words equal to w[k] (one dword, one DPP move
// per pop).  A push adds 1 to e[k] wherever w[k] is the new word; rw (the sum of e) and L (n - 1 - the last k with (e[k] + 1) * 10 > 2T) follow
// from a ballot each.  Only when rw * 10 > L * T do the lanes act as the candidates of find_perfect: candidate i has r = sum of e[k >= i]
// and l = n - i - 1.  The list P of perfect intervals is packed dwords in LDS, in the reference's order (start descending, then by insertion):
//   bits 0-5 start mod 64, bits 6-11 l, bits 12-28 the ratio r / l as floor(4096 r / l).
// finish = start + l + 3; every live start lies in [window start, window start + 64), so six bits recover it.  Two different fractions with
// denominators <= 61 differ by at least 1 / 3721 > 1 / 4096 and r / l <= 31, so the 17-bit key orders the ratios exactly and ties stay ties:
// every comparison the reference makes between (r, l) pairs (sdust.c:122,126) is one between keys.
// A step's insertions are one merge: candidate i goes behind the old entries with start >= its own and behind the inserted candidates above it;
// an old entry with offset o moves right by the number of inserted candidates above o.
//
// No loop waits on another wavefront, and every trip count is fixed before the loop is entered (a uniform break only shortens it):
//   blocks of steps (len + 64) / 64, steps of a block <= 64 (len + 1 in all); list passes <= (cap + 63) / 64; the flush at an N or the end <= 64.
#pragma once
#include <hip/hip_runtime.h>
#include "hip_util.hpp"
#include "sdust.hpp"

namespace mm2amd {

#define SDUST_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

__device__ __forceinline__ uint32_t sd_shl1(uint32_t tail_in, uint32_t v) // lane i <- v[i + 1], lane 63 <- its own tail_in
{
	return (uint32_t)__builtin_amdgcn_update_dpp((int)tail_in, (int)v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t sd_suffix_sum(uint32_t v, int lane) // the sum over the lanes >= this one
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_down(v, (unsigned)d, 64); if (lane + d < 64) v += o; }
	return v;
}
__device__ __forceinline__ uint32_t sd_suffix_max(uint32_t v, int lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_down(v, (unsigned)d, 64); if (lane + d < 64 && o > v) v = o; }
	return v;
}

// one read; lds: 64 bucket keys | 64 bucket counts | cap list entries.  Returns false when the list would outgrow cap: reg_n is not written then
// (the regions closed so far are in reg_s / reg_e; the wide class, which scans the read again, rewrites them).
__device__ inline bool sdust_scan_wave(const SdustParams &P, const uint8_t *seq, const int len, const uint64_t slot, uint32_t *const lds, int *stopped_at)
{
	uint32_t *const bkey = lds, *const bcnt = lds + 64, *const list = lds + 128;
	const int lane = (int)(threadIdx.x & 63u);
	const int cap = P.cap, T = P.T, T2 = P.T << 1, max_pass = (cap + 63) >> 6;
	uint32_t we = 0xffu;               // e << 8 | w; a lane outside the window holds the word 0xff, which equals no code, and e = 0
	int n = 0, rw = 0;                 // the window's length and the sum of e
	int nP = 0, tail_start = 0;        // the list's length and its last entry's start (the smallest)
	int wstart = 0;                    // every live entry's start is in [wstart, wstart + 64)
	int l = 0;                         // bases since the last N
	uint32_t t = 0;
	int last_s = 0, last_f = -1;       // the last masked region (it may still grow)
	uint32_t n_reg = 0;
	bool ok = true;

	auto entry_start = [&](uint32_t v) { return wstart + (int)((v - (uint32_t)wstart) & 63u); };
	auto emit = [&]() {
		if (lane == 0 && n_reg < (uint32_t)len) P.reg_s[slot + n_reg] = (uint32_t)last_s, P.reg_e[slot + n_reg] = (uint32_t)last_f;
		++n_reg;
	};
	// save_masked_regions (sdust.c:92-108) for nP > 0 and tail_start < S: the last entry extends or starts a region; the entries below S leave
	auto save = [&](int S) {
		const uint32_t tv = list[nP - 1];
		const int ps = tail_start, pf = ps + (int)(tv >> 6 & 63u) + 3;
		if (last_f >= 0 && ps <= last_f) { if (pf > last_f) last_f = pf; }
		else { if (last_f >= 0) emit(); last_s = ps, last_f = pf; }
		for (int pass = 0; pass < max_pass; ++pass) { // they are the list's tail: 64 entries a pass
			const int idx = nP - 1 - lane;
			const bool ex = idx >= 0 && entry_start(list[idx]) < S;
			const int c = __popcll(__ballot(ex));
			nP -= c;
			if (c < 64) break;
		}
		if (nP > 0) tail_start = entry_start(list[nP - 1]);
	};
	// find_perfect (sdust.c:110-135) for the window start `start`; false: the list would outgrow cap
	auto find = [&](int start, int L) -> bool {
		const uint32_t R = sd_suffix_sum(we >> 8, lane);
		const int nl = n - lane - 1;
		const bool pass = lane < n - L && (int)R * 10 > T * nl; // (nl > 0 here: the window's last word has R = 0)
		if (__ballot(pass) == 0) return true;
		const uint32_t kc = pass ? (R << 12) / (uint32_t)nl : 0u;
		// per start offset: the largest ratio and the number of the old entries
		bkey[lane] = 0, bcnt[lane] = 0;
		SDUST_SYNC();
		const int n_chunk = (nP + 63) >> 6;
		for (int c = 0; c < n_chunk; ++c) {
			const int idx = c * 64 + lane;
			if (idx < nP) {
				const uint32_t v = list[idx], o6 = (v - (uint32_t)start) & 63u;
				atomicMax(&bkey[o6], v >> 12);
				atomicAdd(&bcnt[o6], 1u);
			}
		}
		SDUST_SYNC();
		// candidate i is inserted iff its ratio is >= those of the old entries with offset >= i and of the passing candidates above i
		uint32_t x = bkey[lane];
		const uint32_t above = __shfl_down(kc, 1u, 64); // (lanes 62 and 63 are never candidates: their kc is 0)
		if (lane < 63 && above > x) x = above;
		const uint32_t M = sd_suffix_max(x, lane);
		const uint32_t J = sd_suffix_sum(bcnt[lane], lane); // the old entries with start >= this candidate's: its place among them
		const bool ins = pass && kc >= M;
		const unsigned long long im = __ballot(ins);
		const int n_ins = __popcll(im);
		if (n_ins == 0) return true;
		if (nP + n_ins > cap) return false;
		for (int c = n_chunk - 1; c >= 0; --c) { // the old entries move right, the last chunk first: by less than 64, into places already vacated
			const int idx = c * 64 + lane;
			uint32_t v = 0;
			if (idx < nP) v = list[idx];
			SDUST_SYNC();
			if (idx < nP) {
				const int sh = __popcll((im >> ((v - (uint32_t)start) & 63u)) >> 1);
				if (sh) list[idx + sh] = v;
			}
			SDUST_SYNC();
		}
		if (ins) list[J + (uint32_t)__popcll((im >> lane) >> 1)] = ((uint32_t)(start + lane) & 63u) | (uint32_t)nl << 6 | kc << 12;
		const int lowest = start + __ffsll((long long)im) - 1;
		tail_start = nP > 0 && tail_start < lowest ? tail_start : lowest;
		nP += n_ins;
		SDUST_SYNC();
		return true;
	};

	const int steps = len + 1, n_blk = (steps + 63) >> 6; // position len is the end: it flushes like an N
	uint32_t cur = lane < len ? seq[lane] : 4u;
	for (int blk = 0; blk < n_blk && ok; ++blk) {
		const int i0 = blk << 6;
		uint32_t nxt = 4u; // the next block's bases, one per lane, asked for a block ahead
		if (blk + 1 < n_blk) { const int p = i0 + 64 + lane; if (p < len) nxt = seq[p]; }
		const int ns = steps - i0 < 64 ? steps - i0 : 64;
		for (int s = 0; s < ns; ++s) {
			const int i = i0 + s;
			const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)cur, s);
			if (b < 4u) {
				++l, t = (t << 2 | b) & 63u;
				if (l < 3) continue;
				const int start = (l > 64 ? l - 64 : 0) + (i + 1 - l);
				if (nP > 0 && tail_start < start) save(start);
				wstart = start;
				// shift_window (sdust.c:70-90)
				if (n >= 62) {
					rw -= (int)((uint32_t)__builtin_amdgcn_readfirstlane((int)we) >> 8);
					we = sd_shl1(0xffu, we), --n;
				}
				const bool eq = (we & 0xffu) == t;
				rw += __popcll(__ballot(eq));
				if (eq) we += 0x100u;
				if (lane == n) we = t;
				++n;
				const unsigned long long bad = __ballot(lane < n && (int)((we >> 8) + 1u) * 10 > T2);
				const int L = bad ? n - 64 + __clzll((long long)bad) : n; // n - 1 - (the highest lane of bad)
				if (rw * 10 > L * T && !find(start, L)) { ok = false; *stopped_at = i + 1; break; }
			} else { // an N or the end: `while (P.n) save_masked_regions(start++)` (sdust.c:157-159); the window itself is not cleared
				int S = (l > 63 ? l - 63 : 0) + (i + 1 - l);
				for (int it = 0; it < 64; ++it) { // one group of equal starts leaves per trip (the first may take two), and there are at most 64
					if (nP == 0) break;
					if (tail_start >= S) S = tail_start + 1;
					save(S);
					++S;
				}
				nP = 0;
				l = 0, t = 0;
			}
		}
		cur = nxt;
	}
	if (!ok) return false;
	if (last_f >= 0) emit();
	if (lane == 0) P.reg_n[slot] = n_reg;
	return true;
}

__global__ __launch_bounds__(64) void sdust_kernel(SdustParams P)
{
	MM2_DYN_LDS(uint32_t, sdust_lds);
	const int lane = (int)(threadIdx.x & 63u);
	const uint32_t n_jobs = P.wide == 1 ? (P.cnt->n_wide < (uint32_t)P.n_reads ? P.cnt->n_wide : (uint32_t)P.n_reads) : (uint32_t)P.n_reads;
	for (uint32_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
		const uint32_t r = P.wide == 1 ? P.wide_list[job] : job;
		if (r >= (uint32_t)P.n_reads) continue;
		const uint64_t o = P.off[r];
		const int len = (int)(P.off[r + 1] - o);
		if (len <= 0) continue; // (an empty read shares its slot with the next one and has no regions)
		int stopped_at = 0;
		const bool ok = sdust_scan_wave(P, P.codes + (uint64_t)P.code_mul * o, len, o, sdust_lds, &stopped_at);
		if (lane == 0) {
			if (P.wide) {
				atomicAdd(&P.cnt->wide_bases, (unsigned long long)len);
				if (!ok) P.reg_n[o] = 0, atomicOr(&P.cnt->err, 1u);
			} else if (!ok) {
				P.wide_list[atomicAdd(&P.cnt->n_wide, 1u)] = r;
				atomicAdd(&P.cnt->narrow_partial, (unsigned long long)stopped_at);
			}
		}
		SDUST_SYNC(); // the next read's list starts from scratch, after this one's last accesses
	}
}

__global__ __launch_bounds__(256) void sdust_count_kernel(SdustParams P, uint32_t *cnt_out)
{
	const int r = (int)(blockIdx.x * 256 + threadIdx.x);
	if (r < P.n_reads) cnt_out[r] = P.off[r + 1] > P.off[r] ? P.reg_n[P.off[r]] : 0u;
}

__global__ __launch_bounds__(64) void sdust_pack_kernel(SdustParams P, const uint64_t *out_off, uint64_t *out)
{
	const int r = (int)blockIdx.x;
	const uint64_t o = P.off[r];
	if (P.off[r + 1] <= o) return;
	const uint32_t n = P.reg_n[o];
	for (uint32_t k = threadIdx.x; k < n; k += 64) out[out_off[r] + k] = (uint64_t)P.reg_s[o + k] << 32 | P.reg_e[o + k];
}

size_t sdust_lds_bytes(int cap) { return (size_t)(128 + cap) * 4; }

void sdust_launch(const SdustParams &P, int grid, void *stream)
{
	if (P.n_reads <= 0) return;
	if (P.cap < 1 || P.cap > kSdustWideCap) throw HipError("[mm2amd] sdust_launch: the list capacity must be in [1, 4096]");
	if (P.wide != 1) grid = P.n_reads;
	else if (grid <= 0) grid = P.n_reads < kSdustWideGrid ? P.n_reads : kSdustWideGrid;
	hipLaunchKernelGGL(sdust_kernel, dim3(grid), dim3(64), sdust_lds_bytes(P.cap), (hipStream_t)stream, P);
	HIP_CHECK(hipGetLastError());
}

void sdust_count_launch(const SdustParams &P, uint32_t *cnt_out, void *stream)
{
	if (P.n_reads <= 0) return;
	hipLaunchKernelGGL(sdust_count_kernel, dim3((P.n_reads + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, cnt_out);
	HIP_CHECK(hipGetLastError());
}

void sdust_pack_launch(const SdustParams &P, const uint64_t *out_off, uint64_t *out, void *stream)
{
	if (P.n_reads <= 0) return;
	hipLaunchKernelGGL(sdust_pack_kernel, dim3(P.n_reads), dim3(64), 0, (hipStream_t)stream, P, out_off, out);
	HIP_CHECK(hipGetLastError());
}

} // namespace mm2amd
