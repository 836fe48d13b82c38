// cigar_eqx_kernel: see cigar_eqx.hpp.  Included by region_finish.hip (one translation unit with the kernel whose output it reads).
//
// One wavefront per region, the operations cut into 64 stretches as in stage C of region_finish_kernel: a lane first adds up what its operations
// consume (a wave scan tells it where its first one starts in the two sequences), then walks the columns of its matches and counts the stretches --
// one more wherever equality flips inside a match; stretches never join across operations, so the lanes need nothing from each other but the sum.
//   [count]  the sum is the region's =/X length.  It equals the incoming length exactly when no match splits: the reference's in-place verdict.
//   [write]  an in-place region is copied with M relabelled = (no column is read).  Otherwise the lanes count again, a wave scan of the counts
//            tells every lane where its first operation goes, and a second walk stores them.
// The sequences are read as stage C reads them: query codes at q_pos + qshift in the byte pool, target codes at t_pos + tshift in the packed
// reference, an aligned 8-byte block / 8-code word at a time.
#pragma once
#include <hip/hip_runtime.h>
#include "hip_util.hpp"
#include "cigar_eqx.hpp"

namespace mm2amd {

namespace {
struct EqxColumns { // the two sequences of a region; the blocks read last are kept
	const uint8_t *qpool;
	const uint32_t *S;
	uint64_t q_pos, t_pos; // of column offsets 0 / 0: the region's start plus mm_fix_cigar's shifts
	int64_t qblk = -4, tblk = -4;
	uint64_t qw = 0;
	uint32_t tw = 0;
	__device__ __forceinline__ bool equal(uint32_t qoff, uint32_t toff)
	{
		const uint64_t a = q_pos + qoff, o = t_pos + toff;
		if ((int64_t)(a >> 3) != qblk) qblk = (int64_t)(a >> 3), qw = *(const uint64_t *)(qpool + (a & ~7ull));
		if ((int64_t)(o >> 3) != tblk) tblk = (int64_t)(o >> 3), tw = S[o >> 3];
		return (uint32_t)(qw >> ((a & 7) << 3) & 0xff) == (tw >> ((o & 7) << 2) & 0xf); // N against N (4 == 4) is equal (align.c:193)
	}
};
__device__ __forceinline__ uint32_t eqx_scan_add(uint32_t v, int lane) // inclusive prefix sum over the wave
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(v, (unsigned)d, 64); if (lane >= d) v += t; }
	return v;
}
// operations [k0, k1) of cg, the first one starting at qoff / toff: emit(word) for every operation of the =/X CIGAR, in order.  Flat -- one column or
// one operation per step -- because the lanes' run lengths differ.
template <class Emit>
__device__ __forceinline__ void eqx_walk(const uint32_t *cg, uint32_t k0, uint32_t k1, uint32_t qoff, uint32_t toff, EqxColumns &C, Emit emit)
{
	uint32_t k = k0, rem = 0, run = 0;
	bool prev = false;
	for (;;) {
		if (rem == 0) {
			if (k >= k1) break;
			const uint32_t c = cg[k++], op = c & 0xf, len = c >> 4;
			if (op == 0) {
				if (len == 0) continue; // (an empty match has no stretch: align.c:192)
				prev = C.equal(qoff, toff), run = 1, rem = len - 1;
				++qoff, ++toff;
				if (rem == 0) emit(run << 4 | (prev ? 7u : 8u));
			} else {
				emit(c);
				if (op == 1) qoff += len;
				else if (op == 2 || op == 3) toff += len;
			}
			continue;
		}
		const bool e = C.equal(qoff, toff);
		++qoff, ++toff, --rem;
		if (e != prev) emit(run << 4 | (prev ? 7u : 8u)), run = 1, prev = e;
		else ++run;
		if (rem == 0) emit(run << 4 | (prev ? 7u : 8u));
	}
}
} // namespace

template <bool WRITE>
__global__ void __launch_bounds__(64) cigar_eqx_kernel(EqxParams P)
{
	const int lane = (int)threadIdx.x;
	const int id = (int)blockIdx.x;
	const FinResult F = P.results[id];
	const uint32_t n = F.n_cigar > 0 ? (uint32_t)F.n_cigar : 0u; // the same in every lane, like everything up to the scan
	if (n == 0) { // an empty region, or one whose CIGAR does not cover its windows (the host throws)
		if (!WRITE && lane == 0) P.n_ops[id] = 0;
		return;
	}
	const FinRegion R = P.regions[id];
	const uint32_t *const cg = P.fin_pool + R.out_off;
	uint32_t n_out = 0;
	uint32_t *out = nullptr;
	if (WRITE) {
		n_out = P.n_ops[id], out = P.out_pool + P.out_off[id];
		if (n_out == n) { // no match splits (n_EQX == n_M, align.c:209-215): every M becomes =, whatever its columns hold
			for (uint32_t k = (uint32_t)lane; k < n; k += 64) { const uint32_t c = cg[k]; out[k] = (c & 0xf) == 0 ? (c | 7u) : c; }
			return;
		}
	}
	const uint32_t per = (n + 63u) / 64u;
	const uint32_t k0 = (uint32_t)lane * per < n ? (uint32_t)lane * per : n, k1 = k0 + per < n ? k0 + per : n;
	uint32_t dq = 0, dt = 0;
	for (uint32_t k = k0; k < k1; ++k) {
		const uint32_t c = cg[k], op = c & 0xf, len = c >> 4;
		if (op == 0) dq += len, dt += len;
		else if (op == 1) dq += len;
		else if (op == 2 || op == 3) dt += len;
	}
	const uint32_t qoff = eqx_scan_add(dq, lane) - dq, toff = eqx_scan_add(dt, lane) - dt;
	EqxColumns C;
	C.qpool = P.qpool, C.S = P.S, C.q_pos = R.q_pos + (uint64_t)(int64_t)F.qshift, C.t_pos = R.t_pos + (uint64_t)(int64_t)F.tshift;
	uint32_t cnt = 0;
	eqx_walk(cg, k0, k1, qoff, toff, C, [&](uint32_t) { ++cnt; });
	const uint32_t incl = eqx_scan_add(cnt, lane);
	if (!WRITE) {
		if (lane == 63) P.n_ops[id] = incl;
		return;
	}
	uint32_t w = incl - cnt;
	eqx_walk(cg, k0, k1, qoff, toff, C, [&](uint32_t word) { if (w < n_out) out[w] = word; ++w; }); // (w < n_out: both passes count the same columns; the pool's bound holds regardless)
}

void cigar_eqx_launch(const EqxParams &P, bool write, void *stream)
{
	if (P.n_regions <= 0) return;
	if (write) hipLaunchKernelGGL(cigar_eqx_kernel<true>, dim3(P.n_regions), dim3(64), 0, (hipStream_t)stream, P);
	else hipLaunchKernelGGL(cigar_eqx_kernel<false>, dim3(P.n_regions), dim3(64), 0, (hipStream_t)stream, P);
	HIP_CHECK(hipGetLastError());
}

} // namespace mm2amd
