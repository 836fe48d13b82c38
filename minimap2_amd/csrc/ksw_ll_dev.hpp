// ksw_ll_kernel: the local (Smith-Waterman) score with end coordinates of ksw_ll_qinit + ksw_ll_i16 (ksw2_ll_sse.c:37-152) for jobs of the plain
// class (ksw_ll.hpp), from the plain affine recurrence -- DESIGN.md section 3c has the argument.  Compiled with region_finish.hip.
//
// Lanes lie across the query: a lane owns kLlCols consecutive columns, a wavefront a strip of kLlStrip.  The sweep over the target rows is skewed:
// in step r lane l computes row r - l, so that its left neighbour's last column of that row is one step old and arrives by one DPP move.  Lane 63's
// last column is the strip's boundary column, (H, F) per row in one word; the next strip's lane 0 reads it.  Nothing is loaded or stored per step:
// the target's codes and the boundary column come in blocks of kLlBlock rows, one row per lane, read one block ahead and handed to lane 0 by a
// rotation (wave_shl) a step; lane 63's column is collected the same way and stored a block at a time.
//
// One template, two launch classes.  NW == 1 (wave): a wavefront per job, strips one after the other, the boundary column in place in the job's
// work buffer.  NW == kLlWgWaves (wg): a workgroup per job; wave w owns strips w, w + NW, ... and starts kLlLagBlocks blocks of steps after wave
// w - 1; all waves meet at a block barrier after every block, which is the only ordering between them.  Strip j's boundary goes to buffer j % NW.
//   written: the rows of strip j's local block b (rows 64b - 63 .. 64b) at the end of that block;
//   read:    the rows 64b .. 64b + 63 by strip j + 1 at the start of ITS local block b - 1 (block 0: at its start), written by strip j's blocks b, b + 1.
// Strip j + 1 starts at least 3 blocks after strip j (the period of a round is at least NW * 3 blocks, so this holds from a round's last strip to the
// next round's first as well), hence its local block b - 1 begins after the barrier that ends strip j's block b + 1.  The buffer's next writer, strip
// j + NW, starts a period after strip j, i.e. no earlier than strip j + 1: it stores rows <= 64b at the end of a block that begins after that read.
#pragma once
#include <hip/hip_runtime.h>
#include "hip_util.hpp"
#include "ksw_ll.hpp"

namespace mm2amd {

__device__ __forceinline__ uint32_t ll_shr1(uint32_t head_in, uint32_t v) // lane i <- v[i - 1], lane 0 <- its own head_in
{
	return (uint32_t)__builtin_amdgcn_update_dpp((int)head_in, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t ll_shl1(uint32_t tail_in, uint32_t v) // lane i <- v[i + 1], lane 63 <- its own tail_in
{
	return (uint32_t)__builtin_amdgcn_update_dpp((int)tail_in, (int)v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ int ll_max3(int a, int b, int c) { const int m = a > b ? a : b; return m > c ? m : c; } // v_max3_i32

template <int NW>
__global__ __launch_bounds__(64 * NW) void ksw_ll_kernel(LlParams P)
{
	constexpr int K = kLlCols;
	__shared__ unsigned long long s_best[NW];
	const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
	const LlJob J = P.jobs[blockIdx.x];
	const int qlen = J.qlen, tlen = J.tlen;
	const uint8_t *const q = P.qpool + J.q_off, *const t = P.tpool + J.t_off;
	const bool qrev = (J.flag & kLlQRev) != 0, qcomp = (J.flag & kLlQComp) != 0, trev = (J.flag & kLlTRev) != 0;
	const int slen = (qlen + 7) >> 3;
	const int n_strips = (qlen + kLlStrip - 1) / kLlStrip;
	const int LB = (tlen + 63 + kLlBlock - 1) / kLlBlock;                               // blocks of steps a strip takes: rows 0 .. tlen - 1 in lanes 0 .. 63
	const int PB = NW == 1 ? LB : (LB > NW * kLlLagBlocks ? LB : NW * kLlLagBlocks);    // blocks from a wave's strip to its next one
	const int total = (n_strips - 1) / NW * PB + (n_strips - 1) % NW * kLlLagBlocks + LB; // ... until the last strip ends
	const size_t bw = ll_bnd_words(tlen);
	uint32_t *const bnd_out = P.bnd + J.bnd_off + (size_t)w * bw;
	const uint32_t *const bnd_in = P.bnd + J.bnd_off + (size_t)((w + NW - 1) % NW) * bw;
	const int goe = P.goe, ge = P.ge;
	auto tcode = [&](int row) -> uint32_t { return row < tlen ? (uint32_t)t[trev ? tlen - 1 - row : row] : 0u; };

	unsigned long long best = 0; // over the lane's columns of the strips done: key << 32 | the column's place in the striped scan
	int Hp[K], E[K], shi[K];     // per column: H of the row above, E into this row; the scores against target codes 0..3 (slo) and 4 (shi)
	uint32_t slo[K], key[K];
	int hdiag = 0;               // H(row - 1) of the left neighbour's last column
	uint32_t out = 0;            // (H << 16 | F) of the lane's last column in the row it has just computed
	uint32_t tcur = 0;           // the target code of the lane's row
	uint32_t bin = 0, bnext = 0, tblk = 0, tnext = 0, bout = 0;
#pragma unroll
	for (int c = 0; c < K; ++c) Hp[c] = E[c] = shi[c] = 0, slo[c] = key[c] = 0;

	for (int g = 0; g < total; ++g) {
		const int gg = g - w * kLlLagBlocks;
		const int b = gg >= 0 ? gg % PB : LB, strip = gg >= 0 ? gg / PB * NW + w : n_strips; // (uniform over the wave)
		if (b < LB && strip < n_strips) {
			const int p0 = strip * kLlStrip + lane * K;
			const bool has_left = strip > 0, has_right = strip + 1 < n_strips;
			if (b == 0) {
#pragma unroll
				for (int c = 0; c < K; ++c) {
					const int p = p0 + c;
					uint32_t lo = 0;
					int hi = 0;
					if (p < qlen) {
						int qc = q[qrev ? qlen - 1 - p : p];
						if (qcomp) qc = qc < 4 ? 3 - qc : 4;
						lo = qc == 0 ? P.sc_lo[0] : qc == 1 ? P.sc_lo[1] : qc == 2 ? P.sc_lo[2] : qc == 3 ? P.sc_lo[3] : P.sc_lo[4];
						hi = qc == 0 ? P.sc_hi[0] : qc == 1 ? P.sc_hi[1] : qc == 2 ? P.sc_hi[2] : qc == 3 ? P.sc_hi[3] : P.sc_hi[4];
					}
					slo[c] = lo, shi[c] = hi, Hp[c] = E[c] = 0, key[c] = 0;
				}
				hdiag = 0, out = 0, tcur = 0, bout = 0;
				bin = has_left ? bnd_in[lane] : 0u;
				tblk = tcode(lane);
				// these are needed at once; the block ahead, requested below, only 64 steps from here: have nothing pending, so that the steps wait for nothing
				__builtin_amdgcn_s_waitcnt(0);
			} else bin = bnext, tblk = tnext;
			if (b + 1 < LB) { // the next block's rows: needed 64 steps from here
				const int row = (b + 1) * kLlBlock + lane;
				bnext = has_left ? bnd_in[row] : 0u;
				tnext = tcode(row);
			}
			for (int s = 0; s < kLlBlock; ++s) {
				const int i = b * kLlBlock + s - lane;          // the lane's row in this step
				const uint32_t in = ll_shr1(bin, out);          // the left neighbour's last column of row i; lane 0: the boundary column's
				tcur = ll_shr1(tblk, tcur);                     // the code of row i moves along with the row
				bin = ll_shl1(bin, bin), tblk = ll_shl1(tblk, tblk);
				if ((unsigned)i < (unsigned)tlen) {
					int hl = (int)(in >> 16), fl = (int)(in & 0xffffu), d = hdiag;
					hdiag = hl;
					const uint32_t tsh = (tcur & 3u) << 3;
					const bool t4 = tcur >= 4u;
#pragma unroll
					for (int c = 0; c < K; ++c) {
						int sc = (int)(int8_t)(slo[c] >> tsh);
						sc = t4 ? shi[c] : sc;
						const int e = ll_max3(E[c] - ge, Hp[c] - goe, 0);
						const int f = ll_max3(fl - ge, hl - goe, 0);
						const int h = ll_max3(d + sc, e, f);
						d = Hp[c], Hp[c] = h, E[c] = e, hl = h, fl = f;
						const uint32_t k = (uint32_t)h << 16 | (uint32_t)i;
						key[c] = key[c] > k ? key[c] : k;
					}
					out = (uint32_t)hl << 16 | (uint32_t)fl;
				}
				bout = ll_shl1(out, bout);                      // lane 63's column, a row a step
			}
			if (has_right) { // lane j holds what lane 63 computed in the block's step j: row 64b + j - 63
				const int row = b * kLlBlock - 63 + lane;
				if ((unsigned)row < (unsigned)tlen) bnd_out[row] = bout;
			}
			if (b == LB - 1) {
#pragma unroll
				for (int c = 0; c < K; ++c) {
					const int p = p0 + c;
					if (p < qlen) {
						const unsigned long long v = (unsigned long long)key[c] << 32 | (unsigned)(p % slen * 8 + p / slen);
						best = best > v ? best : v;
					}
				}
			}
		}
		__syncthreads();
	}

#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) {
		const unsigned long long o = __shfl_xor(best, m, 64);
		best = best > o ? best : o;
	}
	if (lane == 0) s_best[w] = best;
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int k = 1; k < NW; ++k) best = best > s_best[k] ? best : s_best[k];
		const uint32_t top = (uint32_t)(best >> 32), ord = (uint32_t)best;
		LlRes r;
		r.score = (int32_t)(top >> 16), r.te = (int32_t)(top & 0xffffu), r.pad = 0;
		// nothing scores: the striped scan's last slot holds the "maximum" too, padding included (ksw2_ll_sse.c:149-151); every key is then 0 << 16 | tlen - 1
		r.qe = r.score == 0 ? 8 * slen - 1 : (int32_t)((ord >> 3) + (ord & 7u) * (uint32_t)slen);
		P.res[J.out] = r;
	}
}

void ksw_ll_launch(const LlParams &P, void *stream)
{
	if (P.n_jobs <= 0) return;
	if (P.n_waves == 1) hipLaunchKernelGGL(ksw_ll_kernel<1>, dim3(P.n_jobs), dim3(64), 0, (hipStream_t)stream, P);
	else if (P.n_waves == kLlWgWaves) hipLaunchKernelGGL(ksw_ll_kernel<kLlWgWaves>, dim3(P.n_jobs), dim3(64 * kLlWgWaves), 0, (hipStream_t)stream, P);
	else throw HipError("[mm2amd] ksw_ll_launch: no kernel for this number of waves");
	HIP_CHECK(hipGetLastError());
}

} // namespace mm2amd
