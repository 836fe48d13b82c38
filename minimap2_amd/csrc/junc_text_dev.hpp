// junc_text_kernel: see junc_text.hpp.  One wavefront per printable hit.
//   walk     64 operations a step: every lane takes the target advance of its operation (M, =, X, D and N; I, S, H and the rest stand still), a
//            wave inclusive sum with a carry across the steps gives every operation its t_off (32 bits: the sizing pass has checked with 64-bit
//            sums that the advances add up to re - rs);
//   introns  a ballot marks the N lanes.  Each reads its four nibbles of the packed S one by one (a dinucleotide may straddle a word, a sequence
//            starts at any nibble) and forms the score in registers: donor GT 3, GC 2, AT 1, acceptor AG 3, AC 1; on the minus strand of the
//            transcript the two ends swap and are reverse-complemented (revcomp_splice: N stays N);
//   lines    the wave runs over the set ballot bits -- the loop is wave-uniform, every cross-lane operation runs with all 64 lanes -- and per
//            bit writes  tname \t t_off \t t_off+len \t qname \t score \t +|-  with rec_text_dev.hpp's pieces: the names 16 bytes per lane and
//            step, the numbers on lane 0 with the values broadcast from the owning lane.
// Sizing and writing are this one function on a counting and on a storing sink.
#pragma once
#include "rec_text_dev.hpp"
#include "junc_text.hpp"

namespace mm2amd {

namespace {

// The sizing pass's judgement (the same in every lane): what mm_write_junc asserts (an intron of at least 2 bases, the walk ends at re), and no
// operation code beyond the ten of "MIDNSHP=XB".
__device__ __forceinline__ bool junc_bad_ops(const uint32_t *cg, uint32_t n, int32_t rs, int32_t re, int lane)
{
	bool bad = rs < 0 || re < rs;
	unsigned long long st = 0;
	for (uint32_t k = (uint32_t)lane; k < n; k += 64u) {
		const uint32_t w = cg[k], op = w & 0xf, len = w >> 4;
		bad |= op > 9u || (op == 3u && len < 2u);
		if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) st += len;
	}
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) st += __shfl_xor(st, d, 64);
	bad |= st != (unsigned long long)((long long)re - (long long)rs);
	return __ballot(bad) != 0ull;
}

__device__ __forceinline__ uint32_t junc_nibble(const uint32_t *S, uint64_t o)
{
	const uint32_t c = S[o >> 3] >> ((o & 7) << 2) & 0xf;
	return c > 4u ? 4u : c;
}
__device__ __forceinline__ uint32_t junc_comp(uint32_t c) { return c < 4u ? 3u - c : 4u; }

} // namespace

template <bool WRITE>
__global__ void __launch_bounds__(64) junc_text_kernel(RecParams P)
{
	__shared__ uint32_t s_stage[(64 * kTxtColBytes + 4 + 3) / 4 + 1];
	const int lane = (int)threadIdx.x;
	const int id = (int)blockIdx.x;
	const RecJob J = P.jobs[id];
	const RecHit H = P.hits[J.hit];
	const uint32_t n = H.n_cigar;
	const uint32_t *cg = P.cigar + H.cig_off;

	if (WRITE) { // the sizing pass has judged the hit
		const RecRes r = P.res[id];
		if (r.status != kRecOk || r.len == 0) return;
	} else if (junc_bad_ops(cg, n, H.rs, H.re, lane)) {
		if (lane == 0) { RecRes r; r.len = r.before = 0, r.status = kRecBadCigar, r.reserved = 0; P.res[id] = r; }
		return;
	}
	const bool rev = ((H.bits >> kRecTransShift & 3u) == 2u) != ((H.bits & kRecRev) != 0); // (trans_strand == 2) ^ r->rev
	const bool lines = (P.flag & kJuncLines) != 0;
	const char *tname = P.tnames + P.tname_off[H.rid], *qname = P.names + J.name_off;
	const uint32_t tname_len = (uint32_t)(P.tname_off[H.rid + 1] - P.tname_off[H.rid]);

	TxtOut<WRITE> O;
	O.out = WRITE ? P.out + P.off[id] : nullptr, O.stage = s_stage, O.lane = lane, O.nbytes = 0;
	uint32_t t_carry = (uint32_t)H.rs;
	for (uint32_t k0 = 0; k0 < n; k0 += 64u) {
		const uint32_t k = k0 + (uint32_t)lane;
		const uint32_t w = k < n ? cg[k] : 0u, op = w & 0xf, len = w >> 4;
		const bool intron = k < n && op == 3u;
		const uint32_t adv = k < n && (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) ? len : 0u;
		const uint32_t incl = wave_inclusive_sum(adv, lane);
		const uint32_t t_off = t_carry + incl - adv;
		t_carry += (uint32_t)__shfl((int)incl, 63, 64);
		uint32_t score = 0;
		if (intron) { // [t_off, t_off + len) lies inside [rs, re), and len >= 2
			const uint64_t o = H.t_pos + t_off;
			uint32_t d0 = junc_nibble(P.S, o), d1 = junc_nibble(P.S, o + 1), a0 = junc_nibble(P.S, o + len - 2), a1 = junc_nibble(P.S, o + len - 1);
			if (rev) {
				const uint32_t x0 = junc_comp(a1), x1 = junc_comp(a0), y0 = junc_comp(d1), y1 = junc_comp(d0);
				d0 = x0, d1 = x1, a0 = y0, a1 = y1;
			}
			score = (d0 == 2u && d1 == 3u ? 3u : d0 == 2u && d1 == 1u ? 2u : d0 == 0u && d1 == 3u ? 1u : 0u) + (a0 == 0u && a1 == 2u ? 3u : a0 == 0u && a1 == 1u ? 1u : 0u);
		}
		for (unsigned long long m = __ballot(intron); m; m &= m - 1ull) { // (the same in every lane)
			const int b = __ffsll((long long)m) - 1;
			const uint32_t st = (uint32_t)__shfl((int)t_off, b, 64), en = st + (uint32_t)__shfl((int)len, b, 64), sc = (uint32_t)__shfl((int)score, b, 64);
			if (!lines && O.nbytes > 0) rec_small(O, [&](auto &o) { o.ch('\n'); });
			rec_bytes(O, tname, tname_len);
			rec_small(O, [&](auto &o) { o.ch('\t'), o.num(st), o.ch('\t'), o.num(en), o.ch('\t'); });
			rec_bytes(O, qname, J.name_len);
			rec_small(O, [&](auto &o) {
				o.ch('\t'), o.num(sc), o.ch('\t'), o.ch(rev ? '-' : '+');
				if (lines) o.ch('\n');
			});
		}
	}
	if (!WRITE && lane == 0) {
		RecRes r;
		r.len = (uint32_t)O.nbytes, r.before = (uint32_t)O.nbytes, r.status = O.nbytes > 0xffffffffull ? kRecBadCigar : kRecOk, r.reserved = 0;
		if (r.status != kRecOk) r.len = r.before = 0;
		P.res[id] = r;
	}
}

void junc_text_launch(const RecParams &P, bool write, void *stream)
{
	if (P.n_jobs <= 0) return;
	if (write) hipLaunchKernelGGL(junc_text_kernel<true>, dim3(P.n_jobs), dim3(64), 0, (hipStream_t)stream, P);
	else hipLaunchKernelGGL(junc_text_kernel<false>, dim3(P.n_jobs), dim3(64), 0, (hipStream_t)stream, P);
	HIP_CHECK(hipGetLastError());
}

} // namespace mm2amd
