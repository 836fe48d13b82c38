// rec_text_kernel: see rec_text.hpp.  One wavefront per output record.  The record is a sequence of PIECES, every piece one or more steps of
// aln_text_dev.hpp's scheme (count per lane, wave scan, store into the LDS stage, aligned copy out):
//   short pieces  numbers, flags, the tag block: lane 0 runs the piece's emitter -- a few hundred bytes at most;
//   names         16 bytes per lane and step;
//   CIGAR, cs/MD  txt_walk_cigar / txt_walk_columns: all lanes, as in aln_text_kernel.
// Sizing and writing are this one function on a counting and on a storing sink.  Before the first piece the wave counts the CIGAR's gaps
// (mm_count_gaps: de:f precedes cg:Z: in a PAF line, so the counts cannot wait for the CIGAR's own walk) and the sizing pass judges the
// operations, so that every sequence index the cs / MD walk forms lies inside the stretches the planner has checked.
#pragma once
#include "aln_text_dev.hpp"
#include "rec_text.hpp"
#include "fraction.hpp"

namespace mm2amd {

namespace {

constexpr int64_t kRF_OUT_CG = 0x020, kRF_OUT_CS = 0x040, kRF_OUT_SAM = 0x008, kRF_OUT_CS_LONG = 0x800, kRF_SOFTCLIP = 0x80000, kRF_OUT_MD = 0x1000000,
	kRF_QSTRAND = 0x100000000LL, kRF_SECONDARY_SEQ = 0x1000000000LL;
constexpr uint32_t kRecNameStep = 16; // bytes of a name per lane and step (64 x 16 fit the stage)

template <class Sink> __device__ __forceinline__ void rec_str(Sink &o, const char *s) { while (*s) o.ch(*s++); }
template <class Sink> __device__ __forceinline__ void rec_int(Sink &o, int32_t v)
{
	if (v < 0) o.ch('-'), o.num(0u - (uint32_t)v); else o.num((uint32_t)v);
}
template <class Sink> __device__ __forceinline__ void rec_tag(Sink &o, const char *name, int32_t v) { o.ch('\t'), rec_str(o, name), rec_int(o, v); }

// a short piece: lane 0's emitter f(sink)
template <bool WRITE, class F>
__device__ __forceinline__ void rec_small(TxtOut<WRITE> &O, F &&f)
{
	TxtCount cnt;
	if (O.lane == 0) f(cnt);
	uint32_t a, excl;
	const uint32_t tot = O.place(cnt.n, a, excl);
	if (WRITE && O.lane == 0) { TxtStore s; s.p = (char *)O.stage + a + excl; f(s); }
	O.flush(a, tot);
}
// n bytes as they are
template <bool WRITE>
__device__ __forceinline__ void rec_bytes(TxtOut<WRITE> &O, const char *src, uint32_t n)
{
	for (uint32_t k0 = 0; k0 < n; k0 += 64u * kRecNameStep) {
		const uint32_t lo = k0 + (uint32_t)O.lane * kRecNameStep;
		const uint32_t mine = lo >= n ? 0u : n - lo < kRecNameStep ? n - lo : kRecNameStep;
		uint32_t a, excl;
		const uint32_t tot = O.place(mine, a, excl);
		if (WRITE) { char *w = (char *)O.stage + a + excl; for (uint32_t j = 0; j < mine; ++j) w[j] = src[lo + j]; }
		O.flush(a, tot);
	}
}

// "0" or %.4f of a value in [0, 1] (put_fraction, format.cpp); false: the value is snprintf's
template <class Sink>
__device__ __forceinline__ bool rec_fraction(Sink &o, double v)
{
	if (v == 0.0) { o.ch('0'); return true; }
	if (!(v >= 0.0 && v <= 1.0)) return false;
	const unsigned q = fraction_q4(v);
	o.ch('0' + (int)(q / 10000u)), o.ch('.'), o.ch('0' + (int)(q / 1000u % 10u)), o.ch('0' + (int)(q / 100u % 10u)), o.ch('0' + (int)(q / 10u % 10u)), o.ch('0' + (int)(q % 10u));
	return true;
}

// write_tags (format.c:397-423); false: the fraction is outside [0, 1]
template <class Sink>
__device__ __forceinline__ bool rec_tags(Sink &o, const RecHit &h, int n_gap, int n_gapo)
{
	const bool has_p = (h.bits & kRecHasP) != 0, parent = (h.bits & kRecIsParent) != 0, inv = (h.bits & kRecInv) != 0;
	const int split = (int)(h.bits >> kRecSplitShift & 3u), ts = (int)(h.bits >> kRecTransShift & 3u);
	bool ok = true;
	if (has_p) {
		rec_tag(o, "NM:i:", h.blen - h.mlen + (int32_t)h.n_ambi), rec_tag(o, "ms:i:", h.dp_max0), rec_tag(o, "AS:i:", h.dp_score), rec_tag(o, "nn:i:", (int32_t)h.n_ambi);
		if (ts == 1 || ts == 2) rec_str(o, "\tts:A:"), o.ch(ts == 1 ? '+' : '-');
	}
	rec_str(o, "\ttp:A:"), o.ch(parent ? (inv ? 'I' : 'P') : (inv ? 'i' : 'S'));
	rec_tag(o, "cm:i:", h.cnt), rec_tag(o, "s1:i:", h.score);
	if (parent) rec_tag(o, "s2:i:", h.subsc);
	if (has_p) { // mm_event_identity (align.c:997-1003) in IEEE double
		rec_str(o, "\tde:f:");
		const double div = 1.0 - (double)h.mlen / (double)(h.blen + (int32_t)h.n_ambi - n_gap + n_gapo);
		ok = rec_fraction(o, div);
	} else if (h.div >= 0.0f && h.div <= 1.0f) {
		rec_str(o, "\tdv:f:");
		ok = rec_fraction(o, (double)h.div);
	}
	if (split) rec_tag(o, "zd:i:", split);
	return ok;
}

} // namespace

template <bool WRITE>
__global__ void __launch_bounds__(64) rec_text_kernel(RecParams P)
{
	__shared__ uint32_t s_word[kTxtTileOps], s_q[kTxtTileOps], s_t[kTxtTileOps], s_col[kTxtTileOps];
	__shared__ uint32_t s_stage[(64 * kTxtColBytes + 4 + 3) / 4 + 1];
	const int lane = (int)threadIdx.x;
	const int id = (int)blockIdx.x;
	const RecJob J = P.jobs[id];
	const int64_t flag = P.flag;
	const bool sam = (flag & kRF_OUT_SAM) != 0, mapped = J.hit >= 0;
	const int what = (flag & kRF_OUT_MD) ? kTxtMd : (flag & kRF_OUT_CS) ? ((flag & kRF_OUT_CS_LONG) ? kTxtCsLong : kTxtCs) : kTxtCigar; // kTxtCigar: no per-base tag
	RecHit H;
	if (mapped) H = P.hits[J.hit]; else { H = RecHit(); H.bits = 0, H.n_cigar = 0, H.cig_off = 0; }
	const bool has_p = mapped && (H.bits & kRecHasP) != 0, rev = (H.bits & kRecRev) != 0;
	const uint32_t n = has_p ? H.n_cigar : 0u;
	const uint32_t *cg = P.cigar + H.cig_off;
	const bool columns = has_p && what != kTxtCigar;

	if (WRITE) { // the sizing pass has judged the record
		const RecRes r = P.res[id];
		if (r.status != kRecOk || r.len == 0) return;
	} else if (txt_bad_ops(cg, n, columns ? what : kTxtCigar, H.qe - H.qs, H.re - H.rs, lane)) {
		if (lane == 0) { RecRes r; r.len = r.before = 0, r.status = kRecBadCigar, r.reserved = 0; P.res[id] = r; }
		return;
	}
	int n_gap = 0, n_gapo = 0; // mm_count_gaps (align.c:985-995)
	for (uint32_t k = (uint32_t)lane; k < n; k += 64u) {
		const uint32_t w = cg[k], op = w & 0xf;
		if (op == 1u || op == 2u) ++n_gapo, n_gap += (int)(w >> 4);
	}
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) n_gap += __shfl_xor(n_gap, d, 64), n_gapo += __shfl_xor(n_gapo, d, 64);

	TxtOut<WRITE> O;
	O.out = WRITE ? P.out + P.off[id] : nullptr, O.stage = s_stage, O.lane = lane, O.nbytes = 0;
	bool frac_ok = true;   // (lane 0's)
	uint32_t before = 0;   // SAM: the bytes in front of the hole
	const char *tname = nullptr;
	uint32_t tname_len = 0, tlen = 0;
	if (mapped) tname = P.tnames + P.tname_off[H.rid], tname_len = (uint32_t)(P.tname_off[H.rid + 1] - P.tname_off[H.rid]), tlen = P.tlen[H.rid];
	auto per_base = [&]() { // cs / MD with the tag's name in front
		if (!columns) return;
		rec_small(O, [&](auto &o) { rec_str(o, what == kTxtMd ? "\tMD:Z:" : "\tcs:Z:"); });
		TxtSeqs Q;
		Q.qpool = P.qpool, Q.tpool = nullptr, Q.S = P.S, Q.q_pos = H.q_pos, Q.t_pos = H.t_pos, Q.qlen = (uint32_t)(H.qe - H.qs), Q.tlen = (uint32_t)(H.re - H.rs), Q.qsrc = H.qsrc, Q.tsrc = H.tsrc;
		txt_walk_columns(O, Q, what, cg, n, s_word, s_q, s_t, s_col);
	};

	rec_bytes(O, P.names + J.name_off, J.name_len);
	if (!sam) { // mm_write_paf4
		if (!mapped) {
			rec_small(O, [&](auto &o) {
				o.ch('\t'), rec_int(o, J.l_seq), rec_str(o, "\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0");
				if (J.rep_len >= 0) rec_tag(o, "rl:i:", J.rep_len);
				o.ch('\n');
			});
		} else {
			rec_small(O, [&](auto &o) {
				o.ch('\t'), rec_int(o, J.l_seq), o.ch('\t'), rec_int(o, H.qs), o.ch('\t'), rec_int(o, H.qe), o.ch('\t'), o.ch(rev ? '-' : '+'), o.ch('\t');
				if (tname_len == 0) rec_int(o, H.rid); // an index without names: the sequence's number
			});
			rec_bytes(O, tname, tname_len);
			rec_small(O, [&](auto &o) {
				o.ch('\t'), o.num(tlen), o.ch('\t');
				if ((flag & kRF_QSTRAND) && rev) rec_int(o, (int32_t)tlen - H.re), o.ch('\t'), rec_int(o, (int32_t)tlen - H.rs); // format.c:440-443
				else rec_int(o, H.rs), o.ch('\t'), rec_int(o, H.re);
				o.ch('\t'), rec_int(o, H.mlen), o.ch('\t'), rec_int(o, H.blen), o.ch('\t'), o.num(H.bits & 0xffu);
				frac_ok = rec_tags(o, H, n_gap, n_gapo);
				if (J.rep_len >= 0) rec_tag(o, "rl:i:", J.rep_len);
				if (has_p && (flag & kRF_OUT_CG)) rec_str(o, "\tcg:Z:");
			});
			if (has_p && (flag & kRF_OUT_CG)) txt_walk_cigar(O, cg, n);
			per_base();
			rec_small(O, [&](auto &o) { o.ch('\n'); });
		}
		before = (uint32_t)O.nbytes;
	} else { // mm_write_sam3, n_seg == 1
		int sf = 0;
		if (!mapped) sf |= 0x4;
		else {
			if (rev) sf |= 0x10;
			if (!(H.bits & kRecIsParent)) sf |= 0x100;
			else if (!(H.bits & kRecSamPri)) sf |= 0x800;
		}
		if (!mapped) {
			rec_small(O, [&](auto &o) { o.ch('\t'), o.num((uint32_t)sf), rec_str(o, "\t*\t0\t0\t*\t*\t0\t0\t"); });
			before = (uint32_t)O.nbytes;
		} else {
			const uint32_t clip0 = (uint32_t)(rev ? J.l_seq - H.qe : H.qs), clip1 = (uint32_t)(rev ? H.qs : J.l_seq - H.qe); // write_sam_cigar (format.c:494-520)
			const bool hard = ((sf & 0x800) || ((sf & 0x100) && (flag & kRF_SECONDARY_SEQ))) && !(flag & kRF_SOFTCLIP);
			rec_small(O, [&](auto &o) { o.ch('\t'), o.num((uint32_t)sf), o.ch('\t'); });
			rec_bytes(O, tname, tname_len);
			rec_small(O, [&](auto &o) {
				o.ch('\t'), rec_int(o, H.rs + 1), o.ch('\t'), o.num(H.bits & 0xffu), o.ch('\t');
				if (!has_p) o.ch('*');
				else if (clip0) o.num(clip0), o.ch(hard ? 'H' : 'S');
			});
			if (has_p) txt_walk_cigar(O, cg, n);
			rec_small(O, [&](auto &o) {
				if (has_p && clip1) o.num(clip1), o.ch(hard ? 'H' : 'S');
				rec_str(o, "\t*\t0\t0\t");
			});
			before = (uint32_t)O.nbytes;
			rec_small(O, [&](auto &o) { frac_ok = rec_tags(o, H, n_gap, n_gapo); });
			if ((H.bits & kRecIsParent) && has_p && J.n_hits > 1u) { // supplementary alignments of the same read (format.c:638-664)
				bool first = true;
				for (uint32_t i = J.hit0; i < J.hit0 + J.n_hits; ++i) {
					if ((int32_t)i == J.hit) continue;
					const RecHit Q = P.hits[i];
					if (!(Q.bits & kRecIsParent) || !(Q.bits & kRecHasP)) continue;
					if (first) rec_small(O, [&](auto &o) { rec_str(o, "\tSA:Z:"); });
					first = false;
					rec_bytes(O, P.tnames + P.tname_off[Q.rid], (uint32_t)(P.tname_off[Q.rid + 1] - P.tname_off[Q.rid]));
					rec_small(O, [&](auto &o) {
						const bool qrev = (Q.bits & kRecRev) != 0;
						int l_M, l_I = 0, l_D = 0;
						if (Q.qe - Q.qs < Q.re - Q.rs) l_M = Q.qe - Q.qs, l_D = (Q.re - Q.rs) - l_M;
						else l_M = Q.re - Q.rs, l_I = (Q.qe - Q.qs) - l_M;
						const int clip5 = qrev ? J.l_seq - Q.qe : Q.qs, clip3 = qrev ? Q.qs : J.l_seq - Q.qe;
						o.ch(','), rec_int(o, Q.rs + 1), o.ch(','), o.ch(qrev ? '-' : '+'), o.ch(',');
						if (clip5) rec_int(o, clip5), o.ch('S');
						if (l_M) rec_int(o, l_M), o.ch('M');
						if (l_I) rec_int(o, l_I), o.ch('I');
						if (l_D) rec_int(o, l_D), o.ch('D');
						if (clip3) rec_int(o, clip3), o.ch('S');
						o.ch(','), o.num(Q.bits & 0xffu), o.ch(','), rec_int(o, Q.blen - Q.mlen + (int32_t)Q.n_ambi), o.ch(';');
					});
				}
			}
			per_base();
		}
		rec_small(O, [&](auto &o) {
			if (J.rep_len >= 0) rec_tag(o, "rl:i:", J.rep_len);
			o.ch('\n');
		});
	}
	if (!WRITE && lane == 0) {
		RecRes r;
		r.len = (uint32_t)O.nbytes, r.before = before, r.status = O.nbytes > 0xffffffffull ? kRecBadCigar : frac_ok ? kRecOk : kRecFraction, r.reserved = 0;
		if (r.status != kRecOk) r.len = r.before = 0;
		P.res[id] = r;
	}
}

void rec_text_launch(const RecParams &P, bool write, void *stream)
{
	if (P.n_jobs <= 0) return;
	if (write) hipLaunchKernelGGL(rec_text_kernel<true>, dim3(P.n_jobs), dim3(64), 0, (hipStream_t)stream, P);
	else hipLaunchKernelGGL(rec_text_kernel<false>, dim3(P.n_jobs), dim3(64), 0, (hipStream_t)stream, P);
	HIP_CHECK(hipGetLastError());
}

} // namespace mm2amd
