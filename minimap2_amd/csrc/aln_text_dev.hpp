// aln_text_kernel: see aln_text.hpp.  One wavefront per alignment; the lanes walk the alignment's COLUMNS 64 at a time.
//
//   columns   a base pair of an M / = / X operation is a column in every mode.  cs: every inserted and every deleted base is one, an intron
//             (N) is ONE pseudo-column whatever its length.  MD: a deleted base is one; insertions and introns have none (the reference's
//             counter runs across them).  One more column, the terminator, follows the last: it only flushes what is pending;
//   staging   kTxtTileOps operations at a time go to LDS with their exclusive query / target / column offsets (three wave scans with
//             carries); a lane finds the operation of its column there by bisection;
//   runs      the text of a column may start with the length of the identity run that ends before it (cs ":n", MD "n").  A column that
//             ends or starts a run publishes the column the next run starts at; an exclusive max-scan (carried from step to step) gives
//             every column the start of the run it would flush, and so the run's length, without walking it;
//   bytes     every lane runs the column emitter on a counting sink; wave_inclusive_sum (with a 64-bit carry) turns the counts into
//             offsets.  The writing pass runs the SAME emitter again on a sink that stores into an LDS stage, placed so that the stage and
//             the destination agree modulo 4, and the wave copies the stage out in aligned dwords (single bytes at the two ragged ends);
//   ds        cs, except that an inserted or deleted stretch carries brackets around the bases by which the gap can be shifted (write_indel_ds).
//             The two extents of every I / D operation are found when its tile is staged (txt_ds_extents) and kept in two more LDS arrays; a
//             column of the operation then knows from (its index, len, ll, lr) alone which brackets it carries.
//
// The sizing pass validates first (64-bit sums: a CIGAR whose lengths wrap must not pass for one that covers the sequences), so that every
// sequence index the walk forms lies inside [0, qlen) / [0, tlen).
#pragma once
#include <hip/hip_runtime.h>
#include "hip_util.hpp"
#include "device_sort_dev.hpp"
#include "aln_text.hpp"

namespace mm2amd {

#define TXT_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); } while (0)

namespace {

__device__ __forceinline__ int txt_ndigits(uint32_t v)
{
	return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}
__device__ __forceinline__ int txt_lower(int c) { return (int)(0x6e74676361ull >> (c << 3) & 0xff); } // "acgtn"[c], c in 0..4
__device__ __forceinline__ int txt_upper(int c) { return txt_lower(c) - 0x20; }                        // "ACGTN"[c]
__device__ __forceinline__ int txt_nt4(uint32_t c) // kNt4Table (tables.cpp) without the table
{
	if (c < 4u) return (int)c;
	const uint32_t l = c | 0x20u;
	return l == 'a' ? 0 : l == 'c' ? 1 : l == 'g' ? 2 : (l == 't' || l == 'u') ? 3 : 4;
}
__device__ __forceinline__ uint32_t txt_inclusive_max(uint32_t v, int lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t u = __shfl_up(v, (unsigned)d);
		if (lane >= d) v = u > v ? u : v;
	}
	return v;
}

struct TxtCount { // the sizing sink
	uint32_t n = 0;
	__device__ __forceinline__ void ch(int) { ++n; }
	__device__ __forceinline__ void num(uint32_t v) { n += (uint32_t)txt_ndigits(v); }
};
struct TxtStore { // the writing sink: into the LDS stage
	char *p;
	__device__ __forceinline__ void ch(int c) { *p++ = (char)c; }
	__device__ __forceinline__ void num(uint32_t v)
	{
		char *e = p + txt_ndigits(v);
		p = e;
		do { *--e = (char)('0' + v % 10u); v /= 10u; } while (v);
	}
};

enum { TXT_NONE = 0, TXT_M, TXT_I, TXT_D, TXT_N, TXT_TERM };
struct TxtCol {
	int kind = TXT_NONE;
	bool first = false, ident = false; // first column of its operation; query base == target base (by code: N against N is a match)
	uint32_t pend = 0;                 // identity columns waiting to be flushed before this one
	uint32_t len = 0;                  // N: the intron's length; ds I / D: the operation's length
	uint32_t j = 0, ll = 0, lr = 0;    // ds I / D: the column's index in its operation; the operation's shift extents (txt_ds_extents)
	int a = 4, b = 4, c = 4, d = 4;    // M: query, target base; I: a; D: b; N: the first two (a, b) and the last two (c, d) target bases
};

// One base of a ds indel with the brackets of write_indel_ds (format.c:142-169) in closed form: ll + lr >= len brackets the whole stretch, otherwise
// the first ll and the last lr bases.
template <class Sink>
__device__ __forceinline__ void txt_emit_ds_base(Sink &o, const TxtCol &k, int base)
{
	const bool all = k.ll + k.lr >= k.len;
	const bool open = k.j == 0u ? (all || k.ll > 0u) : (!all && k.lr > 0u && k.j == k.len - k.lr);
	const bool close = k.j == k.len - 1u ? (all || k.lr > 0u) : (!all && k.ll > 0u && k.j == k.ll - 1u);
	if (open) o.ch('[');
	o.ch(txt_lower(base));
	if (close) o.ch(']');
}

// The text of one column -- the only place that knows what cs, ds, MD and CIGAR text look like; sizing and writing both go through it.
// DS: `what` may be a ds mode (the instances without it carry no code for the brackets).
template <bool DS, class Sink>
__device__ __forceinline__ void txt_emit_column(Sink &o, const TxtCol &k, int what)
{
	if (k.kind == TXT_NONE) return;
	if (what == kTxtMd) { // write_MD_core, format.c:302-331
		if (k.kind == TXT_M) { if (!k.ident) o.num(k.pend), o.ch(txt_upper(k.b)); }
		else if (k.kind == TXT_D) { if (k.first) o.num(k.pend), o.ch('^'); o.ch(txt_upper(k.b)); }
		else if (k.kind == TXT_TERM) { if (k.pend > 0) o.num(k.pend); }
		return;
	}
	// write_cs_ds_core, format.c:171-254: an identity run ends at a mismatch and at the end of every M / = / X operation; is_ds changes + and - only
	const bool lng = what == kTxtCsLong || (DS && what == kTxtDsLong), ds = DS && (what == kTxtDs || what == kTxtDsLong);
	if (!lng && k.pend > 0 && (!k.ident || k.first)) o.ch(':'), o.num(k.pend);
	if (k.kind == TXT_M) {
		if (!k.ident) o.ch('*'), o.ch(txt_lower(k.b)), o.ch(txt_lower(k.a));
		else if (lng) { if (k.first || k.pend == 0) o.ch('='); o.ch(txt_upper(k.a)); }
	} else if (k.kind == TXT_I) { if (k.first) o.ch('+'); if (ds) txt_emit_ds_base(o, k, k.a); else o.ch(txt_lower(k.a)); }
	else if (k.kind == TXT_D) { if (k.first) o.ch('-'); if (ds) txt_emit_ds_base(o, k, k.b); else o.ch(txt_lower(k.b)); }
	else if (k.kind == TXT_N) o.ch('~'), o.ch(txt_lower(k.a)), o.ch(txt_lower(k.b)), o.num(k.len), o.ch(txt_lower(k.c)), o.ch(txt_lower(k.d));
}
template <class Sink>
__device__ __forceinline__ void txt_emit_cigar(Sink &o, uint32_t w) { o.num(w >> 4), o.ch("MIDNSHP=XB"[w & 0xf]); } // write_sam_cigar; w & 15 <= 9

// n bytes of the stage, which start at stage byte `a` (= dst & 3), go to dst: whole dwords where both sides are aligned, bytes at the ends.
// Nothing outside [dst, dst + n) is written.
__device__ __forceinline__ void txt_copy_out(const uint32_t *stage, uint32_t a, uint32_t n, char *dst, int lane)
{
	const char *sb = (const char *)stage;
	char *gb = dst - a; // 4-byte aligned
	const uint32_t end = a + n, ndw = (end + 3u) >> 2;
	for (uint32_t j = (uint32_t)lane; j < ndw; j += 64u) {
		const uint32_t lo = j << 2, hi = lo + 4u;
		if (lo >= a && hi <= end) *(uint32_t *)(gb + lo) = stage[j];
		else for (uint32_t b = lo > a ? lo : a, e = hi < end ? hi : end; b < e; ++b) gb[b] = sb[b];
	}
}

// Where a walk's text goes: the bytes so far, and one step's way from per-lane counts to the destination.  place(): every lane has counted its
// bytes; offsets by a wave scan.  flush(): the writing pass has stored into the stage at `a` + its offset and the wave copies the step out.
template <bool WRITE>
struct TxtOut {
	char *out;                 // WRITE: where the text starts
	uint32_t *stage;           // LDS, (64 * kTxtColBytes + 4 + 3) / 4 + 1 words
	int lane;
	unsigned long long nbytes; // text so far (the same in every lane)
	__device__ __forceinline__ uint32_t place(uint32_t mine, uint32_t &a, uint32_t &excl) const
	{
		const uint32_t incl = wave_inclusive_sum(mine, lane);
		excl = incl - mine;
		a = WRITE ? (uint32_t)((uintptr_t)(out + nbytes) & 3u) : 0u;
		return (uint32_t)__shfl((int)incl, 63, 64);
	}
	__device__ __forceinline__ void flush(uint32_t a, uint32_t tot)
	{
		if (WRITE) {
			TXT_SYNC();
			txt_copy_out(stage, a, tot, out + nbytes, lane);
			TXT_SYNC();
		}
		nbytes += tot;
	}
};

// The sizing pass's judgement of a CIGAR (64-bit sums: lengths that wrap must not pass for a CIGAR that covers the sequences); the same in every lane.
__device__ __forceinline__ bool txt_bad_ops(const uint32_t *cg, uint32_t n, int what, int32_t qlen, int32_t tlen, int lane)
{
	bool bad = false;
	unsigned long long sq = 0, st = 0;
	for (uint32_t k = (uint32_t)lane; k < n; k += 64u) {
		const uint32_t w = cg[k], op = w & 0xf, len = w >> 4;
		if (what == kTxtCigar) { bad |= op > 9u; continue; }
		bad |= !(op <= 3u || op == 7u || op == 8u) || len == 0u || (op == 3u && len < 2u);
		if (op == 0u || op == 7u || op == 8u) sq += len, st += len;
		else if (op == 1u) sq += len;
		else if (op == 2u || op == 3u) st += len;
	}
	if (what != kTxtCigar) {
#pragma unroll
		for (int d = 32; d > 0; d >>= 1) sq += __shfl_xor(sq, d, 64), st += __shfl_xor(st, d, 64);
		bad |= qlen < 0 || tlen < 0 || sq != (unsigned long long)(long long)qlen || st != (unsigned long long)(long long)tlen;
	}
	return __ballot(bad) != 0ull;
}

// "<len><op>" of every operation, 64 operations a step
template <bool WRITE>
__device__ __forceinline__ void txt_walk_cigar(TxtOut<WRITE> &O, const uint32_t *cg, uint32_t n)
{
	const int lane = O.lane;
	for (uint32_t k0 = 0; k0 < n; k0 += 64u) {
		const uint32_t k = k0 + (uint32_t)lane;
		const uint32_t w = k < n ? cg[k] : 0u;
		TxtCount cnt;
		if (k < n) txt_emit_cigar(cnt, w);
		uint32_t a, excl;
		const uint32_t tot = O.place(cnt.n, a, excl);
		if (WRITE && k < n) { TxtStore s; s.p = (char *)O.stage + a + excl; txt_emit_cigar(s, w); }
		O.flush(a, tot);
	}
}

struct TxtSeqs { // where the bases of a walk come from (aln_text.hpp: kTxtQ* / kTxtT*)
	const uint8_t *qpool, *tpool;
	const uint32_t *S;
	uint64_t q_pos, t_pos;
	uint32_t qlen, tlen, qsrc, tsrc;
	__device__ __forceinline__ int qbase(uint32_t i) const
	{
		if (qsrc == kTxtQCodes) { const int c = qpool[q_pos + i]; return c > 4 ? 4 : c; }
		if (qsrc == kTxtQAscii) return txt_nt4(qpool[q_pos + i]);
		const int c = txt_nt4(qpool[q_pos + (qlen - 1u - i)]);
		return c >= 4 ? 4 : 3 - c;
	}
	__device__ __forceinline__ int tbase(uint32_t i) const
	{
		if (tsrc == kTxtTCodes) { const int c = tpool[t_pos + i]; return c > 4 ? 4 : c; }
		const uint64_t o = t_pos + (tsrc == kTxtTPacked ? i : tlen - 1u - i);
		const int c = (int)(S[o >> 3] >> ((o & 7) << 2) & 0xf);
		return tsrc == kTxtTPacked ? (c > 4 ? 4 : c) : (c < 4 ? 3 - c : 4);
	}
};

// ds: the shift extents of the nt staged operations (write_cs_ds_core, format.c:209-218 and :228-237).  For an I / D operation of length len that
// starts at y of its sequence s (the aligned query for I, the aligned target for D; L bases):
//   lr = the number of i = 1 .. len, from 1 on without a gap, with y - i >= 0 and s[y + len - i] == s[y - i]   (the gap can move left by lr)
//   ll = the number of z = 0 .. len - 1, from 0 on without a gap, with y + len + z < L and s[y + z] == s[y + len + z]   (... right by ll)
// The bounds are tested before a base is read, so every index lies in [0, L).  A lane scans the operations up to kTxtDsLaneScan long that it
// staged, on its own; the wave then takes the longer ones in turn, 64 comparisons a step, the first failure by ballot -- so no lane walks more
// than kTxtDsLaneScan bases alone, whatever the operation's length (a homopolymer makes every comparison succeed).
__device__ __forceinline__ void txt_ds_extents(const TxtSeqs &Q, uint32_t nt, const uint32_t *s_word, const uint32_t *s_q, const uint32_t *s_t,
                                               uint32_t *s_ll, uint32_t *s_lr, int lane)
{
	auto base = [&](bool ins, uint32_t i) { return ins ? Q.qbase(i) : Q.tbase(i); };
	auto left_ok = [&](bool ins, uint32_t y, uint32_t len, uint32_t i) { return y >= i && base(ins, y + len - i) == base(ins, y - i); };                 // i in 1 .. len
	auto right_ok = [&](bool ins, uint32_t y, uint32_t len, uint32_t L, uint32_t z) { return y + len + z < L && base(ins, y + z) == base(ins, y + len + z); }; // z in 0 .. len - 1
	for (uint32_t r = 0; r < nt; r += 64u) {
		const uint32_t i = r + (uint32_t)lane;
		uint32_t ll = 0, lr = 0;
		bool wide = false;
		if (i < nt) {
			const uint32_t w = s_word[i], op = w & 0xf, len = w >> 4;
			if (op == 1u || op == 2u) {
				const bool ins = op == 1u;
				const uint32_t y = ins ? s_q[i] : s_t[i], L = ins ? Q.qlen : Q.tlen;
				if (len <= (uint32_t)kTxtDsLaneScan) {
					while (lr < len && left_ok(ins, y, len, lr + 1u)) ++lr;
					while (ll < len && right_ok(ins, y, len, L, ll)) ++ll;
				} else wide = true;
			}
		}
		for (unsigned long long m = __ballot(wide); m; m &= m - 1ull) { // (the same in every lane)
			const int b = __ffsll((long long)m) - 1;
			const uint32_t k = r + (uint32_t)b, w = s_word[k], len = w >> 4;
			const bool ins = (w & 0xf) == 1u;
			const uint32_t y = ins ? s_q[k] : s_t[k], L = ins ? Q.qlen : Q.tlen;
			uint32_t zl = len, zr = len; // a lane beyond len fails, so the last step of a scan that runs to the end still ends it at len
			for (uint32_t z0 = 0; z0 < len; z0 += 64u) {
				const uint32_t z = z0 + (uint32_t)lane;
				const unsigned long long f = __ballot(!(z < len && left_ok(ins, y, len, z + 1u)));
				if (f) { zr = z0 + (uint32_t)(__ffsll((long long)f) - 1); break; }
			}
			for (uint32_t z0 = 0; z0 < len; z0 += 64u) {
				const uint32_t z = z0 + (uint32_t)lane;
				const unsigned long long f = __ballot(!(z < len && right_ok(ins, y, len, L, z)));
				if (f) { zl = z0 + (uint32_t)(__ffsll((long long)f) - 1); break; }
			}
			if (lane == b) ll = zl, lr = zr;
		}
		if (i < nt) s_ll[i] = ll, s_lr[i] = lr;
	}
}

// cs or ds (short or long) or MD of a CIGAR that txt_bad_ops has passed; s_word / s_q / s_t / s_col: kTxtTileOps words of LDS each.  DS: the walk
// can write ds, and s_ll / s_lr are two more such arrays; without it they are not touched (and `what` is not a ds mode).  Returns the columns walked.
template <bool WRITE, bool DS = false>
__device__ __forceinline__ uint32_t txt_walk_columns(TxtOut<WRITE> &O, const TxtSeqs &Q, int what, const uint32_t *cg, uint32_t n,
                                                     uint32_t *s_word, uint32_t *s_q, uint32_t *s_t, uint32_t *s_col,
                                                     uint32_t *s_ll = nullptr, uint32_t *s_lr = nullptr)
{
	const int lane = O.lane;
	const bool md = what == kTxtMd;
	const bool ds = DS && (what == kTxtDs || what == kTxtDsLong);
	uint32_t cq = 0, ct = 0, ccol = 0; // what the operations staged so far consume: query, target, columns
	uint32_t run_from = 0;             // the column the pending identity run starts at (max over the columns walked so far)
	// one step: the lane's column c (or none) -> its text
	auto step = [&](bool active, uint32_t c, uint32_t nt, bool term) {
		TxtCol k;
		uint32_t next_run = 0; // where a run that follows this column starts: 0 = this column says nothing
		if (active && term) k.kind = TXT_TERM;
		else if (active) {
			uint32_t lo = 0, hi = nt; // the last staged operation that starts at or before c (operations without columns never hold one)
			while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (s_col[mid] <= c) lo = mid; else hi = mid; }
			const uint32_t w = s_word[lo], op = w & 0xf, j = c - s_col[lo];
			k.first = j == 0u;
			if (op == 1u) k.kind = TXT_I, k.a = Q.qbase(s_q[lo] + j);
			else if (op == 2u) k.kind = TXT_D, k.b = Q.tbase(s_t[lo] + j);
			else if (op == 3u) {
				const uint32_t t0 = s_t[lo];
				k.kind = TXT_N, k.len = w >> 4;
				k.a = Q.tbase(t0), k.b = Q.tbase(t0 + 1u), k.c = Q.tbase(t0 + k.len - 2u), k.d = Q.tbase(t0 + k.len - 1u);
			} else k.kind = TXT_M, k.a = Q.qbase(s_q[lo] + j), k.b = Q.tbase(s_t[lo] + j), k.ident = k.a == k.b;
			if (DS && ds && (op == 1u || op == 2u)) k.len = w >> 4, k.j = j, k.ll = s_ll[lo], k.lr = s_lr[lo];
			if (md) next_run = k.ident ? 0u : c + 1u;          // a mismatch or a deleted base: the count starts again behind it
			else next_run = !k.ident ? c + 1u : k.first ? c : 0u; // cs: ... and an operation's first column starts a run of its own
		}
		const uint32_t incl = txt_inclusive_max(next_run, lane);
		uint32_t before = __shfl_up(incl, 1u);
		if (lane == 0) before = 0;
		before = before > run_from ? before : run_from;
		const uint32_t last = (uint32_t)__shfl((int)incl, 63, 64);
		run_from = last > run_from ? last : run_from;
		if (active) k.pend = c - before;
		TxtCount cnt;
		txt_emit_column<DS>(cnt, k, what);
		uint32_t a, excl;
		const uint32_t tot = O.place(cnt.n, a, excl);
		if (WRITE && cnt.n) { TxtStore s; s.p = (char *)O.stage + a + excl; txt_emit_column<DS>(s, k, what); }
		O.flush(a, tot);
	};

	for (uint32_t tile0 = 0; tile0 < n; tile0 += (uint32_t)kTxtTileOps) {
		const uint32_t nt = n - tile0 < (uint32_t)kTxtTileOps ? n - tile0 : (uint32_t)kTxtTileOps;
		const uint32_t col0 = ccol;
		TXT_SYNC(); // (the steps of the tile before have read the arrays)
		for (uint32_t r = 0; r < nt; r += 64u) {
			const uint32_t i = r + (uint32_t)lane;
			uint32_t w = 0, dq = 0, dt = 0, dc = 0;
			if (i < nt) {
				w = cg[tile0 + i];
				const uint32_t op = w & 0xf, len = w >> 4;
				if (op == 1u) dq = len, dc = md ? 0u : len;
				else if (op == 2u) dt = len, dc = len;
				else if (op == 3u) dt = len, dc = md ? 0u : 1u;
				else dq = dt = dc = len;
			}
			const uint32_t iq = wave_inclusive_sum(dq, lane), it = wave_inclusive_sum(dt, lane), ic = wave_inclusive_sum(dc, lane);
			if (i < nt) s_word[i] = w, s_q[i] = cq + iq - dq, s_t[i] = ct + it - dt, s_col[i] = ccol + ic - dc;
			cq += (uint32_t)__shfl((int)iq, 63, 64), ct += (uint32_t)__shfl((int)it, 63, 64), ccol += (uint32_t)__shfl((int)ic, 63, 64);
		}
		TXT_SYNC();
		if (DS && ds) {
			txt_ds_extents(Q, nt, s_word, s_q, s_t, s_ll, s_lr, lane);
			TXT_SYNC();
		}
		for (unsigned long long c0 = col0; c0 < ccol; c0 += 64ull) { // (64 bits: columns may reach 2^32 - 2)
			const unsigned long long c = c0 + (unsigned long long)lane;
			step(c < ccol, (uint32_t)c, nt, false);
		}
	}
	step(lane == 0, ccol, 0u, true); // the terminator
	return ccol;
}

} // namespace

// DS: the instance for the two ds modes, with the two arrays of shift extents; the other modes run the instance without them.
template <bool WRITE, bool DS>
__global__ void __launch_bounds__(64) aln_text_kernel(TxtParams P)
{
	__shared__ uint32_t s_word[kTxtTileOps], s_q[kTxtTileOps], s_t[kTxtTileOps], s_col[kTxtTileOps];
	__shared__ uint32_t s_ll[DS ? kTxtTileOps : 1], s_lr[DS ? kTxtTileOps : 1];
	__shared__ uint32_t s_stage[(64 * kTxtColBytes + 4 + 3) / 4 + 1];
	const int lane = (int)threadIdx.x;
	const int id = (int)blockIdx.x;
	const TxtJob J = P.jobs[id];
	const int what = P.what;
	const uint32_t n = J.n_cigar;
	const uint32_t *cg = P.cigar + J.cig_off;

	if (WRITE) { // the sizing pass has judged the job
		const TxtRes r = P.res[id];
		if (r.status != 0 || r.len == 0) return;
	} else if (txt_bad_ops(cg, n, what, J.qlen, J.tlen, lane)) { // (an invalid job writes nothing but its own result)
		if (lane == 0) { TxtRes r; r.cols = 0, r.len = 0, r.status = -1; P.res[id] = r; }
		return;
	}

	TxtOut<WRITE> O;
	O.out = WRITE ? P.out + P.off[id] : nullptr, O.stage = s_stage, O.lane = lane, O.nbytes = 0;
	uint32_t cols = n;
	if (what == kTxtCigar) txt_walk_cigar(O, cg, n);
	else {
		TxtSeqs Q;
		Q.qpool = P.qpool, Q.tpool = P.tpool, Q.S = P.S, Q.q_pos = J.q_pos, Q.t_pos = J.t_pos, Q.qlen = (uint32_t)J.qlen, Q.tlen = (uint32_t)J.tlen, Q.qsrc = J.qsrc, Q.tsrc = J.tsrc;
		cols = txt_walk_columns<WRITE, DS>(O, Q, what, cg, n, s_word, s_q, s_t, s_col, s_ll, s_lr);
	}
	if (!WRITE && lane == 0) { TxtRes r; r.cols = cols, r.len = (uint32_t)O.nbytes, r.status = O.nbytes > 0xffffffffull ? -1 : 0; if (r.status) r.len = 0; P.res[id] = r; }
}

void aln_text_launch(const TxtParams &P, bool write, void *stream)
{
	if (P.n_jobs <= 0) return;
	const bool ds = P.what == kTxtDs || P.what == kTxtDsLong;
	if (write && ds) hipLaunchKernelGGL((aln_text_kernel<true, true>), dim3(P.n_jobs), dim3(64), 0, (hipStream_t)stream, P);
	else if (write) hipLaunchKernelGGL((aln_text_kernel<true, false>), dim3(P.n_jobs), dim3(64), 0, (hipStream_t)stream, P);
	else if (ds) hipLaunchKernelGGL((aln_text_kernel<false, true>), dim3(P.n_jobs), dim3(64), 0, (hipStream_t)stream, P);
	else hipLaunchKernelGGL((aln_text_kernel<false, false>), dim3(P.n_jobs), dim3(64), 0, (hipStream_t)stream, P);
	HIP_CHECK(hipGetLastError());
}

} // namespace mm2amd
