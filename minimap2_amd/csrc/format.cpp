// Host output stage: the text the reference writes in step 2 of its pipeline (map.c:585-623) -- SAM
// records as mm_write_sam3 (format.c:522-679) and PAF records as mm_write_paf4 (format.c:425-458) produce them, with the tag
// block of write_tags (:397-423) and the cs / ds / MD strings of write_cs_ds_core / write_MD_core (:171-254, :302-331) --
// formatted for a whole mini-batch on the host thread pool instead of by the single pipeline thread.  Once mapping is an
// order of magnitude faster, that single thread is the Amdahl term; records are independent, so reads are cut into chunks,
// every chunk is formatted into its own buffer by one pool thread, and the buffers are concatenated in input order.
// Single-segment fragments only (the mapper's scope); no read-group tag (-R is CLI state of the reference).
#include <array>
#include <atomic>
#include <chrono>
#include <cassert>
#include <cstdio>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>
#include "format.hpp"
#include "fraction.hpp"
#include "backend.hpp"
#include "aln_text.hpp"
#include "threads.hpp"
#include "host_prof.hpp"
#include "tables.hpp"
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace mm2amd {

using namespace ref;

namespace {

constexpr int64_t F_OUT_CG = 0x020, F_OUT_CS = 0x040, F_OUT_CS_LONG = 0x800, F_LONG_CIGAR = 0x10000, F_SOFTCLIP = 0x80000, F_OUT_MD = 0x1000000,
	F_COPY_COMMENT = 0x2000000, F_PAF_NO_HIT = 0x8000000, F_SAM_HIT_ONLY = 0x40000000, F_SECONDARY_SEQ = 0x1000000000LL, F_OUT_DS = 0x2000000000LL,
	F_OUT_JUNC = 0x10000000000LL;
const char kCigarOps[] = "MIDNSHP=XB";

// append-only byte buffer.  One per chunk of fragments, in a vector, each filled by a different pool thread: the object is padded to
// two cache lines, because std::string updates its length field on EVERY appended byte and neighbouring objects sharing a line made 64
// threads on two sockets ping-pong it -- 20-40 ns per byte instead of 1.3 (profiles/r03: 25-50 core-seconds per Gbase of reads).
struct alignas(128) Text {
	char *p = nullptr;
	size_t n = 0, cap = 0;
	Text() = default;
	Text(Text &&o) noexcept : p(o.p), n(o.n), cap(o.cap) { o.p = nullptr, o.n = o.cap = 0; }
	Text(const Text &) = delete;
	Text &operator=(const Text &) = delete;
	~Text() { free(p); }
	void clear() { n = 0; }
	size_t size() const { return n; }
	const char *data() const { return p; }
	char *need(size_t k) // room for k more bytes; returns where they go (the caller advances n)
	{
		if (n + k > cap) {
			size_t c = cap ? cap : 4096;
			while (c < n + k) c += c / 2 + 64;
			char *q = (char *)realloc(p, c);
			if (!q) throw std::bad_alloc();
			p = q, cap = c;
		}
		return p + n;
	}
	void ch(char c) { *need(1) = c, ++n; }
	void str(const char *s) { str(s, strlen(s)); }
	void str(const char *s, size_t l) { memcpy(need(l), s, l), n += l; }
	static char *put_u64(char *w, uint64_t x) // decimal digits of x at w; returns the end
	{
		char buf[20];
		int l = 0;
		do buf[l++] = (char)('0' + x % 10), x /= 10; while (x);
		while (l) *w++ = buf[--l];
		return w;
	}
	static char *put_u32(char *w, uint32_t x) // the common case: CIGAR lengths and flags, one to three digits
	{
		if (x < 10) { *w++ = (char)('0' + x); return w; }
		if (x < 100) { w[0] = (char)('0' + x / 10), w[1] = (char)('0' + x % 10); return w + 2; }
		if (x < 1000) { w[0] = (char)('0' + x / 100), w[1] = (char)('0' + x / 10 % 10), w[2] = (char)('0' + x % 10); return w + 3; }
		return put_u64(w, x);
	}
	void num(int64_t v)
	{
		char *w = need(21);
		if (v < 0) *w++ = '-';
		const uint64_t x = v < 0 ? (uint64_t)(-v) : (uint64_t)v;
		w = x <= UINT32_MAX ? put_u32(w, (uint32_t)x) : put_u64(w, x);
		n = (size_t)(w - p);
	}
	void tag(const char *name, int64_t v) { ch('\t'), str(name), num(v); } // "\tNM:i:" + value
	// (round 5) the writer of a CIGAR's text also counts its gaps -- what the de:f tag of the same record needs (mm_count_gaps): the record's second and third
	// walk over the 1400 operations of a 10 kb read were a third of the formatting time
	// (round 6) the counts belong to the Text they were made for, not to the thread: whoever writes a record's tags into this object finds what the
	// same object's cigar() counted, keyed by the CIGAR's address and length; a caller with a fresh Text finds nothing and counts itself
	struct GapCount { const uint32_t *c = nullptr; uint32_t n = 0; int n_gap = 0, n_gapo = 0; } gaps;
	void cigar(const uint32_t *c, uint32_t n_cigar) // <len><op> per entry
	{
		int n_gap = 0, n_gapo = 0;
		// lengths below 1000 (all but a handful per read) from a table: four bytes stored, the digit count added -- no branch on the number of digits
		static const struct Small { uint32_t chars[1000]; uint8_t len[1000]; Small() { for (uint32_t x = 0; x < 1000; ++x) { char b[8] = {0}; len[x] = (uint8_t)(put_u32(b, x) - b); memcpy(&chars[x], b, 4); } } } small;
		char *w = need((size_t)n_cigar * 11 + 4);
		for (uint32_t k = 0; k < n_cigar; ++k) {
			const uint32_t x = c[k] >> 4, op = c[k] & 0xf;
			if (x < 1000) memcpy(w, &small.chars[x], 4), w += small.len[x];
			else w = put_u32(w, x);
			*w++ = kCigarOps[op];
			const uint32_t is_gap = (op - 1u) < 2u; // I or D
			n_gapo += (int)is_gap, n_gap += (int)(is_gap ? x : 0u);
		}
		n = (size_t)(w - p);
		gaps.c = c, gaps.n = n_cigar, gaps.n_gap = n_gap, gaps.n_gapo = n_gapo;
	}
};

struct Seqs { std::vector<uint8_t> q, t; std::string tmp; }; // per-thread scratch for cs/ds/MD

void count_gaps(const Text &o, const Reg1 &r, int *n_gap, int *n_gapo) // mm_count_gaps (align.c:985-995)
{
	*n_gap = *n_gapo = 0;
	if (!r.p) return;
	const Text::GapCount &g = o.gaps;
	if (g.c == r.p->cigar && g.n == r.p->n_cigar) { *n_gap = g.n_gap, *n_gapo = g.n_gapo; return; } // counted while this record's CIGAR text was written
	for (uint32_t i = 0; i < r.p->n_cigar; ++i) {
		const int op = r.p->cigar[i] & 0xf, len = r.p->cigar[i] >> 4;
		if (op == 1 || op == 2) ++*n_gapo, *n_gap += len;
	}
}

double event_identity(const Text &o, const Reg1 &r) // mm_event_identity (align.c:997-1003)
{
	if (!r.p) return -1.0f;
	int n_gap, n_gapo;
	count_gaps(o, r, &n_gap, &n_gapo);
	return (double)r.mlen / (r.blen + r.p->n_ambi - n_gap + n_gapo);
}

// "%.4f" of v in [0, 1] exactly as printf rounds it (fraction.hpp).  Anything else goes to snprintf.
bool put_fraction_exact(Text &o, double v)
{
	if (!(v >= 0.0 && v <= 1.0)) return false;
	const unsigned q = fraction_q4(v); // fraction.hpp: the rounding rec_text_kernel uses as well
	char *w = o.need(8);
	w[0] = (char)('0' + q / 10000), w[1] = '.';
	w[2] = (char)('0' + q / 1000 % 10), w[3] = (char)('0' + q / 100 % 10), w[4] = (char)('0' + q / 10 % 10), w[5] = (char)('0' + q % 10);
	o.n += 6;
	return true;
}
void put_fraction(Text &o, double v) // "0" or %.4f (format.c:413-414, :418-419)
{
	if (v == 0.0) { o.ch('0'); return; }
	if (put_fraction_exact(o, v)) return;
	char buf[16];
	snprintf(buf, 16, "%.4f", v);
	o.str(buf);
}

void put_tags(Text &o, const Reg1 &r) // write_tags
{
	const char type = r.id == r.parent ? (r.inv ? 'I' : 'P') : (r.inv ? 'i' : 'S');
	if (r.p) {
		o.tag("NM:i:", r.blen - r.mlen + (int)r.p->n_ambi), o.tag("ms:i:", r.p->dp_max0), o.tag("AS:i:", r.p->dp_score), o.tag("nn:i:", (int)r.p->n_ambi);
		if (r.p->trans_strand == 1 || r.p->trans_strand == 2) o.str("\tts:A:"), o.ch("?+-?"[r.p->trans_strand]);
	}
	o.str("\ttp:A:"), o.ch(type), o.tag("cm:i:", r.cnt), o.tag("s1:i:", r.score);
	if (r.parent == r.id) o.tag("s2:i:", r.subsc);
	if (r.p) {
		o.str("\tde:f:");
		const double div = 1.0 - event_identity(o, r);
		if (div == 0.0) o.ch('0'); else put_fraction(o, div);
	} else if (r.div >= 0.0f && r.div <= 1.0f) {
		o.str("\tdv:f:");
		if (r.div == 0.0f) o.ch('0'); else put_fraction(o, r.div);
	}
	if (r.split) o.tag("zd:i:", r.split);
}

// the aligned stretches of query and target as nt4 codes, query on the alignment strand (write_cs_ds_or_MD, format.c:333-362)
void fetch_pair(const FlatIndex &fi, const Bseq1 &t, const Reg1 &r, Seqs &sq, bool is_qstrand)
{
	sq.q.resize(r.qe - r.qs), sq.t.resize(r.re - r.rs);
	fi.getseq2(is_qstrand && r.rev, r.rid, r.rs, r.re, sq.t.data()); // format.c:343-346: query as given, reference reverse-complemented
	if (!r.rev || is_qstrand) for (int i = r.qs; i < r.qe; ++i) sq.q[i - r.qs] = kNt4Table[(uint8_t)t.seq[i]];
	else for (int i = r.qs; i < r.qe; ++i) { const uint8_t c = kNt4Table[(uint8_t)t.seq[i]]; sq.q[r.qe - i - 1] = c >= 4 ? 4 : 3 - c; }
}

void put_bases(Text &o, const char *alphabet, const uint8_t *s, int64_t n) { for (int64_t i = 0; i < n; ++i) o.ch(alphabet[s[i]]); }

void put_ds_indel(Text &o, int64_t len, const uint8_t *seq, int64_t ll, int64_t lr) // write_indel_ds (format.c:142-169)
{
	if (ll + lr >= len) { o.ch('['), put_bases(o, "acgtn", seq, len), o.ch(']'); return; }
	int64_t k = 0;
	if (ll > 0) o.ch('['), put_bases(o, "acgtn", seq, ll), o.ch(']'), k += ll;
	put_bases(o, "acgtn", seq + k, len - lr - ll), k += len - lr - ll;
	if (lr > 0) o.ch('['), put_bases(o, "acgtn", seq + k, lr), o.ch(']');
}

void put_cs(Text &o, const Reg1 &r, const Seqs &sq, bool no_iden, bool is_ds) // write_cs_ds_core
{
	const uint8_t *qs = sq.q.data(), *ts = sq.t.data();
	o.str(is_ds ? "\tds:Z:" : "\tcs:Z:");
	int q_len = 0, t_len = 0;
	for (uint32_t i = 0; i < r.p->n_cigar; ++i) {
		const int op = r.p->cigar[i] & 0xf, len = r.p->cigar[i] >> 4;
		if (op == 0 || op == 7 || op == 8) q_len += len, t_len += len;
		else if (op == 1) q_len += len;
		else if (op == 2 || op == 3) t_len += len;
	}
	int q_off = 0, t_off = 0;
	for (uint32_t i = 0; i < r.p->n_cigar; ++i) {
		const int op = r.p->cigar[i] & 0xf, len = r.p->cigar[i] >> 4;
		if (op == 0 || op == 7 || op == 8) {
			int run = 0; // identical bases seen since the last difference
			auto flush = [&](int end) {
				if (run == 0) return;
				if (no_iden) o.ch(':'), o.num(run);
				else o.ch('='), put_bases(o, "ACGTN", qs + q_off + end - run, run);
				run = 0;
			};
			for (int j = 0; j < len; ++j) {
				if (qs[q_off + j] != ts[t_off + j]) flush(j), o.ch('*'), o.ch("acgtn"[ts[t_off + j]]), o.ch("acgtn"[qs[q_off + j]]);
				else ++run;
			}
			flush(len);
			q_off += len, t_off += len;
		} else if (op == 1) {
			o.ch('+');
			if (is_ds) { // how far the inserted bases could be shifted right / left (format.c:214-222)
				int z, y = q_off;
				for (z = 1; z <= len; ++z) if (y - z < 0 || qs[y + len - z] != qs[y - z]) break;
				const int lr = z - 1;
				for (z = 0; z < len; ++z) if (y + len + z >= q_len || qs[y + len + z] != qs[y + z]) break;
				put_ds_indel(o, len, qs + y, z, lr);
			} else put_bases(o, "acgtn", qs + q_off, len);
			q_off += len;
		} else if (op == 2) {
			o.ch('-');
			if (is_ds) {
				int z, x = t_off;
				for (z = 1; z <= len; ++z) if (x - z < 0 || ts[x + len - z] != ts[x - z]) break;
				const int lr = z - 1;
				for (z = 0; z < len; ++z) if (x + len + z >= t_len || ts[x + z] != ts[x + len + z]) break;
				put_ds_indel(o, len, ts + x, z, lr);
			} else put_bases(o, "acgtn", ts + t_off, len);
			t_off += len;
		} else { // intron: its first and last two bases
			o.ch('~'), o.ch("acgtn"[ts[t_off]]), o.ch("acgtn"[ts[t_off + 1]]), o.num(len), o.ch("acgtn"[ts[t_off + len - 2]]), o.ch("acgtn"[ts[t_off + len - 1]]);
			t_off += len;
		}
	}
}

void put_md(Text &o, const Reg1 &r, const Seqs &sq) // write_MD_core
{
	const uint8_t *qs = sq.q.data(), *ts = sq.t.data();
	o.str("\tMD:Z:");
	int q_off = 0, t_off = 0, l_md = 0;
	for (uint32_t i = 0; i < r.p->n_cigar; ++i) {
		const int op = r.p->cigar[i] & 0xf, len = r.p->cigar[i] >> 4;
		if (op == 0 || op == 7 || op == 8) {
			for (int j = 0; j < len; ++j) {
				if (qs[q_off + j] != ts[t_off + j]) o.num(l_md), o.ch("ACGTN"[ts[t_off + j]]), l_md = 0;
				else ++l_md;
			}
			q_off += len, t_off += len;
		} else if (op == 1) q_off += len;
		else if (op == 2) o.num(l_md), o.ch('^'), put_bases(o, "ACGTN", ts + t_off, len), l_md = 0, t_off += len;
		else if (op == 3) t_off += len;
	}
	if (l_md > 0) o.num(l_md);
}

void put_cs_or_md(Text &o, const FlatIndex &fi, const Bseq1 &t, const Reg1 &r, int64_t flag, Seqs &sq)
{
	if (!r.p) return;
	fetch_pair(fi, t, r, sq, (flag & F_QSTRAND) != 0);
	if (flag & F_OUT_MD) put_md(o, r, sq);
	else put_cs(o, r, sq, !(flag & F_OUT_CS_LONG), flag & F_OUT_DS);
}

void put_paf(Text &o, const FlatIndex &fi, const Bseq1 &t, const Reg1 *r, int64_t flag, int rep_len, int n_seg, int seg_idx, Seqs &sq) // mm_write_paf4
{
	o.str(t.name);
	if ((flag & F_FRAG_MODE) && n_seg >= 2 && seg_idx >= 0) o.ch('/'), o.num(seg_idx + 1);
	if (!r) {
		o.ch('\t'), o.num(t.l_seq), o.str("\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0");
		if (rep_len >= 0) o.tag("rl:i:", rep_len);
		return;
	}
	o.ch('\t'), o.num(t.l_seq), o.ch('\t'), o.num(r->qs), o.ch('\t'), o.num(r->qe), o.ch('\t'), o.ch("+-"[r->rev]), o.ch('\t');
	if (!fi.names[r->rid].empty()) o.str(fi.names[r->rid].c_str()); else o.num(r->rid);
	o.ch('\t'), o.num(fi.seq_len[r->rid]), o.ch('\t');
	if ((flag & F_QSTRAND) && r->rev) o.num((int)fi.seq_len[r->rid] - r->re), o.ch('\t'), o.num((int)fi.seq_len[r->rid] - r->rs); // format.c:440-443
	else o.num(r->rs), o.ch('\t'), o.num(r->re);
	o.ch('\t'), o.num(r->mlen), o.ch('\t'), o.num(r->blen), o.ch('\t'), o.num(r->mapq);
	put_tags(o, *r);
	if (rep_len >= 0) o.tag("rl:i:", rep_len);
	if (r->p && (flag & F_OUT_CG)) {
		o.str("\tcg:Z:");
		o.cigar(r->p->cigar, r->p->n_cigar);
	}
	if (r->p && (flag & (F_OUT_CS | F_OUT_DS | F_OUT_MD))) put_cs_or_md(o, fi, t, *r, flag, sq);
	if ((flag & F_COPY_COMMENT) && t.comment) o.ch('\t'), o.str(t.comment);
}

// --write-junc (map.c:601-607): the hits whose junctions are printed -- map.c's filter and the three tests of mm_write_junc (format.c:267-268)
bool junc_printable(const Reg1 &r)
{
	return r.id == r.parent && r.mapq >= 10 && r.is_spliced && r.p && (r.p->trans_strand == 1 || r.p->trans_strand == 2);
}
// an index mm_write_junc cannot print from (it would read a null name or no sequence)
void junc_index_check(const FlatIndex &fi)
{
	if (fi.flag & I_NO_NAME) throw std::invalid_argument("[mm2amd] --write-junc: the index holds no sequence names");
	if ((fi.flag & I_NO_SEQ) || !fi.S) throw std::invalid_argument("[mm2amd] --write-junc: the index holds no sequence");
}
// ... and a printable hit it cannot print (what the kernel indexes with; the CIGAR is the walk's business)
void junc_hit_check(const FlatIndex &fi, const Bseq1 &t, const Reg1 &r)
{
	if (!t.name) throw std::invalid_argument("[mm2amd] --write-junc: a read without a name");
	if (r.rid < 0 || (uint32_t)r.rid >= fi.n_seq || r.rs < 0 || r.rs > r.re || (uint32_t)r.re > fi.seq_len[r.rid])
		throw std::invalid_argument("[mm2amd] --write-junc: a hit lies outside its reference sequence");
}
const char kJuncBadCigar[] = "[mm2amd] --write-junc: a hit's CIGAR holds an intron shorter than 2, an unknown operation, or does not end at the hit's end";

// mm_write_junc (format.c:263-300) for a printable hit, every line with its \n (mm_err_puts).  The reference asserts an intron of at least 2 bases and a
// walk that ends at re: a CIGAR that breaks either is refused before a byte is written.
void put_junc(Text &o, const FlatIndex &fi, const Bseq1 &t, const Reg1 &r)
{
	junc_hit_check(fi, t, r);
	int64_t end = r.rs;
	bool bad = false;
	for (uint32_t i = 0; i < r.p->n_cigar; ++i) {
		const uint32_t op = r.p->cigar[i] & 0xf, len = r.p->cigar[i] >> 4;
		bad |= op > 9 || (op == 3 && len < 2);
		if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) end += len;
	}
	if (bad || end != r.re) throw std::invalid_argument(kJuncBadCigar);
	const bool rev = (r.p->trans_strand == 2) != (r.rev != 0);
	const std::string &tname = fi.names[r.rid];
	uint32_t t_off = (uint32_t)r.rs;
	for (uint32_t i = 0; i < r.p->n_cigar; ++i) {
		const uint32_t op = r.p->cigar[i] & 0xf, len = r.p->cigar[i] >> 4;
		if (op == 0 || op == 2 || op == 7 || op == 8) t_off += len;
		if (op != 3) continue;
		uint8_t donor[2], acceptor[2];
		if (!rev) fi.getseq(r.rid, t_off, t_off + 2, donor), fi.getseq(r.rid, t_off + len - 2, t_off + len, acceptor);
		else { // revcomp_splice (format.c:256-261) of the two ends, swapped
			uint8_t a[2], d[2];
			fi.getseq(r.rid, t_off, t_off + 2, a), fi.getseq(r.rid, t_off + len - 2, t_off + len, d);
			donor[0] = d[1] < 4 ? 3 - d[1] : 4, donor[1] = d[0] < 4 ? 3 - d[0] : 4;
			acceptor[0] = a[1] < 4 ? 3 - a[1] : 4, acceptor[1] = a[0] < 4 ? 3 - a[0] : 4;
		}
		const int score1 = donor[0] == 2 && donor[1] == 3 ? 3 : donor[0] == 2 && donor[1] == 1 ? 2 : donor[0] == 0 && donor[1] == 3 ? 1 : 0;
		const int score2 = acceptor[0] == 0 && acceptor[1] == 2 ? 3 : acceptor[0] == 0 && acceptor[1] == 1 ? 1 : 0;
		o.str(tname.data(), tname.size()), o.ch('\t'), o.num(t_off), o.ch('\t'), o.num(t_off + len), o.ch('\t'), o.str(t.name), o.ch('\t'), o.num(score1 + score2), o.ch('\t'),
			o.ch("+-"[rev]), o.ch('\n');
		t_off += len;
	}
}

#if defined(__x86_64__)
// Reverse complement, 16 bases per step, for blocks made of A/C/G/T/N in either case: the low nibbles of these five letters differ
// (1, 3, 7, 4, 14), so one byte shuffle maps a letter to its complement and another checks that the block holds nothing else.
static bool have_ssse3() { static const bool v = __builtin_cpu_supports("ssse3"); return v; }
__attribute__((target("ssse3"))) static int revcomp_blocks(const char *seq, int l, char *w)
{
	const __m128i rev = _mm_setr_epi8(15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0);
	const __m128i self = _mm_setr_epi8(0, 'A', 0, 'C', 'T', 0, 0, 'G', 0, 0, 0, 0, 0, 0, 'N', 0);
	const __m128i other = _mm_setr_epi8(0, 'T', 0, 'G', 'A', 0, 0, 'C', 0, 0, 0, 0, 0, 0, 'N', 0);
	const __m128i low = _mm_set1_epi8(0x0f), upper = _mm_set1_epi8((char)0xdf), lower_bit = _mm_set1_epi8(0x20);
	int i = 0;
	for (; i + 16 <= l; i += 16) {
		const __m128i v = _mm_shuffle_epi8(_mm_loadu_si128((const __m128i *)(seq + l - 16 - i)), rev);
		const __m128i nib = _mm_and_si128(v, low), up = _mm_and_si128(v, upper);
		if (_mm_movemask_epi8(_mm_cmpeq_epi8(_mm_shuffle_epi8(self, nib), up)) != 0xffff) break;
		_mm_storeu_si128((__m128i *)(w + i), _mm_or_si128(_mm_shuffle_epi8(other, nib), _mm_and_si128(v, lower_bit)));
	}
	return i;
}
#endif

void seq_into(char *w, const char *seq, int l, bool rev, bool comp) // sam_write_sq (format.c:470-482): l bytes at w
{
	static const std::array<char, 128> kComp = [] { // seq_comp_table (bseq.c:11-28) for ASCII: IUPAC complements, case preserved
		std::array<char, 128> t;
		for (int c = 0; c < 128; ++c) t[c] = (char)c;
		const char *a = "ACGTUMRWSYKVHDBNacgtumrwsykvhdbn", *b = "TGCAAKYWSRMBDHVNtgcaakywsrmbdhvn";
		for (int i = 0; a[i]; ++i) t[(int)a[i]] = b[i];
		return t;
	}();
	if (!rev) { memcpy(w, seq, (size_t)l); return; }
	if (comp) {
		int i = 0;
#if defined(__x86_64__)
		if (have_ssse3()) i = revcomp_blocks(seq, l, w); // whole 16-base blocks of plain A/C/G/T/N (either case); stops at the first block holding anything else
#endif
		for (; i < l; ++i) { const int c = (unsigned char)seq[l - 1 - i]; w[i] = c < 128 ? kComp[c] : (char)c; }
	}
	else for (int i = 0; i < l; ++i) w[i] = seq[l - 1 - i];
}
void put_seq(Text &o, const char *seq, int l, bool rev, bool comp)
{
	seq_into(o.need((size_t)l), seq, l, rev, comp);
	o.n += (size_t)l;
}

void put_sam_cigar(Text &o, int sam_flag, bool in_tag, int qlen, const Reg1 &r, int64_t flag) // write_sam_cigar (format.c:494-520)
{
	if (!r.p) { o.ch('*'); return; }
	const uint32_t clip0 = r.rev ? qlen - r.qe : r.qs, clip1 = r.rev ? r.qs : qlen - r.qe;
	const bool hard = ((sam_flag & 0x800) || ((sam_flag & 0x100) && (flag & F_SECONDARY_SEQ))) && !(flag & F_SOFTCLIP);
	if (in_tag) {
		const uint32_t op = hard ? 5 : 4;
		o.str("\tCG:B:I");
		if (clip0) o.ch(','), o.num(clip0 << 4 | op);
		for (uint32_t k = 0; k < r.p->n_cigar; ++k) o.ch(','), o.num(r.p->cigar[k]);
		if (clip1) o.ch(','), o.num(clip1 << 4 | op);
	} else {
		const char c = hard ? 'H' : 'S';
		if (clip0) o.num(clip0), o.ch(c);
		o.cigar(r.p->cigar, r.p->n_cigar);
		if (clip1) o.num(clip1), o.ch(c);
	}
}

// mm_write_sam3 for a single-segment read: reg_idx < 0 writes the unmapped record
const Reg1 *sam_primary(int n_regs, const Reg1 *regs) // get_sam_pri (format.c:484-492)
{
	for (int i = 0; i < n_regs; ++i) if (regs[i].sam_pri) return &regs[i];
	return nullptr;
}

// mm_write_sam3 (format.c:522-700) for fragments of one or two segments
void put_sam(Text &o, const FlatIndex &fi, const Bseq1 &t, int seg_idx, int reg_idx, int n_seg, const int *n_regss, void *const *regss, int64_t flag, int rep_len, Seqs &sq)
{
	const int n_regs = n_regss[seg_idx];
	const Reg1 *regs = (const Reg1 *)regss[seg_idx];
	const Reg1 *r = n_regs > 0 && reg_idx >= 0 && reg_idx < n_regs ? &regs[reg_idx] : nullptr;
	const Reg1 *r_next = nullptr, *r_prev = nullptr; // the mate's primary, if it is mapped
	if (n_seg > 1) {
		const int next_sid = (seg_idx + 1) % n_seg;
		r_prev = r_next = sam_primary(n_regss[next_sid], (const Reg1 *)regss[next_sid]);
	}
	if (n_seg > 1) { // the name without a /1 or /2 suffix (mm_qname_len, bseq.h:31-36)
		size_t l = strlen(t.name);
		if (l >= 3 && t.name[l - 1] >= '0' && t.name[l - 1] <= '9' && t.name[l - 2] == '/') l -= 2;
		for (size_t i = 0; i < l; ++i) o.ch(t.name[i]);
	} else o.str(t.name);
	int sf = n_seg > 1 ? 0x1 : 0x0;
	if (!r) sf |= 0x4;
	else {
		if (r->rev) sf |= 0x10;
		if (r->parent != r->id) sf |= 0x100;
		else if (!r->sam_pri) sf |= 0x800;
	}
	if (n_seg > 1) {
		if (r && r->proper_frag) sf |= 0x2;
		if (seg_idx == 0) sf |= 0x40;
		else if (seg_idx == n_seg - 1) sf |= 0x80;
		if (!r_next) sf |= 0x8;
		else if (r_next->rev) sf |= 0x20;
	}
	int this_rid = -1, this_pos = -1;
	o.ch('\t'), o.num(sf);
	bool cigar_in_tag = false;
	if (!r) {
		if (r_prev) { // an unmapped read is placed at its mate's position
			this_rid = r_prev->rid, this_pos = r_prev->rs;
			o.ch('\t'), o.str(fi.names[this_rid].c_str()), o.ch('\t'), o.num(this_pos + 1), o.str("\t0\t*");
		} else o.str("\t*\t0\t0\t*");
	} else {
		this_rid = r->rid, this_pos = r->rs;
		o.ch('\t'), o.str(fi.names[r->rid].c_str()), o.ch('\t'), o.num(r->rs + 1), o.ch('\t'), o.num(r->mapq), o.ch('\t');
		if ((flag & F_LONG_CIGAR) && r->p && r->p->n_cigar > 65535 - 2) {
			int n_cigar = (int)r->p->n_cigar;
			if (r->qs != 0) ++n_cigar;
			if (r->qe != t.l_seq) ++n_cigar;
			cigar_in_tag = n_cigar > 65535;
		}
		if (cigar_in_tag) {
			int slen;
			if ((sf & 0x900) == 0 || (flag & F_SOFTCLIP)) slen = t.l_seq;
			else if ((sf & 0x100) && !(flag & F_SECONDARY_SEQ)) slen = 0;
			else slen = r->qe - r->qs;
			o.num(slen), o.ch('S'), o.num(r->re - r->rs), o.ch('N');
		} else put_sam_cigar(o, sf, false, t.l_seq, *r, flag);
	}
	if (n_seg > 1) { // mate position and template length (format.c:592-613)
		int tlen = 0;
		if (this_rid >= 0 && r_next) {
			if (this_rid == r_next->rid) {
				if (r) {
					const int this_pos5 = r->rev ? r->re - 1 : this_pos, next_pos5 = r_next->rev ? r_next->re - 1 : r_next->rs;
					tlen = next_pos5 - this_pos5;
				}
				o.str("\t=\t");
			} else o.ch('\t'), o.str(fi.names[r_next->rid].c_str()), o.ch('\t');
			o.num(r_next->rs + 1), o.ch('\t');
		} else if (r_next) o.ch('\t'), o.str(fi.names[r_next->rid].c_str()), o.ch('\t'), o.num(r_next->rs + 1), o.ch('\t');
		else if (this_rid >= 0) o.str("\t=\t"), o.num(this_pos + 1), o.ch('\t');
		else o.str("\t*\t0\t");
		if (tlen > 0) ++tlen;
		else if (tlen < 0) --tlen;
		o.num(tlen), o.ch('\t');
	} else o.str("\t*\t0\t0\t"); // no mate
	if (!r) {
		put_seq(o, t.seq, t.l_seq, false, false), o.ch('\t');
		if (t.qual) put_seq(o, t.qual, t.l_seq, false, false); else o.ch('*');
	} else if ((sf & 0x900) == 0 || (flag & F_SOFTCLIP)) {
		put_seq(o, t.seq, t.l_seq, r->rev, r->rev), o.ch('\t');
		if (t.qual) put_seq(o, t.qual, t.l_seq, r->rev, false); else o.ch('*');
	} else if ((sf & 0x100) && !(flag & F_SECONDARY_SEQ)) o.str("*\t*");
	else {
		put_seq(o, t.seq + r->qs, r->qe - r->qs, r->rev, r->rev), o.ch('\t');
		if (t.qual) put_seq(o, t.qual + r->qs, r->qe - r->qs, r->rev, false); else o.ch('*');
	}
	if (r) {
		put_tags(o, *r);
		if (r->parent == r->id && r->p && n_regs > 1) { // supplementary alignments of the same read (format.c:638-664)
			int n_sa = 0;
			for (int i = 0; i < n_regs; ++i) if (i != reg_idx && regs[i].parent == regs[i].id && regs[i].p) ++n_sa;
			if (n_sa > 0) {
				o.str("\tSA:Z:");
				for (int i = 0; i < n_regs; ++i) {
					const Reg1 &q = regs[i];
					if (i == reg_idx || q.parent != q.id || !q.p) continue;
					int l_M, l_I = 0, l_D = 0;
					if (q.qe - q.qs < q.re - q.rs) l_M = q.qe - q.qs, l_D = (q.re - q.rs) - l_M;
					else l_M = q.re - q.rs, l_I = (q.qe - q.qs) - l_M;
					const int clip5 = q.rev ? t.l_seq - q.qe : q.qs, clip3 = q.rev ? q.qs : t.l_seq - q.qe;
					o.str(fi.names[q.rid].c_str()), o.ch(','), o.num(q.rs + 1), o.ch(','), o.ch("+-"[q.rev]), o.ch(',');
					if (clip5) o.num(clip5), o.ch('S');
					if (l_M) o.num(l_M), o.ch('M');
					if (l_I) o.num(l_I), o.ch('I');
					if (l_D) o.num(l_D), o.ch('D');
					if (clip3) o.num(clip3), o.ch('S');
					o.ch(','), o.num(q.mapq), o.ch(','), o.num(q.blen - q.mlen + (int)q.p->n_ambi), o.ch(';');
				}
			}
		}
		if (r->p && (flag & (F_OUT_CS | F_OUT_DS | F_OUT_MD))) put_cs_or_md(o, fi, t, *r, flag, sq);
		if (cigar_in_tag) put_sam_cigar(o, sf, true, t.l_seq, *r, flag);
	}
	if (rep_len >= 0) o.tag("rl:i:", rep_len);
	if ((flag & F_COPY_COMMENT) && t.comment) o.ch('\t'), o.str(t.comment);
}

} // namespace

std::string format_check(const MapOpt &opt)
{
	if (opt.split_prefix) return "split-index output is not implemented";
	return "";
}

// the records of fragments [lo, hi), in order (map.c:585-623)
// mm2amd_format_fraction (diagnostics, include/mm2amd.h): "%.4f" as the output stage writes it
int format_fraction_for_test(double v, char *buf)
{
	Text t;
	put_fraction(t, v);
	memcpy(buf, t.data(), t.size());
	buf[t.size()] = 0;
	return (int)t.size();
}

static void format_range(const FlatIndex &fi, const MapOpt &opt, const int *seg_off, const int *n_seg, const Bseq1 *seq, const int *n_reg, void *const *reg,
                         const int *rep_len, long lo, long hi, Text &o)
{
	Seqs sq;
	const int64_t flag = opt.flag;
	hostprof::Scope hp(hostprof::FORMAT_RANGE);
	o.gaps = Text::GapCount(); // (the gap counts kept from a record's CIGAR text are only good while the batch's blocks are alive)
	for (long f = lo; f < hi; ++f) {
		const int seg_st = seg_off ? seg_off[f] : (int)f, ns = n_seg ? n_seg[f] : 1;
		for (int i = seg_st; i < seg_st + ns; ++i) {
			const Bseq1 &t = seq[i];
			const Reg1 *regs = (const Reg1 *)reg[i];
			const int rl = rep_len ? rep_len[i] : -1;
			if (flag & F_OUT_JUNC) { // --write-junc (map.c:601-607): ahead of the SAM / PAF branches, the other output flags play no part
				for (int j = 0; j < n_reg[i]; ++j) if (junc_printable(regs[j])) put_junc(o, fi, t, regs[j]);
			} else if (n_reg[i] > 0) {
				for (int j = 0; j < n_reg[i]; ++j) {
					if ((flag & F_NO_PRINT_2ND) && regs[j].id != regs[j].parent) continue;
					if (flag & F_OUT_SAM) put_sam(o, fi, t, i - seg_st, j, ns, &n_reg[seg_st], &reg[seg_st], flag, rl, sq);
					else put_paf(o, fi, t, &regs[j], flag, rl, ns, i - seg_st, sq);
					o.ch('\n');
				}
			} else if ((flag & F_PAF_NO_HIT) || ((flag & F_OUT_SAM) && !(flag & F_SAM_HIT_ONLY))) {
				if (flag & F_OUT_SAM) put_sam(o, fi, t, i - seg_st, -1, ns, &n_reg[seg_st], &reg[seg_st], flag, rl, sq);
				else put_paf(o, fi, t, nullptr, flag, rl, ns, i - seg_st, sq);
				o.ch('\n');
			}
		}
	}
}

struct FormatScratch::Impl { std::vector<Text> parts; };
FormatScratch::FormatScratch() : impl(new Impl) {}
FormatScratch::~FormatScratch() { delete impl; free(buf); }

// the chunks' texts (64 fragments each, formatted by one pool thread each) and where each starts in the concatenation
static size_t format_parts(const FlatIndex &fi, const MapOpt &opt, int n_threads, long n, const int *seg_off, const int *n_seg, const Bseq1 *seq, const int *n_reg,
                           void *const *reg, const int *rep_len, std::vector<Text> &parts, std::vector<size_t> &off)
{
	const long chunk = 64, n_chunks = (n + chunk - 1) / chunk;
	if (opt.flag & F_OUT_JUNC) junc_index_check(fi);
	if ((long)parts.size() < n_chunks) parts.resize(n_chunks);
	static const bool trace = getenv("MM2AMD_FMT_TRACE") != nullptr;
	const auto t0 = std::chrono::steady_clock::now();
	std::atomic<long long> busy_ns{0};
	parallel_for_side(n_threads, n_chunks, [&](long c, int) {
		const auto c0 = std::chrono::steady_clock::now();
		const long lo = c * chunk, hi = std::min(n, lo + chunk);
		parts[c].clear(); // keeps its capacity: a reused scratch formats into memory it already owns
		format_range(fi, opt, seg_off, n_seg, seq, n_reg, reg, rep_len, lo, hi, parts[c]);
		if (trace) busy_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - c0).count();
	}, 1);
	if (trace) fprintf(stderr, "[mm2amd] format: %ld chunks, wall %.3f s, summed chunk time %.3f s on %d threads\n", n_chunks,
	                   std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), busy_ns.load() * 1e-9, n_threads);
	off.assign(n_chunks + 1, 0);
	for (long c = 0; c < n_chunks; ++c) off[c + 1] = off[c] + parts[c].size();
	return off[n_chunks];
}

char *format_batch(const FlatIndex &fi, const MapOpt &opt, int n_threads, long n_frag, const int *seg_off, const int *n_seg, const Bseq1 *seq, const int *n_reg,
                   void *const *reg, const int *rep_len, size_t *out_len)
{
	std::vector<Text> parts;
	std::vector<size_t> off;
	const size_t total = format_parts(fi, opt, n_threads, n_frag, seg_off, n_seg, seq, n_reg, reg, rep_len, parts, off);
	char *out = (char *)malloc(total + 1);
	if (!out) return nullptr;
	parallel_for_side(n_threads, (long)off.size() - 1, [&](long c, int) { memcpy(out + off[c], parts[c].data(), parts[c].size()); }, 8);
	out[total] = 0;
	*out_len = total;
	return out;
}

const char *format_batch_view(const FlatIndex &fi, const MapOpt &opt, int n_threads, long n_frag, const int *seg_off, const int *n_seg, const Bseq1 *seq, const int *n_reg,
                              void *const *reg, const int *rep_len, FormatScratch &fs, size_t *out_len)
{
	std::vector<size_t> off;
	const size_t total = format_parts(fi, opt, n_threads, n_frag, seg_off, n_seg, seq, n_reg, reg, rep_len, fs.impl->parts, off);
	if (fs.cap < total + 1) { // grow-only: in the steady state of a pipeline no page of this buffer is new
		free(fs.buf);
		fs.cap = (total + 1) + (total + 1) / 4;
		fs.buf = (char *)malloc(fs.cap);
		if (!fs.buf) { fs.cap = 0; return nullptr; }
	}
	parallel_for_side(n_threads, (long)off.size() - 1, [&](long c, int) { memcpy(fs.buf + off[c], fs.impl->parts[c].data(), fs.impl->parts[c].size()); }, 8);
	fs.buf[total] = 0;
	*out_len = total;
	return fs.buf;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The same text with the records written on the device (rec_text.hpp).  The planner below decides which records a batch prints and in which
// order (format_range's rules), fills one RecJob per record and one RecHit per hit, gathers the CIGARs, the read names and -- for cs / MD --
// the reads' [qs, qe) letters into the backend's pinned buffers; the backend runs the sizing pass, the host turns the lengths into 64-bit
// offsets, the backend runs the writing pass and brings the text back.  SEQ and QUAL of a SAM record are a hole in that text: the pool copies
// every record's two pieces around put_seq's bytes into the final buffer.
// ---------------------------------------------------------------------------------------------------------------------------------------
namespace {

struct DevRec { int read, j; }; // a record: the read and its hit (-1: none)

int sam_flag_of(const Reg1 *r) // mm_write_sam3's FLAG for a single-segment read
{
	if (!r) return 0x4;
	int sf = r->rev ? 0x10 : 0;
	if (r->parent != r->id) sf |= 0x100;
	else if (!r->sam_pri) sf |= 0x800;
	return sf;
}
// the hole of a SAM record, SEQ \t QUAL (format.c:617-634): 0 = whole read, 1 = "*\t*", 2 = [qs, qe)
int hole_kind(const Reg1 *r, int64_t flag)
{
	const int sf = sam_flag_of(r);
	if (!r || (sf & 0x900) == 0 || (flag & F_SOFTCLIP)) return 0;
	return (sf & 0x100) && !(flag & F_SECONDARY_SEQ) ? 1 : 2;
}
size_t hole_len(const Bseq1 &t, const Reg1 *r, int64_t flag)
{
	const int k = hole_kind(r, flag);
	if (k == 1) return 3;
	const size_t l = k == 0 ? (size_t)t.l_seq : (size_t)(r->qe - r->qs);
	return l + 1 + (t.qual ? l : 1);
}
char *hole_into(char *w, const Bseq1 &t, const Reg1 *r, int64_t flag)
{
	const int k = hole_kind(r, flag);
	if (k == 1) { memcpy(w, "*\t*", 3); return w + 3; }
	const bool rev = r && r->rev;
	const int st = k == 0 ? 0 : r->qs, l = k == 0 ? t.l_seq : r->qe - r->qs;
	seq_into(w, t.seq + st, l, rev, rev), w += l, *w++ = '\t';
	if (t.qual) seq_into(w, t.qual + st, l, rev, false), w += l; else *w++ = '*';
	return w;
}

// --write-junc on the device (junc_text.hpp): a job and a hit per printable hit, in format_range's order; the kernel's sizing pass judges the CIGARs
const char *format_junc_dev(Backend &be, const FlatIndex &fi, const MapOpt &opt, int n_threads, long n_frag, const int *seg_off, const int *n_seg, const Bseq1 *seq,
                            const int *n_reg, void *const *reg, FormatScratch &fs, size_t *out_len)
{
	junc_index_check(fi);
	struct JuncPlan { int read, j; bool first; uint64_t name_off, cig_off; }; // first: the first printable hit of its read copies the name
	std::vector<JuncPlan> plan;
	Backend::RecTextSizes sz;
	for (long f = 0; f < n_frag; ++f) {
		const int seg_st = seg_off ? seg_off[f] : (int)f, ns = n_seg ? n_seg[f] : 1;
		for (int i = seg_st; i < seg_st + ns; ++i) {
			const Reg1 *regs = (const Reg1 *)reg[i];
			bool first = true;
			for (int j = 0; j < n_reg[i]; ++j) {
				if (!junc_printable(regs[j])) continue;
				junc_hit_check(fi, seq[i], regs[j]);
				plan.push_back(JuncPlan{ i, j, first, sz.name_bytes, sz.cigar_words });
				sz.cigar_words += regs[j].p->n_cigar, first = false;
			}
			if (!first) sz.name_bytes += strlen(seq[i].name);
		}
	}
	sz.n_jobs = sz.n_hits = plan.size();
	if (sz.n_jobs > 0x7fffffffull) throw std::invalid_argument("[mm2amd] --write-junc: too many hits in one batch");
	const Backend::RecTextBufs B = be.rec_text_begin(sz);
	const long chunk = 256, n_chunks = ((long)sz.n_jobs + chunk - 1) / chunk;
	parallel_for_side(n_threads, n_chunks, [&](long c, int) {
		for (size_t k = (size_t)(c * chunk); k < std::min(sz.n_jobs, (size_t)((c + 1) * chunk)); ++k) {
			const JuncPlan &pl = plan[k];
			const Bseq1 &t = seq[pl.read];
			const Reg1 &r = ((const Reg1 *)reg[pl.read])[pl.j];
			const uint32_t name_len = (uint32_t)strlen(t.name);
			if (pl.first) memcpy(B.names + pl.name_off, t.name, name_len);
			RecHit &h = B.hits[k];
			memset(&h, 0, sizeof h);
			h.rid = r.rid, h.rs = r.rs, h.re = r.re, h.qs = r.qs, h.qe = r.qe, h.n_cigar = r.p->n_cigar, h.cig_off = pl.cig_off, h.t_pos = fi.seq_off[r.rid];
			h.bits = r.mapq | (r.rev ? kRecRev : 0u) | kRecHasP | kRecIsParent | kRecIsSpliced | (uint32_t)r.p->trans_strand << kRecTransShift;
			memcpy(B.cigar + pl.cig_off, r.p->cigar, (size_t)r.p->n_cigar * 4);
			RecJob &J = B.jobs[k];
			J.name_off = pl.name_off, J.name_len = name_len, J.l_seq = t.l_seq, J.rep_len = -1, J.hit = (int32_t)k, J.hit0 = (uint32_t)k, J.n_hits = 1;
		}
	}, 1);
	const RecRes *res = be.junc_text_size(opt.flag);
	uint64_t total = 0;
	for (size_t k = 0; k < sz.n_jobs; ++k) {
		if (res[k].status != kRecOk) throw std::invalid_argument(kJuncBadCigar);
		B.off[k] = total, total += res[k].len;
	}
	const char *text = be.junc_text_write(total);
	if (fs.cap < total + 1) { // grow-only, as format_batch_view
		free(fs.buf);
		fs.cap = (total + 1) + (total + 1) / 4;
		fs.buf = (char *)malloc(fs.cap);
		if (!fs.buf) { fs.cap = 0; return nullptr; }
	}
	if (total) memcpy(fs.buf, text, total);
	fs.buf[total] = 0;
	*out_len = total;
	return fs.buf;
}

} // namespace

const char *format_batch_dev(Backend &be, const FlatIndex &fi, const MapOpt &opt, int n_threads, long n_frag, const int *seg_off, const int *n_seg, const Bseq1 *seq,
                             const int *n_reg, void *const *reg, const int *rep_len, FormatScratch &fs, size_t *out_len, bool *on_device)
{
	const int64_t flag = opt.flag;
	const bool sam = (flag & F_OUT_SAM) != 0, per_base = (flag & (F_OUT_CS | F_OUT_MD)) != 0, qstrand = (flag & F_QSTRAND) != 0;
	auto host = [&]() { *on_device = false; return format_batch_view(fi, opt, n_threads, n_frag, seg_off, n_seg, seq, n_reg, reg, rep_len, fs, out_len); };
	*on_device = true;
	if (flag & F_OUT_JUNC) { // junction records do not depend on the mate: fragments of one and of two segments are the device's
		if (!be.writes_records()) return host();
		return format_junc_dev(be, fi, opt, n_threads, n_frag, seg_off, n_seg, seq, n_reg, reg, fs, out_len);
	}
	if (!be.writes_records() || (flag & F_OUT_DS)) return host();
	if (per_base && ((fi.flag & ref::I_NO_SEQ) || !fi.S)) return host(); // cs / MD of an index without sequence
	if (n_seg) for (long f = 0; f < n_frag; ++f) if (n_seg[f] != 1) return host();

	// pass 1: the records, and where every read's share of the pools starts
	struct ReadPlan { uint32_t hit0; uint64_t job0, name_off, cig_off, q_off; };
	std::vector<ReadPlan> plan((size_t)n_frag);
	std::vector<DevRec> recs;
	Backend::RecTextSizes sz;
	for (long f = 0; f < n_frag; ++f) {
		const int i = seg_off ? seg_off[f] : (int)f;
		const Bseq1 &t = seq[i];
		const Reg1 *regs = (const Reg1 *)reg[i];
		ReadPlan &pl = plan[f];
		pl.hit0 = (uint32_t)sz.n_hits, pl.job0 = recs.size(), pl.name_off = sz.name_bytes, pl.cig_off = sz.cigar_words, pl.q_off = sz.q_bytes;
		if ((flag & F_COPY_COMMENT) && t.comment) return host();
		if (t.l_seq < 0 || !t.name || (t.l_seq > 0 && !t.seq)) return host();
		if (n_reg[i] > 0) {
			for (int j = 0; j < n_reg[i]; ++j) {
				const Reg1 &r = regs[j];
				// (what the kernel indexes with: a record the host writer would have to refuse as well goes to it)
				if (r.rid < 0 || (uint32_t)r.rid >= fi.n_seq || r.rs < 0 || r.rs > r.re || (uint32_t)r.re > fi.seq_len[r.rid] || r.qs < 0 || r.qs > r.qe || r.qe > t.l_seq) return host();
				if ((flag & F_NO_PRINT_2ND) && r.id != r.parent) continue;
				if (sam && (flag & F_LONG_CIGAR) && r.p && r.p->n_cigar > 65535 - 2 && (int)r.p->n_cigar + (r.qs != 0) + (r.qe != t.l_seq) > 65535) return host(); // CG:B:I
				recs.push_back(DevRec{ (int)f, j });
				if (r.p) sz.cigar_words += r.p->n_cigar, sz.q_bytes += per_base ? (size_t)(r.qe - r.qs) : 0;
			}
			sz.n_hits += (size_t)n_reg[i];
		} else if ((flag & F_PAF_NO_HIT) || (sam && !(flag & F_SAM_HIT_ONLY))) recs.push_back(DevRec{ (int)f, -1 });
		if (recs.size() > pl.job0) sz.name_bytes += strlen(t.name);
	}
	sz.n_jobs = recs.size();
	if (sz.n_jobs > 0x7fffffffull || sz.n_hits > 0x7fffffffull) return host();

	// pass 2: the table and the pools, in the backend's pinned memory
	const Backend::RecTextBufs B = be.rec_text_begin(sz);
	const long chunk = 64, n_chunks = (n_frag + chunk - 1) / chunk;
	parallel_for_side(n_threads, n_chunks, [&](long c, int) {
		for (long f = c * chunk; f < std::min(n_frag, (c + 1) * chunk); ++f) {
			const int i = seg_off ? seg_off[f] : (int)f;
			const Bseq1 &t = seq[i];
			const Reg1 *regs = (const Reg1 *)reg[i];
			const ReadPlan &pl = plan[f];
			const uint64_t job_end = f + 1 < n_frag ? plan[f + 1].job0 : recs.size();
			if (job_end == pl.job0) continue;
			const uint32_t name_len = (uint32_t)strlen(t.name);
			memcpy(B.names + pl.name_off, t.name, name_len);
			uint64_t cig = pl.cig_off, qo = pl.q_off;
			const int n_hits = n_reg[i] > 0 ? n_reg[i] : 0;
			uint64_t job = pl.job0;
			for (int j = 0; j < n_hits; ++j) {
				const Reg1 &r = regs[j];
				RecHit &h = B.hits[pl.hit0 + j];
				memset(&h, 0, sizeof h);
				h.rid = r.rid, h.rs = r.rs, h.re = r.re, h.qs = r.qs, h.qe = r.qe, h.mlen = r.mlen, h.blen = r.blen, h.cnt = r.cnt, h.score = r.score, h.subsc = r.subsc, h.div = r.div;
				h.bits = r.mapq | (uint32_t)r.split << kRecSplitShift | (r.rev ? kRecRev : 0u) | (r.inv ? kRecInv : 0u) | (r.sam_pri ? kRecSamPri : 0u) | (r.p ? kRecHasP : 0u) |
				         (r.id == r.parent ? kRecIsParent : 0u) | (r.is_spliced ? kRecIsSpliced : 0u);
				if (r.p) h.dp_max0 = r.p->dp_max0, h.dp_score = r.p->dp_score, h.n_ambi = r.p->n_ambi, h.bits |= (uint32_t)r.p->trans_strand << kRecTransShift;
				const bool printed = job < job_end && recs[job].j == j;
				if (!printed) continue;
				RecJob &J = B.jobs[job];
				J.name_off = pl.name_off, J.name_len = name_len, J.l_seq = t.l_seq, J.rep_len = rep_len ? rep_len[i] : -1, J.hit = (int32_t)(pl.hit0 + j), J.hit0 = pl.hit0, J.n_hits = (uint32_t)n_hits;
				++job;
				if (!r.p) continue;
				h.n_cigar = r.p->n_cigar, h.cig_off = cig;
				memcpy(B.cigar + cig, r.p->cigar, (size_t)r.p->n_cigar * 4), cig += r.p->n_cigar;
				if (!per_base) continue;
				const uint64_t so = fi.seq_off[r.rid];
				h.q_pos = qo;
				memcpy(B.q + qo, t.seq + r.qs, (size_t)(r.qe - r.qs)), qo += (uint64_t)(r.qe - r.qs);
				if (qstrand) { // format.c:343-346: mm_idx_getseq2's window, the read as it is
					h.qsrc = (uint8_t)kTxtQAscii, h.tsrc = (uint8_t)(r.rev ? kTxtTPackedRev : kTxtTPacked);
					h.t_pos = r.rev ? so + (fi.seq_len[r.rid] - (uint32_t)r.re) : so + (uint32_t)r.rs;
				} else h.qsrc = (uint8_t)(r.rev ? kTxtQAsciiRev : kTxtQAscii), h.tsrc = (uint8_t)kTxtTPacked, h.t_pos = so + (uint32_t)r.rs; // format.c:347-358
			}
			if (n_hits == 0) {
				RecJob &J = B.jobs[job];
				J.name_off = pl.name_off, J.name_len = name_len, J.l_seq = t.l_seq, J.rep_len = rep_len ? rep_len[i] : -1, J.hit = -1, J.hit0 = pl.hit0, J.n_hits = 0;
			}
		}
	}, 1);

	const RecRes *res = be.rec_text_size(flag);
	uint64_t dev_total = 0;
	std::vector<uint64_t> at(sz.n_jobs + 1, 0); // where every record starts in the final text
	for (size_t k = 0; k < sz.n_jobs; ++k) {
		if (res[k].status != kRecOk) return host(); // a fraction outside [0, 1], or operations the walk refuses
		B.off[k] = dev_total, dev_total += res[k].len;
		const DevRec &d = recs[k];
		const int i = seg_off ? seg_off[d.read] : d.read;
		at[k + 1] = at[k] + res[k].len + (sam ? hole_len(seq[i], d.j < 0 ? nullptr : (const Reg1 *)reg[i] + d.j, flag) : 0);
	}
	const char *text = be.rec_text_write(dev_total);
	const size_t total = at[sz.n_jobs];
	if (fs.cap < total + 1) { // grow-only, as format_batch_view
		free(fs.buf);
		fs.cap = (total + 1) + (total + 1) / 4;
		fs.buf = (char *)malloc(fs.cap);
		if (!fs.buf) { fs.cap = 0; return nullptr; }
	}
	const long rchunk = 256, n_rchunks = ((long)sz.n_jobs + rchunk - 1) / rchunk;
	parallel_for_side(n_threads, n_rchunks, [&](long c, int) {
		const size_t lo = (size_t)(c * rchunk), hi = std::min(sz.n_jobs, lo + (size_t)rchunk);
		if (!sam) { memcpy(fs.buf + at[lo], text + B.off[lo], at[hi] - at[lo]); return; } // PAF: no hole
		for (size_t k = lo; k < hi; ++k) {
			const DevRec &d = recs[k];
			const int i = seg_off ? seg_off[d.read] : d.read;
			const char *src = text + B.off[k];
			char *w = fs.buf + at[k];
			memcpy(w, src, res[k].before), w += res[k].before;
			w = hole_into(w, seq[i], d.j < 0 ? nullptr : (const Reg1 *)reg[i] + d.j, flag);
			memcpy(w, src + res[k].before, res[k].len - res[k].before);
		}
	}, 1);
	fs.buf[total] = 0;
	*out_len = total;
	return fs.buf;
}

} // namespace mm2amd
