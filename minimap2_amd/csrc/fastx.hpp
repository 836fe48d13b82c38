// FASTA / FASTQ text into sequence records: what kseq_read (kseq.h:192-232) + kseq2bseq (bseq.c:65-78) make of a file, over a buffer in memory.
// DESIGN.md section 3h has the grammar, the incremental contract and the device's share (fastx_dev.hpp, compiled with index_build.hip); this header
// holds the host's parser -- the `device=False` route and the fallback of the device path -- and the host-side declarations of the kernels' launches.
//
// Both are formulated over LINES, not over a character stream.  A record is
//   a header: a marker byte ('>' or '@'), the name up to the first isspace byte, and, when that byte is not the line's '\n', the rest of the line
//             as the comment;
//   sequence lines: every following line whose first byte is none of '>', '@', '+' (empty lines contribute nothing);
//   for a line beginning with '+': that line, then quality lines until they hold at least as many bytes as the sequence (at least one line).
// A line's contribution to the string it is appended to loses one trailing CR iff the string, with the line appended, is longer than one byte.
// After a FASTQ-type record the next marker is looked for from the next line's start ANYWHERE in the text; after a FASTA-type record the
// next header is the line that ended it.  A quality of another length than the sequence, or a '+' line the text ends in, is a malformed record
// (kseq_read's -2): it is reported as a table entry with `reserved` = 1 and nothing else, because mm_bseq_read3 ends its batch there.
#pragma once
#include <cstdint>
#include <cstddef>
#include <cstring>
#include <vector>
#include <utility>
#include <hip/hip_runtime.h>
#include "../../include/mm2amd.h"

namespace mm2amd {

constexpr uint32_t kFastxTile = 4096;          // bytes of text a workgroup of fastx_lines_kernel takes: 256 lanes, one aligned 16-byte vector each
constexpr uint32_t kFastxLongLine = 4096;      // a sequence / quality line of at least this many payload bytes is copied by the long class
constexpr uint32_t kFastxLongChunk = 16384;    // bytes of a long line one workgroup of the long class copies
constexpr uint32_t kFastxShortLanes = 16;      // lanes that share a line in the short class
constexpr size_t kFastxMaxText = (size_t)1 << 30; // offsets and the pool's length stay below 2^31 in uint32

struct FastxDevRec { uint32_t name, name_len, comment_len, seq, l_seq; }; // a record as the kernels leave it: offsets into the pool (l_seq: FASTQ4 only)

struct FastxParams {
	const uint8_t *text;      // len bytes on the device, at the host buffer's alignment modulo 16
	uint32_t len, flags;
	int cls;                  // MM2AMD_FASTX_PATH_FASTQ4 or MM2AMD_FASTX_PATH_FASTA: what the buffer is validated as
	uint32_t n_tiles;         // tiles of kFastxTile bytes from the aligned address below `text`
	uint32_t *tile_cnt;       // n_tiles + 1: '\n' per tile, then their exclusive sum
	uint32_t n_nl, n_lines;   // '\n' in the text; lines the later stages look at (line i < n_nl ends in '\n', a last one beyond ends with the text)
	uint32_t *line_off;       // n_nl + 1: line i starts at line_off[i] (line_off[n_nl] may equal len: no such line then)
	uint32_t *dst;            // n_lines + 1: bytes line i contributes to the pool, then their exclusive sum
	uint32_t *ridx;           // FASTA, n_lines + 1: 1 for a header line, then the exclusive sum (a header's record index)
	uint32_t *name_len;       // n_lines: a header line's name length
	uint32_t *state;          // [0] violations of the class, [1] work items of the long class, [2] the last header line (FASTA)
	uint32_t long_line;       // the class threshold in force
	uint2 *work;              // (line, chunk) per work item
	uint32_t work_cap;
	uint32_t n_rec, pool_len;
	FastxDevRec *recs;
	uint8_t *pool;
};

void fastx_lines_launch(const FastxParams &P, bool write, void *stream);
void fastx_classify_launch(const FastxParams &P, void *stream);
void fastx_copy_launch(const FastxParams &P, bool long_class, uint32_t n_work, void *stream);

// ---- the host's parser ----

struct FastxSink { // the caller's table and pool; lengths keep counting beyond the capacities, nothing is written at or beyond them
	mm2amd_fastx_rec_t *recs;
	size_t recs_cap;
	char *pool;
	size_t pool_cap;
	size_t n_recs = 0, pool_len = 0;
	FastxSink(mm2amd_fastx_rec_t *r, size_t rc, char *p, size_t pc) : recs(r), recs_cap(r ? rc : 0), pool(p), pool_cap(p ? pc : 0) {}
	uint64_t put(const char *s, size_t n, bool u2t) // s[0, n) and a NUL
	{
		const uint64_t at = pool_len;
		if (pool_len + n + 1 <= pool_cap) {
			char *d = pool + pool_len;
			if (u2t) for (size_t i = 0; i < n; ++i) d[i] = (char)(s[i] - ((s[i] | 0x20) == 'u')); // U -> T, u -> t (bseq.c:72-74)
			else if (n) memcpy(d, s, n);
			d[n] = 0;
		}
		pool_len += n + 1;
		return at;
	}
	void append(const char *s, size_t n, bool u2t) // without the NUL; `pool_len` is the string's end
	{
		if (pool_len + n <= pool_cap) {
			char *d = pool + pool_len;
			if (u2t) for (size_t i = 0; i < n; ++i) d[i] = (char)(s[i] - ((s[i] | 0x20) == 'u'));
			else if (n) memcpy(d, s, n);
		}
		pool_len += n;
	}
	void nul() { if (pool_len + 1 <= pool_cap) pool[pool_len] = 0; ++pool_len; }
};

inline bool fastx_isspace(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); } // isspace of the C locale

// Records of text[0, len) into `out`; returns `consumed`, the offset of the first byte that belongs to no complete record (len for a final
// buffer).  In a non-final buffer a FASTA-type record is complete once the next header's first byte has been seen, a FASTQ-type record once its
// quality has reached the sequence's length on a line that '\n' ends, and every line a record uses has to end in '\n'.
inline size_t fastx_parse_host(const char *t, const size_t len, const bool fin, const int flags, FastxSink &out)
{
	typedef std::pair<size_t, size_t> Span;
	std::vector<Span> seq, qual;
	const auto line_end = [&](size_t b) -> size_t { const void *p = b < len ? memchr(t + b, '\n', len - b) : nullptr; return p ? (size_t)((const char *)p - t) : len; };
	size_t pos = 0;          // the next record is looked for from here
	bool at_header = false;  // t[pos] is a header's marker (the line that ended a FASTA-type record)
	for (;;) {
		size_t h = pos;
		if (!at_header) while (h < len && t[h] != '>' && t[h] != '@') ++h;
		if (h >= len) return fin ? len : pos;
		const size_t he = line_end(h);
		if (he == len && !fin) return h;
		if (h + 1 >= len) return len; // the text ends in a marker: no record (fin holds here)
		size_t q = h + 1;
		while (q < he && !fastx_isspace((unsigned char)t[q])) ++q;
		const size_t name_b = h + 1, name_n = q - name_b;
		size_t com_b = q, com_n = 0;
		if (q < he) { com_b = q + 1, com_n = he - com_b; if (com_n > 1 && t[he - 1] == '\r') --com_n; }
		// the sequence lines
		seq.clear(), qual.clear();
		size_t l_seq = 0, l_qual = 0, cur = he < len ? he + 1 : len;
		int stop = 0; // what ended them: 0 the text, else the byte
		for (;;) {
			if (cur >= len) { if (!fin) return h; break; }
			const char c = t[cur];
			if (c == '\n') { ++cur; continue; }
			if (c == '>' || c == '@' || c == '+') { stop = c; break; }
			const size_t e = line_end(cur);
			if (e == len && !fin) return h;
			size_t n = e - cur;
			if (l_seq + n > 1 && t[e - 1] == '\r' && !(e == len && n == 1)) --n; // (a last line of one byte that no '\n' ends keeps it: nothing is left to read behind the byte that opened the line)
			seq.push_back(Span(cur, n)), l_seq += n;
			cur = e < len ? e + 1 : len;
		}
		bool bad = false;
		if (stop == '+') {
			const size_t pe = line_end(cur);
			if (pe == len) { // the text ends inside the '+' line
				if (!fin) return h;
				bad = true, cur = len;
			} else {
				cur = pe + 1;
				do {
					if (cur >= len) { if (!fin) return h; break; }
					const size_t e = line_end(cur);
					if (e == len && !fin) return h;
					size_t n = e - cur;
					if (n > 0 && l_qual + n > 1 && t[e - 1] == '\r') --n;
					qual.push_back(Span(cur, n)), l_qual += n;
					cur = e < len ? e + 1 : len;
				} while (l_qual < l_seq);
				bad = l_qual != l_seq;
			}
			pos = cur, at_header = false;
		} else {
			pos = cur, at_header = stop != 0;
		}
		mm2amd_fastx_rec_t r;
		r.name = r.comment = r.seq = r.qual = UINT64_MAX, r.name_len = r.comment_len = 0, r.l_seq = 0, r.reserved = 0;
		if (bad) {
			r.l_seq = -2, r.reserved = 1;
		} else {
			r.name = out.put(t + name_b, name_n, false), r.name_len = (uint32_t)name_n;
			if ((flags & MM2AMD_FASTX_WITH_COMMENT) && com_n > 0) r.comment = out.put(t + com_b, com_n, false), r.comment_len = (uint32_t)com_n;
			r.seq = out.pool_len, r.l_seq = (int32_t)l_seq;
			for (const Span &s : seq) out.append(t + s.first, s.second, true);
			out.nul();
			if ((flags & MM2AMD_FASTX_WITH_QUAL) && l_qual > 0) {
				r.qual = out.pool_len;
				for (const Span &s : qual) out.append(t + s.first, s.second, false);
				out.nul();
			}
		}
		if (out.n_recs < out.recs_cap) out.recs[out.n_recs] = r;
		++out.n_recs;
	}
}

} // namespace mm2amd
