// Splice junctions on the device: the lines of mm_write_junc (format.c:263-300), the output of --write-junc (map.c:601-607).  One wavefront per
// PRINTABLE hit -- the host applies map.c's filter (id == parent, mapq >= 10) and mm_write_junc's three tests (is_spliced, p, trans_strand 1 or
// 2), so no wave is launched for a hit that prints nothing -- walks the hit's CIGAR 64 operations a step and writes one line per intron
// (junc_text_dev.hpp).  The tables are rec_text.hpp's: a RecJob per printable hit (the read's name, the hit's index), a RecHit per hit (rid, rs,
// re, the CIGAR, rev and trans_strand in bits, t_pos = the first nibble of sequence rid in S), a RecRes per job; q_pos, the query pool and
// RecRes::before are not used.  As rec_text_kernel it runs twice around a prefix sum on the host: the sizing pass judges the operations (an N
// shorter than 2, an operation code above 9, lengths that do not add up to re - rs: kRecBadCigar) and counts, the writing pass stores.
// RecParams::flag with MM_F_OUT_JUNC set: every line ends with \n (map.c's mm_err_puts); without it the lines of a hit are joined by \n, as
// mm_write_junc leaves them in its kstring (mm2amd_hits_junc_batch).
#pragma once
#include "rec_text.hpp"

namespace mm2amd {

constexpr int64_t kJuncLines = 0x10000000000LL; // MM_F_OUT_JUNC (minimap.h:50)

void junc_text_launch(const RecParams &P, bool write, void *stream);

} // namespace mm2amd
