// Whole output records on the device: the PAF lines of mm_write_paf4 (format.c:425-458) and the SAM lines of mm_write_sam3 (format.c:522-679)
// for single-segment reads, tag block (write_tags, :397-423), SA:Z: (:638-664), CIGAR, cs and MD included.  One wavefront per record
// (rec_text_dev.hpp); like aln_text_kernel it runs twice around a prefix sum on the host: a sizing pass, then the same walk on a storing sink.
// SEQ and QUAL of a SAM record are copies of host bytes and stay a HOLE in the device's text: the sizing pass reports how many of the record's
// bytes lie in front of it, and the host writes SEQ \t QUAL between the two pieces (format.cpp: format_batch_dev).
#pragma once
#include <cstdint>

namespace mm2amd {

constexpr uint32_t kRecRev = 1u << 10, kRecInv = 1u << 11, kRecSamPri = 1u << 12, kRecHasP = 1u << 13, kRecIsParent = 1u << 14; // RecHit::bits; mapq in bits 0-7,
constexpr uint32_t kRecIsSpliced = 1u << 15;                                                                                      // (mm_reg1_t::is_spliced: junc_text.hpp)
constexpr int kRecSplitShift = 8, kRecTransShift = 16;                                                                            // split in 8-9, trans_strand in 16-17

struct RecHit { // one per hit of the batch; the hits of a read are neighbours (SA:Z: walks them)
	int32_t rid, rs, re, qs, qe, mlen, blen, cnt, score, subsc;
	int32_t dp_max0, dp_score;
	uint32_t n_ambi, n_cigar;
	uint64_t cig_off;       // first operation in the CIGAR pool
	uint64_t q_pos, t_pos;  // cs / MD: the read's [qs, qe) letters in the query pool; the first nibble of the target stretch in S
	float div;
	uint32_t bits;
	uint8_t qsrc, tsrc;     // kTxtQ* / kTxtT* (aln_text.hpp)
	uint8_t pad[6];
};
struct RecJob { // one per record
	uint64_t name_off;      // the read's name in the name pool
	uint32_t name_len;
	int32_t l_seq, rep_len;
	int32_t hit;            // the record's hit, or -1: the no-hit (PAF) / unmapped (SAM) record
	uint32_t hit0, n_hits;  // the read's hits
};
constexpr int32_t kRecOk = 0, kRecFraction = 1, kRecBadCigar = -1; // RecRes::status: 1 = a de / dv value outside [0, 1] (snprintf's business), -1 = operations the walk refuses
struct RecRes { uint32_t len, before; int32_t status; uint32_t reserved; }; // bytes of device text; how many of them precede the hole (SAM; PAF: all)

struct RecParams {
	const RecJob *jobs; int n_jobs;
	const RecHit *hits;
	int64_t flag;           // mm_mapopt_t::flag
	const char *names;      // read names
	const uint8_t *qpool;
	const uint32_t *S;      // packed reference
	const uint32_t *cigar;
	const char *tnames; const uint64_t *tname_off; const uint32_t *tlen; // target names back to back, n_seq + 1 offsets, lengths
	RecRes *res;            // written by the sizing pass, read by the writing pass
	const uint64_t *off;    // writing pass: where each record's device text starts in out
	char *out;
};

void rec_text_launch(const RecParams &P, bool write, void *stream);

} // namespace mm2amd
