// Per-base alignment text on the device: the CIGAR string, the cs tag (short and long form), the ds tag (short and long form) and the MD tag of
// a batch of alignments -- what the reference writes one hit at a time in write_sam_cigar, write_cs_ds_core with write_indel_ds
// (format.c:142-254) and write_MD_core (format.c:302-331).  One wavefront per alignment walks its columns 64 at a time (aln_text_dev.hpp); the
// output is variable-length, so the kernel runs twice: the first pass checks the operations and counts every job's bytes, the host turns the
// lengths into 64-bit offsets, the second pass writes.  Both passes run the same per-column emitter.  ds is cs with brackets around the bases
// by which an insertion or a deletion can be shifted: the two extents of every indel are found when its operation is staged, by scans of the
// aligned query (I) or target (D) that never leave [0, qlen) / [0, tlen) of the job.
#pragma once
#include <cstdint>

namespace mm2amd {

constexpr int kTxtCigar = 0, kTxtCs = 1, kTxtCsLong = 2, kTxtMd = 3, kTxtDs = 4, kTxtDsLong = 5; // MM2AMD_TXT_* (include/mm2amd.h)
constexpr int kTxtTileOps = 256;  // CIGAR operations staged in LDS at a time, with their exclusive query / target / column offsets (ds: and their two shift extents)
constexpr int kTxtDsLaneScan = 6; // ds: an indel up to this long has its shift extents scanned by one lane (at most this many comparisons each way);
                                  // a longer one by the whole wave, 64 comparisons a step
constexpr int kTxtColBytes = 25;  // the most one column emits: ":<10 digits>" of a pending identity run, then "~gt<9 digits>ag" of an intron
                                  // (a ds indel column stays below it: ":<10 digits>" + "+[a]" is 15 bytes)

// where a job's sequences come from
constexpr uint32_t kTxtQCodes = 0,     // nt4 codes, forward: base i at qpool[q_pos + i]
                   kTxtQAscii = 1,     // the read's letters through the nt4 table, forward
                   kTxtQAsciiRev = 2;  // the read's letters, reverse-complemented: base i from qpool[q_pos + qlen - 1 - i] (format.c:353-356)
constexpr uint32_t kTxtTCodes = 0,     // nt4 codes: base i at tpool[t_pos + i]
                   kTxtTPacked = 1,    // the index's 4-bit packed S: base i is the nibble at t_pos + i (FlatIndex::base)
                   kTxtTPackedRev = 2; // ... reverse-complemented: base i from the nibble at t_pos + tlen - 1 - i (mm_idx_getseq_rev, index.c:176-190)

struct TxtJob {
	uint64_t q_pos, t_pos;  // see above
	uint64_t cig_off;       // first operation in the CIGAR pool
	uint32_t n_cigar;
	int32_t qlen, tlen;     // bases the operations must cover (cs / MD)
	uint8_t qsrc, tsrc;
	uint16_t reserved;
};
struct TxtRes { uint64_t cols; uint32_t len; int32_t status; }; // columns walked; bytes of text; 0, or -1 for a job the kernel refuses (then len is 0)

struct TxtParams {
	const TxtJob *jobs; int n_jobs;
	int what;               // kTxtCigar .. kTxtDsLong
	const uint8_t *qpool, *tpool;
	const uint32_t *S;      // packed reference (kTxtTPacked*)
	const uint32_t *cigar;
	TxtRes *res;            // written by the sizing pass, read by the writing pass
	const uint64_t *off;    // writing pass: where each job's text starts in out
	char *out;
};

// write == false: the sizing pass (res[i] for every job); write == true: the text of every job with status 0 at out + off[i]
void aln_text_launch(const TxtParams &P, bool write, void *stream);

} // namespace mm2amd
