/* mm2amd.h -- C ABI of libmm2amd.so, the MI355X-native seed-chain-extend engine behind minimap2's API.
 *
 * Everything here is plain C: pointers, sizes, PODs.  Each entry point names the reference interface it
 * replaces (file:line under lh3/minimap2 v2.30).  INTEGRATION.md shows the binding a minimap2 maintainer
 * would add.  All functions return 0 on success and a negative MM2AMD_E* code on failure; the text of the
 * last failure on the calling thread is available from mm2amd_last_error().  There is NO CPU fallback: if
 * no gfx950 device is usable, every compute entry point fails with MM2AMD_ENODEV.
 */
#ifndef MM2AMD_H
#define MM2AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM2AMD_EINVAL  (-1)   /* bad argument */
#define MM2AMD_ENODEV  (-2)   /* no usable HIP device / kernel image */
#define MM2AMD_EHIP    (-3)   /* HIP runtime error */
#define MM2AMD_ENOMEM  (-4)   /* a caller-provided pool was too small */
#define MM2AMD_ESTATE  (-5)   /* called in the wrong state (e.g. map before init) */
#define MM2AMD_EIO     (-6)   /* open/read/write failed; text carries strerror */

const char *mm2amd_last_error(void);
int mm2amd_last_error_code(void);         /* the MM2AMD_E* code that text belongs to (for the entry points that return a pointer) */
int mm2amd_version(void);                 /* ABI version, currently 1 */
int mm2amd_host_cpus(void);                     /* CPUs this process may use: hardware threads capped by the container's CPU quota (cgroup cpu.max); what n_threads <= 0 resolves against */
int mm2amd_device_count(void);            /* number of visible HIP devices, or negative error */

/* ------------------------------------------------------------------------------------------------
 * Kernel-level entry points: batched forms of the reference's per-call kernels.
 * ------------------------------------------------------------------------------------------------ */

/* One extension/global DP problem; same argument meaning as ksw_extd2_sse (ksw2.h:72-73). */
typedef struct {
	const uint8_t *query;    /* qlen codes in 0..m-1 (host memory) */
	const uint8_t *target;   /* tlen codes in 0..m-1 (host memory) */
	int32_t qlen, tlen;
	int32_t w;               /* band width, <0 to disable */
	int32_t zdrop, end_bonus;
	int32_t flag;            /* KSW_EZ_* bits of ksw2.h:8-19 */
} mm2amd_ksw_job_t;

/* Result of one DP problem; field meaning as ksw_extz_t (ksw2.h:34-43).  The CIGAR (BAM encoding,
 * len<<4|op) is at cigar_pool[cigar_off .. cigar_off+n_cigar). */
typedef struct {
	int32_t max, zdropped;
	int32_t max_q, max_t;
	int32_t mqe, mqe_t;
	int32_t mte, mte_q;
	int32_t score;
	int32_t n_cigar;
	int32_t reach_end;
	uint32_t cigar_off;
} mm2amd_ksw_res_t;

/* Batched ksw_extd2_sse (ksw2_extd2_sse.c:34): dual-affine gap cost, results bit-identical to the
 * reference for every job, including jobs whose band binds.  cigar_pool must hold at least
 * sum(qlen+tlen) entries over the batch (MM2AMD_ENOMEM otherwise). */
int mm2amd_ksw_extd2_batch(int n_jobs, const mm2amd_ksw_job_t *jobs, int8_t m, const int8_t *mat,
                           int8_t gapo, int8_t gape, int8_t gapo2, int8_t gape2,
                           mm2amd_ksw_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_cap);

/* Batched mm_update_extra (align.c:254-303, with mm_append_cigar :320-334 and mm_fix_cigar :105-181): a region's window CIGARs are stitched,
 * indels left-aligned, I/D clusters merged, empty operations and a leading gap dropped, and the block / match lengths, ambiguous bases and
 * the best-scoring segment (dp_max) counted -- region_finish_kernel, one wavefront per region.  query / target: nt4 codes (0-3, 4 = N) of
 * the aligned stretches; piece[i] / piece_len[i]: the windows' CIGARs in alignment order.  cigar_pool must hold the sum of all piece lengths
 * (MM2AMD_ENOMEM otherwise).  Results are those of the reference for every input the reference accepts (its asserts hold: the operations
 * cover exactly qlen and tlen); n_cigar < 0 marks a region whose operations do not.  A region of more than MM2AMD_FIN_MAX_OPS operations (the
 * kernel stages a region's CIGAR in LDS) is refused with MM2AMD_EINVAL: the mapper finishes such regions with its host routine. */
#define MM2AMD_FIN_MAX_OPS 7168
typedef struct {
	const uint8_t *query, *target;
	int32_t qlen, tlen;
	int32_t n_pieces;
	const uint32_t *const *piece;
	const int32_t *piece_len;
} mm2amd_fin_job_t;
typedef struct { int32_t n_cigar, blen, mlen, n_ambi, dp_max, qshift, tshift, is_spliced; uint32_t cigar_off; } mm2amd_fin_res_t;
int mm2amd_update_extra_batch(int n_jobs, const mm2amd_fin_job_t *jobs, const int8_t *mat25, int8_t q, int8_t e, int log_gap,
                              mm2amd_fin_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_cap);

/* mm_update_extra with is_eqx = 1: the same jobs, the same result fields, and on top mm_update_cigar_eqx (align.c:183-252) -- every match
 * operation cut into its maximal stretches of equal (=, operation 7) and unequal (X, 8) columns, N against N being equal; a CIGAR none of whose
 * matches splits is relabelled M -> = as it stands, as the reference does in place (cigar_eqx_kernel after region_finish_kernel, one wavefront
 * per region).  n_cigar and the operations are the =/X ones; they can outnumber the sum of the piece lengths, so the pool is sized by a call of
 * its own: cigar_pool == NULL fills every res[i] (n_cigar and cigar_off included) and returns 0; a pool smaller than the sum of the n_cigar
 * returns MM2AMD_ENOMEM with the results filled and nothing written.  MM2AMD_FIN_MAX_OPS bounds the operations coming in, as above. */
int mm2amd_update_extra_eqx_batch(int n_jobs, const mm2amd_fin_job_t *jobs, const int8_t *mat25, int8_t q, int8_t e, int log_gap,
                                  mm2amd_fin_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_cap);

/* Alignment text on the device (aln_text_kernel, one wavefront per alignment): the per-base strings the reference writes hit by hit.
 *   MM2AMD_TXT_CIGAR    "<len><op>" per operation, op letter from "MIDNSHP=XB" (write_sam_cigar, format.c)
 *   MM2AMD_TXT_CS       the short cs string, identity runs as ":n" (write_cs_ds_core with no_iden = 1 and is_ds = 0, format.c:171-254)
 *   MM2AMD_TXT_CS_LONG  the long cs string, identity runs as "=ACGT" (no_iden = 0)
 *   MM2AMD_TXT_MD       the MD string (write_MD_core, format.c:302-331)
 *   MM2AMD_TXT_DS       the short ds string: cs with, for every insertion and deletion, brackets around the bases by which the gap can be
 *                       shifted without changing the alignment, as in "+[a]" or "+[t]aca[gat]" (write_cs_ds_core with is_ds = 1 and
 *                       no_iden = 1, and write_indel_ds, format.c:142-254).  The shifts stop at the ends of the aligned stretches.
 *   MM2AMD_TXT_DS_LONG  the long ds string (no_iden = 0)
 * without the "cs:Z:" / "ds:Z:" / "MD:Z:" tag in front, as mm_gen_cs / mm_gen_ds / mm_gen_MD (format.c:364-395) return them.
 * A job is one alignment: the aligned stretches as nt4 codes (0-3, 4 = N) and its CIGAR.  For cs / ds / MD the operations must be M, I, D, N, = or
 * X, none of length 0, no N shorter than 2, and they must cover exactly qlen and tlen (what the reference's asserts demand): a job that
 * breaks this gets status -1 and no text, and the call still succeeds.  For MM2AMD_TXT_CIGAR only an operation above 9 is refused; the
 * sequences are not read and may be NULL.
 * The text of job i is pool[res[i].off, res[i].off + res[i].len), without a NUL; the jobs' texts follow each other in job order.
 * pool == NULL sizes the batch: res[i].len and res[i].status are filled (the sum of the lengths is the pool the real call needs).
 * A pool that is too small gives MM2AMD_ENOMEM with the lengths filled in; nothing is written at or beyond pool + pool_cap. */
#define MM2AMD_TXT_CIGAR   0
#define MM2AMD_TXT_CS      1
#define MM2AMD_TXT_CS_LONG 2
#define MM2AMD_TXT_MD      3
#define MM2AMD_TXT_DS      4
#define MM2AMD_TXT_DS_LONG 5
typedef struct { const uint8_t *query, *target; int32_t qlen, tlen; const uint32_t *cigar; int32_t n_cigar; } mm2amd_txt_job_t;
typedef struct { uint64_t off; uint32_t len; int32_t status; } mm2amd_txt_res_t;
int mm2amd_aln_text_batch(int n_jobs, const mm2amd_txt_job_t *jobs, int what, mm2amd_txt_res_t *res, char *pool, size_t pool_cap);

/* Batched ksw_ll_qinit + ksw_ll_i16 (ksw2_ll_sse.c:37-152, ksw2.h:93-94): the local (Smith-Waterman) score of a pair with the end coordinates the
 * reference reports -- te the LAST target row whose maximum equals the final maximum, qe the last slot of the 8-lane striped scan that holds it in
 * that row -- as minimap2 uses it for the inversion test (align.c:84-101), mm_seed_ext_score (align.c:591-636) and mm_align1_inv (align.c:916-971).
 * query / target: nt4 codes (0-3, 4 = N) in host memory; mat: the m x m score matrix, m = 5, target code a against query code b scores
 * mat[a * m + b]; gapo, gape: a gap of length l costs gapo + l * gape.  flag says how the kernel reads the sequences, so that a caller needs no
 * staging pass: MM2AMD_LL_QREV the query backwards, MM2AMD_LL_QCOMP the query complemented (code c < 4 becomes 3 - c, anything else 4; both
 * together are the reverse complement of align.c:91-96), MM2AMD_LL_TREV the target backwards (with MM2AMD_LL_QREV: align.c:938-941).  res[i] is
 * what ksw_ll_qinit(km, 2, ...) + ksw_ll_i16 return on the sequences so transformed, coordinates in those sequences; qe may be >= qlen when
 * nothing scores (the scan's last slot is padding).  res[i].path says where job i ran -- the routing is a function of the job alone:
 *   MM2AMD_LL_PATH_HOST  by the host's scalar routine inside the call: a job outside the class in which the plain affine recurrence equals the
 *                        striped scan (it needs -min(mat) <= 2 * (gapo + gape), gapo >= 1, gape > 0, max(mat) * min(qlen, tlen) < 32000 and
 *                        gapo + gape < 16000), a job with qlen or tlen above max_len, and an empty job;
 *   MM2AMD_LL_PATH_WG    ksw_ll_kernel, one workgroup of wg_waves wavefronts per job: qlen > strip_cols and qlen * tlen >= wg_min_cells;
 *   MM2AMD_LL_PATH_WAVE  ksw_ll_kernel, one wavefront per job: every other job.
 * An empty job (qlen == 0 or tlen == 0) gives score 0 and qe = te = -1 (the reference reads outside its arrays there).  Results are in job
 * order.  MM2AMD_EINVAL for m != 5, a null argument, a negative length or a code above 4; n_jobs == 0 returns 0; like every compute entry point
 * the call needs a device (MM2AMD_ENODEV), also when the host would compute every job.  Device buffers are kept between calls.
 * mm2amd_ksw_ll_limits reports strip_cols, wg_waves, wg_min_cells (as in force, see below) and max_len (65535); any pointer may be NULL.
 * Two environment variables are read at every call: MM2AMD_LL_NO_WG=1 sends every device job through the wave class (the A/B of
 * tools/ksw_ll_bench.py); MM2AMD_LL_WG_MIN_CELLS=<n> replaces wg_min_cells (tests send tiny jobs through the workgroup class with it). */
#define MM2AMD_LL_QREV  1
#define MM2AMD_LL_QCOMP 2
#define MM2AMD_LL_TREV  4
#define MM2AMD_LL_PATH_WAVE 0
#define MM2AMD_LL_PATH_WG   1
#define MM2AMD_LL_PATH_HOST 2
typedef struct { const uint8_t *query, *target; int32_t qlen, tlen; int32_t flag; } mm2amd_ll_job_t;
typedef struct { int32_t score, qe, te, path; } mm2amd_ll_res_t;
int mm2amd_ksw_ll_batch(int n_jobs, const mm2amd_ll_job_t *jobs, int8_t m, const int8_t *mat, int gapo, int gape, mm2amd_ll_res_t *res);
int mm2amd_ksw_ll_limits(int *strip_cols, int *wg_waves, int64_t *wg_min_cells, int *max_len);

/* Batched sdust() (sdust.h / sdust.c:134-175): the low-complexity regions of each sequence for score threshold T and window W = 64, the window
 * minimap2 masks its reads with before seeding (mm_dust_minier, map.c:41) -- sdust_kernel, one wavefront per sequence.  seq is ASCII, as sdust()
 * takes it: seq_nt4_table decides, so lower case counts and every other letter, IUPAC codes included, breaks the sequence like an N.
 * The regions of job i are pool[res[i].off, res[i].off + res[i].n), ascending, each start << 32 | finish with the values sdust() returns; the jobs'
 * regions follow each other in job order.  pool == NULL sizes the batch: every res[i].n (and off, path) is filled, the sum of the n is the pool
 * the real call needs.  A pool that is too small gives MM2AMD_ENOMEM with every n filled in; nothing is written at or beyond pool + pool_cap.
 * A job of length 0 has no regions.  res[i].path says which launch class scanned job i -- a function of the job alone:
 *   MM2AMD_SDUST_PATH_NARROW  the list of perfect intervals never held more than narrow_cap entries (it lives in LDS, a dword an entry);
 *   MM2AMD_SDUST_PATH_WIDE    it did: the job stopped there, listed itself on the device, and was scanned again from its first base with
 *                             wide_cap entries, which no list exceeds (an entry lives at most 62 steps and a step adds at most 62).
 * MM2AMD_EINVAL for T <= 0, a null argument, a negative length or a length above max_len; n_jobs == 0 returns 0; MM2AMD_ENODEV without a device.
 * Device buffers are kept between calls.  mm2amd_sdust_limits reports narrow_cap (as in force, see below), wide_cap (4096) and max_len
 * (2^30); any pointer may be NULL.  Two environment variables are read at every call: MM2AMD_SDUST_NARROW_CAP=<n> replaces the narrow
 * capacity (1 .. wide_cap; tests send 100-base reads through the wide class with it); MM2AMD_SDUST_NO_NARROW=1 sends every job through the
 * wide class at once (the A/B of tools/sdust_bench.py).
 * mm2amd_sdust_host_batch is a benchmark and test hook, not part of the drop-in surface: the host's routine (sdust_scan, the default of the
 * `-T` path) on n_threads threads with the same results (path is not set), which tools/sdust_bench.py times against the kernel; it needs no
 * device.  *core_seconds, unless NULL, receives the threads' summed time inside the scans. */
#define MM2AMD_SDUST_PATH_NARROW 0
#define MM2AMD_SDUST_PATH_WIDE   1
typedef struct { const char *seq; int32_t len; } mm2amd_sdust_job_t;
typedef struct { uint64_t off; uint32_t n; int32_t path; } mm2amd_sdust_res_t;
int mm2amd_sdust_batch(int n_jobs, const mm2amd_sdust_job_t *jobs, int T, mm2amd_sdust_res_t *res, uint64_t *pool, size_t pool_cap);
int mm2amd_sdust_limits(int *narrow_cap, int *wide_cap, int *max_len);
int mm2amd_sdust_host_batch(int n_jobs, const mm2amd_sdust_job_t *jobs, int T, int n_threads, mm2amd_sdust_res_t *res, uint64_t *pool, size_t pool_cap,
                            double *core_seconds);

/* The hit-list rules of a split-index merge (merge_hits, map.c:520-531) for a batch of read segments -- hits_merge_kernel, one wavefront per
 * segment.  Segment s owns hits[seg_off[s], seg_off[s + 1]): the records of all index parts concatenated in part order, rid already shifted,
 * dp_max as mm_update_dp_max left it.  Per segment, in the reference's order: subsc, n_sub and dp_max2 start at 0; mm_hit_sort with opt->alt_drop
 * (dead hits -- cnt == 0 and not an inversion -- go, a list of one hit is left alone, equal keys come in the order of the reference's unstable
 * radix sort); mm_set_parent; unless MM2AMD_HM_ALL_CHAINS, mm_select_sub and mm_set_sam_pri.  mm_update_dp_max before and mm_set_mapq2 / mm_pair
 * after stay with the caller (libm and CIGAR walks in double).
 * out[k] answers hits[k]: pos is the hit's place in its segment's final list, -1 if it was dropped (every other field is then 0); id, parent,
 * subsc, n_sub and dp_max2 are the record's fields there (dp_max2 is 0 for a hit without alignment); flags holds MM2AMD_HM_SAM_PRI and
 * MM2AMD_HM_STRAND_RETAINED (with MM2AMD_HM_ALL_CHAINS the two are the input's).  seg[s].n_kept is the length of the final list and seg[s].path
 * the class that ran the segment:
 *   MM2AMD_HM_PATH_NARROW  up to narrow_cap (64) hits, the records in 8.5 KB of LDS
 *   MM2AMD_HM_PATH_WIDE    up to wide_cap (448) hits, 58 KB of LDS
 *   MM2AMD_HM_PATH_HOST    more hits than that, or more than 64 live hits two of which have equal sort keys (the order among them is then a
 *                          property of the radix sort's cycle walk, which the host replays): the same rules on the host's pool threads
 * MM2AMD_EINVAL for a null argument, descending offsets or a segment above max_hits; n_seg == 0 returns 0; MM2AMD_ENODEV without a device.
 * mm2amd_hits_merge_host_batch is the host twin (test and benchmark hook; no device): the same rules on n_threads threads, path is
 * MM2AMD_HM_PATH_HOST throughout; with MM2AMD_HM_WAVE_PARENTS it runs the kernel's lane-wise form of mm_set_parent, lane after lane.
 * *core_seconds, unless NULL, receives the threads' summed time. */
#define MM2AMD_HM_PATH_NARROW 0
#define MM2AMD_HM_PATH_WIDE   1
#define MM2AMD_HM_PATH_HOST   2
#define MM2AMD_HM_REV 1u              /* mm2amd_hm_hit_t::flags */
#define MM2AMD_HM_INV 2u
#define MM2AMD_HM_ALT 4u
#define MM2AMD_HM_ALIGNED 8u          /* the hit has an mm_extra_t: dp_max is read, dp_max2 is kept */
#define MM2AMD_HM_SAM_PRI 16u         /* also in mm2amd_hm_out_t::flags */
#define MM2AMD_HM_STRAND_RETAINED 32u /* also in mm2amd_hm_out_t::flags */
#define MM2AMD_HM_HARD_MLEVEL 1u      /* mm2amd_hm_opt_t::flags: MM_F_HARD_MLEVEL */
#define MM2AMD_HM_ALL_CHAINS 2u       /* MM_F_ALL_CHAINS */
#define MM2AMD_HM_CHECK_STRAND 4u     /* mm_select_sub's check_strand (0 in merge_hits) */
#define MM2AMD_HM_WAVE_PARENTS 8u     /* host twin only */
typedef struct { int32_t cnt, rid, score, qs, qe, rs, re, dp_max; uint32_t hash, flags; } mm2amd_hm_hit_t;
typedef struct { int32_t pos, id, parent, subsc, n_sub, dp_max2; uint32_t flags; int32_t reserved; } mm2amd_hm_out_t;
typedef struct { int32_t n_kept, path; } mm2amd_hm_seg_t;
typedef struct {
	float mask_level; int32_t mask_len;       /* mm_set_parent */
	float pri_ratio; int32_t best_n;          /* mm_select_sub */
	float alt_drop;
	int32_t sub_diff;                         /* 2 a + b */
	int32_t min_diff;                         /* 2 k */
	int32_t min_strand_sc;                    /* 0.8 max_gap */
	uint32_t flags;
} mm2amd_hm_opt_t;
int mm2amd_hits_merge_batch(int n_seg, const uint64_t *seg_off, const mm2amd_hm_hit_t *hits, const mm2amd_hm_opt_t *opt, mm2amd_hm_out_t *out,
                            mm2amd_hm_seg_t *seg);
int mm2amd_hits_merge_host_batch(int n_seg, const uint64_t *seg_off, const mm2amd_hm_hit_t *hits, const mm2amd_hm_opt_t *opt, int n_threads,
                                 mm2amd_hm_out_t *out, mm2amd_hm_seg_t *seg, double *core_seconds);
int mm2amd_hits_merge_limits(int *narrow_cap, int *wide_cap, int *max_hits);

/* Pairing the two mates of a batch of fragments: mm_pair (pe.c:81-182) followed by mm_set_pe_thru (pe.c:50-68) -- pair_kernel, one wavefront
 * per fragment.  Fragment f owns hits[hit0, hit0 + n[0] + n[1]): segment 0's hits, then segment 1's, as they stand after mm_set_mapq2 (id,
 * parent, mapq, sam_pri; dp_max is mm_extra_t::dp_max: every hit is aligned).  The fragments' ranges must not overlap; out entries between
 * them are unspecified after a call.  max_gap_ref is per fragment (the mapper's frag_gap).
 * out[k] answers hits[k]: parent and mapq are the record's fields after the call, flags holds MM2AMD_PE_SAM_PRI (as it stands after the call),
 * MM2AMD_PE_PROPER_FRAG (pe.c:143: the two hits of the pair) and MM2AMD_PE_THRU (pe.c:65).  A fragment with an unmapped mate (n[s] == 0) is
 * answered unchanged (pe.c:102-105 returns before mm_set_pe_thru) by the entry point itself, as MM2AMD_PE_PATH_NARROW.
 * res[f].n_pairs is the number of candidate pairs over the dp_max bar (sc.n, pe.c:130), best[s] the position of the pair's hit in segment s
 * (-1: no pair, pe.c:139), status MM2AMD_PE_OK or MM2AMD_PE_BAD_PARENT -- a parent that does not index its own segment, where pe.c:146 would read
 * out of bounds: the fragment is answered unchanged --, and path the class that ran the fragment:
 *   MM2AMD_PE_PATH_NARROW  up to narrow_cap (64) ends, one per lane
 *   MM2AMD_PE_PATH_WIDE    up to wide_cap (1024) ends, 36 KB of LDS
 *   MM2AMD_PE_PATH_HOST    more ends than that, or more than 64 ends two of which have equal keys (pe.c:95; radix_sort_pair's order among them is
 *                          then the cycle walk's, which the host replays): the same rules on the host's pool threads, inside the same call
 * MM2AMD_EINVAL for a negative count, a null array with work to do, match_sc <= 0, a segment above max_hits, overlapping ranges or ranges that
 * span more than 2^31 hits; n_frag == 0 returns 0; MM2AMD_ENODEV without a device.  mm2amd_pair_host_batch is the host twin (test and benchmark
 * hook; no device): the same rules on n_threads threads, path is MM2AMD_PE_PATH_HOST throughout (an unmapped mate included); *core_seconds,
 * unless NULL, receives the threads' summed time. */
#define MM2AMD_PE_PATH_NARROW 0
#define MM2AMD_PE_PATH_WIDE   1
#define MM2AMD_PE_PATH_HOST   2
#define MM2AMD_PE_OK 0                /* mm2amd_pe_res_t::status */
#define MM2AMD_PE_BAD_PARENT 1
#define MM2AMD_PE_REV 1u              /* mm2amd_pe_hit_t::flags */
#define MM2AMD_PE_SAM_PRI 2u          /* also in mm2amd_pe_out_t::flags */
#define MM2AMD_PE_PROPER_FRAG 4u      /* mm2amd_pe_out_t::flags */
#define MM2AMD_PE_THRU 8u
typedef struct { int32_t rid, rs, re, qs, qe, dp_max, id, parent, mapq; uint32_t hash, flags, reserved; } mm2amd_pe_hit_t;
typedef struct { int32_t parent, mapq; uint32_t flags; int32_t reserved; } mm2amd_pe_out_t;
typedef struct { uint64_t hit0; int32_t n[2], qlen[2], max_gap_ref, reserved; } mm2amd_pe_frag_t;
typedef struct { int32_t path, status, n_pairs, best[2], reserved; } mm2amd_pe_res_t;
typedef struct { int32_t pe_bonus, sub_diff /* 2 a + b */, match_sc /* a */, reserved; } mm2amd_pe_opt_t;
int mm2amd_pair_batch(int n_frag, const mm2amd_pe_frag_t *frag, const mm2amd_pe_hit_t *hits, const mm2amd_pe_opt_t *opt, mm2amd_pe_out_t *out,
                      mm2amd_pe_res_t *res);
int mm2amd_pair_host_batch(int n_frag, const mm2amd_pe_frag_t *frag, const mm2amd_pe_hit_t *hits, const mm2amd_pe_opt_t *opt, int n_threads,
                           mm2amd_pe_out_t *out, mm2amd_pe_res_t *res, double *core_seconds);
int mm2amd_pair_limits(int *narrow_cap, int *wide_cap, int *max_hits);

/* FASTA / FASTQ text into sequence records: kseq_read (kseq.h:192-232, with ks_getuntil2's CR rule, kseq.h:101-149) + kseq2bseq (bseq.c:65-78:
 * U -> T, u -> t; qual and comment only on request and when not empty) over a buffer in memory -- fastx_lines_kernel, fastx_classify_kernel and
 * fastx_copy_kernel for the two regular shapes, the host's parser (fastx.hpp) for everything else.  The batching of mm_bseq_read3 (bseq.c:80-119)
 * and mm_bseq_read_frag2 (bseq.c:131-159) is the caller's (minimap2_amd.FastxReader), as is decompression.
 * text[0, len) is a block of the file; is_final says that the file ends with it.  The call returns the records that are COMPLETE and *consumed, the
 * offset of the first byte that belongs to none of them: the caller puts text[consumed, len) in front of the next block.  In a non-final block a
 * FASTA-type record is complete once the first byte of the next header has been seen, a FASTQ-type record once its quality has reached the
 * sequence's length on a line that '\n' ends; a final block's end completes what the reference returns at EOF.  A non-final block without a
 * complete record returns 0 with *n_recs = 0 and *consumed = 0: supply a longer one.
 * Record i is recs[i]: offsets into pool of its NUL-terminated strings, UINT64_MAX for a string that is absent (NULL in mm_bseq1_t): qual unless
 * MM2AMD_FASTX_WITH_QUAL is set and the quality is not empty, comment unless MM2AMD_FASTX_WITH_COMMENT is set and the comment is not empty.
 * An entry with reserved == 1 (l_seq == -2, no strings) stands for a malformed record -- kseq_read's -2: a quality of another length than the
 * sequence, or a '+' line the file ends in -- after which mm_bseq_read3 ends its batch; only the host class reports such entries.
 * *path is a function of the buffer alone:
 *   MM2AMD_FASTX_PATH_FASTQ4  the first byte is '@' and every record is four lines: '@' header, a sequence line of at least one payload byte
 *                             that begins with none of '>', '+', '@', CR, a '+' line, a quality line of the same payload length; LF or CRLF; the
 *                             last '\n' may be missing in a final block; the lines of a trailing incomplete record of a non-final block are left;
 *   MM2AMD_FASTX_PATH_FASTA   the first byte is '>' and no line begins with '+' or '@'; any number of sequence lines, empty lines anywhere,
 *                             LF or CRLF.  A line that is a lone CR, or a final block that ends in a lone '>', sends the buffer to the host;
 *   MM2AMD_FASTX_PATH_HOST    everything else: the host's parser on the same buffer (one scan on the device is then lost).
 * recs == NULL or pool == NULL sizes the call: *n_recs, *pool_len, *consumed and *path are filled.  A capacity that is too small gives
 * MM2AMD_ENOMEM with the sizes filled; nothing is written at or beyond either capacity.  len == 0 returns 0 with no records.  MM2AMD_EINVAL for a
 * null text with len > 0, a null out-pointer or len > max_text (2^30); MM2AMD_ENODEV without a device.  Device and pinned buffers are kept
 * between calls; the call has a stream and a profiler slot of its own and runs one at a time.  MM2AMD_FASTX_LONG_LINE=<n> (read at every call,
 * at least 16) replaces the payload length from which fastx_copy_kernel's long class copies a line (4096; tests send 100-byte lines through it).
 * mm2amd_fastx_parse_host is the host's parser alone with the same results (path = HOST): it needs no device and has no length limit.
 * mm2amd_fastx_limits reports max_text and long_line as in force; either pointer may be NULL.  mm2amd_fastx_last_times is a benchmark hook: the
 * last mm2amd_fastx_parse's seconds in upload, device work up to the sizes, copy kernels, download, the host's table, the host's parser. */
#define MM2AMD_FASTX_WITH_QUAL    1
#define MM2AMD_FASTX_WITH_COMMENT 2
#define MM2AMD_FASTX_PATH_HOST   0
#define MM2AMD_FASTX_PATH_FASTQ4 1
#define MM2AMD_FASTX_PATH_FASTA  2
typedef struct { uint64_t name, comment, seq, qual;   /* offsets into pool; UINT64_MAX = absent (NULL in mm_bseq1_t) */
                 uint32_t name_len, comment_len; int32_t l_seq, reserved; } mm2amd_fastx_rec_t;
int mm2amd_fastx_parse(const char *text, size_t len, int is_final, int flags, mm2amd_fastx_rec_t *recs, size_t recs_cap, char *pool, size_t pool_cap,
                       size_t *n_recs, size_t *pool_len, size_t *consumed, int *path);
int mm2amd_fastx_parse_host(const char *text, size_t len, int is_final, int flags, mm2amd_fastx_rec_t *recs, size_t recs_cap, char *pool, size_t pool_cap,
                            size_t *n_recs, size_t *pool_len, size_t *consumed, int *path);
int mm2amd_fastx_limits(size_t *max_text, int *long_line);
int mm2amd_fastx_last_times(double *out, int cap);

/* The two device-wide primitives of the index build (device_sort.hip), exposed for testing.  mm2amd_sort_pairs_u64: n (key, value) pairs
 * sorted in place by key bits [0, bits), stably -- what radix_sort_128x (ksort.h:101-151, instantiated at sketch.c:13 and called per bucket
 * at index.c:236) yields for pairs whose input order is ascending in the value: rs_hist / rs_chunk_scan / rs_block_offsets / rs_scatter
 * kernels, one LSD pass per 8 bits.  mm2amd_exclusive_sum_u32: out[i] = in[0] + ... + in[i-1] mod 2^32 for i in [0, n], i.e. out holds
 * n + 1 entries (the running offsets of index.c:249-268).  n < 2^32 for both. */
int mm2amd_sort_pairs_u64(uint64_t *keys, uint64_t *vals, uint64_t n, int bits);
int mm2amd_exclusive_sum_u32(const uint32_t *in, uint32_t *out, uint64_t n);

/* encode_kernel (ASCII -> nt4, forward and reverse complement: align.c:1056-1061) on a batch of its own, exposed for testing: the n
 * fragments are packed into one pinned buffer the way a mapping batch is, and the kernel runs with the launch shape the mapper uses.
 * seqs[i] holds lens[i] bases, followed by lens2[i] bases of a mate when lens2 is not NULL and lens2[i] > 0 (the two are then units of their
 * own, as in a batch of read pairs); lengths may be 0.  With T the sum of all lengths, out receives 2 * T + 32 bytes: 16 bytes 0xff, the query
 * pool -- for the unit at base offset o with len bases, forward codes at 2 * o + j and the reverse complement at 2 * o + 2 * len - 1 - j --,
 * 16 bytes 0xff: the pool is set to 0xff before the launch, so a byte the kernel did not write shows.  MM2AMD_ENCODE_BLOCKS=<n> (read once
 * per process) replaces the grid size, for A/B runs.  mm2amd_encode_range launches the kernel on fragments [lo, hi) of that batch only, the
 * way a mapper lane launches it on its sub-batch (offsets into the whole batch's buffers, a first word that starts anywhere): the blocks of
 * the other fragments stay 0xff. */
int mm2amd_encode_batch(int n, const char *const *seqs, const int32_t *lens, const int32_t *lens2, uint8_t *out);
int mm2amd_encode_range(int n, const char *const *seqs, const int32_t *lens, const int32_t *lens2, int lo, int hi, uint8_t *out);

/* Batched ksw_extz2_sse (ksw2_extz2_sse.c:25, ksw2.h:70-71): single-affine gap cost; same contract as above. */
int mm2amd_ksw_extz2_batch(int n_jobs, const mm2amd_ksw_job_t *jobs, int8_t m, const int8_t *mat, int8_t gapo, int8_t gape,
                           mm2amd_ksw_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_cap);

/* Batched ksw_exts2_sse (ksw2_exts2_sse.c:33, ksw2.h:77-79): splice-aware alignment (intron state on the target, N operations;
 * flag carries KSW_EZ_SPLICE_FOR/REV/FLANK/CMPLX as in the reference; the job's w is ignored: this DP has no band).  Junction
 * annotation (the reference's junc/junc_bonus/junc_pen arguments) is not taken at this boundary: the call equals the
 * reference's with junc == NULL.  Same contract as above otherwise. */
int mm2amd_ksw_exts2_batch(int n_jobs, const mm2amd_ksw_job_t *jobs, int8_t m, const int8_t *mat, int8_t gapo, int8_t gape, int8_t gapo2, int8_t noncan,
                           mm2amd_ksw_res_t *res, uint32_t *cigar_pool, size_t cigar_pool_cap);

/* ------------------------------------------------------------------------------------------------
 * Drop-in boundary: the batched replacement of kt_for(n_threads, worker_for, step, n_frag) (map.c:576).
 *
 * The pointer arguments are the reference's own objects (their layouts are mirrored in
 * minimap2_amd/csrc/abi_ref.hpp): mi = const mm_idx_t* (minimap.h:88-100), opt = const mm_mapopt_t*
 * (minimap.h:136-192), seq = const mm_bseq1_t* (bseq.h:14-17), reg = mm_reg1_t** (minimap.h:112-127).
 * When this header is included after minimap.h the real types are used in the prototypes.
 * ------------------------------------------------------------------------------------------------ */
#ifdef MINIMAP2_H
typedef mm_idx_t mm2amd_idx_t; typedef mm_mapopt_t mm2amd_mapopt_t; typedef mm_reg1_t mm2amd_reg1_t;
struct mm2amd_bseq1_s; /* mm_bseq1_t lives in bseq.h; pass it as-is */
#define MM2AMD_BSEQ_PTR const void *
#define MM2AMD_REG_PP   void **
#else
typedef void mm2amd_idx_t; typedef void mm2amd_mapopt_t;
#define MM2AMD_BSEQ_PTR const void *
#define MM2AMD_REG_PP   void **
#endif

/* ------------------------------------------------------------------------------------------------
 * Options (options.c).  io = mm_idxopt_t* (minimap.h:130-134), mo = mm_mapopt_t* (minimap.h:136-192).
 * ------------------------------------------------------------------------------------------------ */
void mm2amd_idxopt_init(void *io);                                /* mm_idxopt_init, options.c:5 */
void mm2amd_mapopt_init(void *mo);                                /* mm_mapopt_init, options.c:14 */
int mm2amd_set_opt(const char *preset, void *io, void *mo);       /* mm_set_opt, options.c:91; -1 for an unknown preset */
int mm2amd_check_opt(const void *io, const void *mo);             /* mm_check_opt, options.c:202 (per-read-path subset) */

/* ------------------------------------------------------------------------------------------------
 * Index built on the device from in-memory sequences: the counterpart of mm_idx_str (index.c:421,
 * minimap.h:324).  seq[i] are NUL-terminated; name may be NULL.  Returns NULL on failure.  A lookup in
 * this index yields the same (count, ascending position list) as mm_idx_get on the reference's index.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mm2amd_index_s mm2amd_index_t;
mm2amd_index_t *mm2amd_idx_str(int w, int k, int is_hpc, int bucket_bits, int n, const char **seq, const char **name);
void mm2amd_idx_destroy(mm2amd_index_t *idx);                     /* mm_idx_destroy, index.c:50 */
int mm2amd_idx_stat(const mm2amd_index_t *idx, int *k, int *w, int *flag, uint32_t *n_seq, uint64_t *sum_len,
                    uint64_t *n_distinct, uint64_t *n_minimizers); /* the figures mm_idx_stat prints, index.c:112-134 */
int32_t mm2amd_idx_cal_max_occ(const mm2amd_index_t *idx, float f); /* mm_idx_cal_max_occ, index.c:198 */
int mm2amd_mapopt_update(void *mo, const mm2amd_index_t *idx);    /* mm_mapopt_update, options.c:69 */
int mm2amd_idx_table_shape(const mm2amd_index_t *idx, int *bucket_bits, int *key_shift);
int mm2amd_idx_export(const mm2amd_index_t *idx, uint32_t *bucket_start, uint64_t *keys, uint32_t *val_off, uint64_t *pos, uint32_t *S);

/* ------------------------------------------------------------------------------------------------
 * Index files: the device-built index written and read in the reference's .mmi format (MMI\2).
 * A file written here loads with the unmodified reference (mm_idx_load, the minimap2 binary) and every section equals what
 * mm_idx_dump writes for the index mm_idx_gen / mm_idx_str builds from the same sequences with the same w, k, b, flag -- magic and
 * header, name/length table, per bucket n, the p array, size, and S -- with ONE exception: a bucket's (key, value) pairs are written
 * in ascending key order, where the reference writes them in khash slot order (an artefact of its probing; mm_idx_load re-inserts
 * them, so the loaded index is the same).
 * ------------------------------------------------------------------------------------------------ */
#define MM2AMD_DUMP_NO_SEQ 1                  /* write an MM_I_NO_SEQ index (no S section) */
/* mm_idx_dump (index.c:475-514): one index part in the reference's MMI\2 format. bucket_bits <= 0: 14.  MM2AMD_EINVAL for what the
 * format cannot hold (a name of more than 255 bytes, a bucket of 2^31 positions or more, bucket_bits outside [1, 2k] or above 28, an
 * index without sequence unless MM2AMD_DUMP_NO_SEQ is given); MM2AMD_EIO when a write fails -- the partial file is removed. */
int mm2amd_idx_dump(const mm2amd_index_t *idx, const char *fn, int bucket_bits, int flags);
/* mm_idx_load (index.c:516-569) for part `part` (0-based) of a possibly multi-part file, as mm_idx_reader_read (index.c:621)
 * walks them. *more (may be NULL) = 1 when another part follows the one loaded. NULL on failure (mm2amd_last_error_code():
 * MM2AMD_EINVAL for a truncated or corrupt file or a part beyond the last, MM2AMD_EIO when the file cannot be opened or read).
 * The tables come from the file's bucket records (they are not rebuilt from S); a file with MM_I_NO_SEQ gives an index that serves
 * chain-level mapping only. */
mm2amd_index_t *mm2amd_idx_load(const char *fn, int part, int *more);
int mm2amd_idx_is_idx(const char *fn);        /* mm_idx_is_idx (index.c:571): 1 an index file, 0 not, <0 error */
int mm2amd_idx_seq(const mm2amd_index_t *idx, uint32_t i, const char **name, uint32_t *len);  /* mi->seq[i]; name NULL with MM_I_NO_NAME */
/* mm_idx_getseq (index.c:164-174): bases [st, en) of sequence rid as nt4 codes (0-3, 4 = N) into out; returns en - st.  MM2AMD_EINVAL for
 * st > en, en beyond the sequence, a rid the index does not have, or an index without sequence (MM_I_NO_SEQ). */
int mm2amd_idx_getseq(const mm2amd_index_t *idx, uint32_t rid, uint32_t st, uint32_t en, uint8_t *out);
/* mm_gen_cs_ds_or_MD (format.c:333-375) for a batch of hits: the text `what` (MM2AMD_TXT_*, above) of hit[i] -- an mm_reg1_t* as
 * mm_gpu_map_batch returns them -- whose read is qseq[i] (letters, qlen[i] of them).  The target comes from the handle's packed sequence on
 * the device; the read's [qs, qe) letters are uploaded.  Orientation as format.c:343-358: is_qstrand = 0 writes on the target's strand (the
 * read reverse-complemented for a hit on the reverse strand), is_qstrand = 1 on the read's (mm_idx_getseq2's window of the reverse strand).
 * A hit without base-level alignment (p == NULL) gets len 0, status 0; res and pool as for mm2amd_aln_text_batch.  MM2AMD_EINVAL for an
 * index without sequence, rid / rs / re outside the sequence, or qs / qe outside the read. */
int mm2amd_hits_text_batch(const mm2amd_index_t *idx, int n_hits, const void *const *hit, const char *const *qseq, const int32_t *qlen,
                           int what, int is_qstrand, mm2amd_txt_res_t *res, char *pool, size_t pool_cap);
/* mm_write_junc (format.c:263-300) for a batch of hits: the splice junctions of hit[i] -- an mm_reg1_t* -- of the read named qname[i], one line
 * tname \t start \t end \t qname \t score \t +|-  per intron (N operation), as the reference leaves them in its kstring: joined by '\n', none at
 * the end.  A hit that writes nothing (not is_spliced, p == NULL, trans_strand neither 1 nor 2, no intron) gets len 0, status 0.  There is no
 * mapq / parent filter here: that is map.c's (:604).  junc_text_kernel, one wavefront per hit that can write; the target comes from the handle's
 * packed sequence on the device.  res and pool as for mm2amd_aln_text_batch (pool == NULL sizes the batch; a pool too small: MM2AMD_ENOMEM, the
 * lengths filled, nothing written).  A hit whose CIGAR breaks the reference's asserts (an intron shorter than 2, a walk that does not end at re)
 * or holds an operation code above 9 gets status -1 and no text, and the call succeeds.  MM2AMD_EINVAL for an index without names
 * (MM_I_NO_NAME) or without sequence, or for rid / rs / re outside the sequence. */
int mm2amd_hits_junc_batch(const mm2amd_index_t *idx, int n_hits, const void *const *hit, const char *const *qname, mm2amd_txt_res_t *res,
                           char *pool, size_t pool_cap);
/* Diagnostics: the phases of this process' last mm2amd_idx_dump / mm2amd_idx_load -- total, regroup (dump: sort by bucket + offsets), serialise / unpack
 * kernels, device<->host copies (HIP events), file write / read (host clock), sort and tables (load), of which S, then image bytes, file bytes, chunks,
 * chunk bytes.  Milliseconds and bytes; returns the number of values there are. */
int mm2amd_idx_io_stats(double *v, int n);

/* Call once per index part after mm_mapopt_update() (main.c:465): builds the device mirror of the index
 * (flat minimizer table + 4-bit packed reference) and captures the mapping options.  n_threads sizes the host
 * worker pool (<=0: all hardware threads).  Replaces nothing in the reference; it is the set-up the GPU path needs. */
int mm_gpu_init(const mm2amd_idx_t *mi, const mm2amd_mapopt_t *opt, int n_threads);

/* Same contract as calling worker_for(step, i, tid) for i in [0, n_frag) (map.c:425-474): for fragment i with
 * segments seq[seg_off[i] .. seg_off[i]+n_seg[i]) fills n_reg[], reg[] (libc-allocated, caller frees reg[k] and each
 * reg[k][j].p), rep_len[] and frag_gap[] at the segment's index.  Output order == input order.
 * n_seg[i] is 1 or 2.  For a read pair the library does what worker_for does around mm_map_frag (map.c:436-473): the mates are
 * mapped in the orientation mm_mapopt_t::pe_ori prescribes (on copies; seq is not modified), jointly, or each on its own with
 * MM_F_INDEPEND_SEG / MM_F_WEAK_PAIRING, paired by mm_pair's rules, and their hits are turned back to the given orientation.
 * mm_gpu_init refuses (MM2AMD_EINVAL) the configurations the library does not handle; see INTEGRATION.md section 2. */
int mm_gpu_map_batch(int n_frag, const int *seg_off, const int *n_seg, MM2AMD_BSEQ_PTR seq,
                     int *n_reg, MM2AMD_REG_PP reg, int *rep_len, int *frag_gap);

/* As mm_gpu_init, for an index built by mm2amd_idx_str (which must outlive the mapper). */
int mm_gpu_init_index(const mm2amd_index_t *idx, const mm2amd_mapopt_t *opt, int n_threads);

/* Several GPUs behind the same hook (the reference has ONE kt_for call per mini-batch, map.c:576, so the
 * dispatcher lives below it): n_gpus replicas, each with a full copy of the index in its device's HBM, map contiguous shares of
 * every batch cut by cumulative bases -- independent shares, no exchange between devices, results straight into the caller's
 * host arrays.  device_ids: HIP ordinals (NULL: 0 .. n_gpus-1); an ordinal may repeat (several replicas on one device: tests on
 * a single-GPU machine).  n_gpus <= 0: $MM2AMD_GPUS, else 1 -- which is what mm_gpu_init / mm_gpu_init_index pass.  n_threads
 * is the host pool of the whole context (<= 0: 64 per GPU, capped by the hardware threads), divided among the replicas. */
int mm_gpu_init_multi(const mm2amd_idx_t *mi, const mm2amd_mapopt_t *opt, int n_threads, int n_gpus, const int *device_ids);
int mm_gpu_init_index_multi(const mm2amd_index_t *idx, const mm2amd_mapopt_t *opt, int n_threads, int n_gpus, const int *device_ids);
int mm_gpu_n_replicas(void);                     /* replicas of the live context (0: none) */

/* SURVEY.md 8(b)(2) as written -- the batch call that names its index and options: the device context for (mi, *opt) is built on first use
 * and rebuilt when either changes (as mm_gpu_map does), then this is mm_gpu_map_batch.  Calls of mm_gpu_map_batch_with, mm_gpu_map and mm_gpu_map_frag
 * are SERIALISED among themselves from the (mi, opt) check to the end of the mapping: there is one context per process, and a thread naming another
 * index or other options rebuilds it only after the batch under way has come back (a rebuild costs seconds -- callers should stick to one pair). */
int mm_gpu_map_batch_with(const mm2amd_idx_t *mi, const mm2amd_mapopt_t *opt, int n_frag, const int *seg_off, const int *n_seg, MM2AMD_BSEQ_PTR seq,
                          int *n_reg, MM2AMD_REG_PP reg, int *rep_len, int *frag_gap);

/* Batch-of-one calls with the reference's signatures: mm_gpu_map for mm_map (map.c:380-392, minimap.h:375-376), mm_gpu_map_frag for
 * mm_map_frag (map.c:227-378, minimap.h:378-379; n_segs 1 or 2).  Results as the reference returns them (libc blocks; NULL / 0 when
 * nothing maps or on failure -- mm2amd_last_error() tells which); b, when not NULL, receives rep_len and frag_gap (mm_tbuf_t,
 * minimap.h:207-210).  The device context is built on first use and rebuilt when (mi, *opt) change.  One GPU pipeline pass per
 * call: the convenience path of a binding that maps read by read (python/cmappy.h:74-102), not the fast path. */
void *mm_gpu_map(const mm2amd_idx_t *mi, int qlen, const char *seq, int *n_regs, void *b, const mm2amd_mapopt_t *opt, const char *qname);
void mm_gpu_map_frag(const mm2amd_idx_t *mi, int n_segs, const int *qlens, const char **seqs, int *n_regs, MM2AMD_REG_PP regs, void *b,
                     const mm2amd_mapopt_t *opt, const char *qname);

/* mm_gpu_map_batch in two halves: mm_gpu_batch_stage copies the batch's sequences to the device (the hand-over the
 * reference's pipeline step 0 makes, map.c:543-575) and returns when they are resident; mm_gpu_map_staged runs the
 * hot path on the staged batch (results placed as mm_gpu_map_batch places them: read seg_off[i] + j of fragment i).  seq, and the
 * seg_off / n_seg the batch was staged with, describe the result arrays; seq must stay valid in between. */
int mm_gpu_batch_stage(int n_frag, const int *seg_off, const int *n_seg, MM2AMD_BSEQ_PTR seq);
int mm_gpu_map_staged(int *n_reg, MM2AMD_REG_PP reg, int *rep_len, int *frag_gap);
/* The pipeline form of the hand-over (kt_pipeline, map.c:541-577: step 0 of batch k+1 runs beside step 1 of batch k): the library keeps two
 * resident batches, so this call may run on another thread WHILE mm_gpu_map_staged maps the previous batch -- pinned-memory packing and H2D
 * then cost no mapping time.  It waits (instead of replacing, as mm_gpu_batch_stage does) while an earlier staged batch has not been taken
 * over by a mapping call yet: every staged batch is mapped exactly once, in staging order.  seq must stay valid until its batch is mapped. */
int mm_gpu_batch_stage_queued(int n_frag, const int *seg_off, const int *n_seg, MM2AMD_BSEQ_PTR seq);
void mm_gpu_batch_discard(void);                 /* drop a staged batch that will not be mapped (a pipeline shutting down) */

/* Host output stage: replaces the record-writing loop of the reference's pipeline step 2
 * (map.c:585-623: mm_write_sam3, format.c:522, or mm_write_paf4, format.c:425, per hit, then mm_err_puts) for one mini-batch.
 * The text is byte-identical to what that loop prints -- SAM or PAF by MM_F_OUT_SAM, cg/cs/ds/MD/ts/SA tags, unmapped records
 * by MM_F_PAF_NO_HIT / MM_F_SAM_HIT_ONLY, secondaries by MM_F_NO_PRINT_2ND -- but produced on the host thread pool.
 * Arguments as for mm_gpu_map_batch (results as it returned them); *out receives ONE malloc'd block of '\n'-terminated
 * records in input order (free() it), *out_len its length.  Fragments of one or two segments (mate fields of mm_write_sam3,
 * /1 /2 names of mm_write_paf4); no RG tag; uses the index and
 * options given to mm_gpu_init.
 * With MM_F_OUT_JUNC (--write-junc) the text is that of map.c:601-607 instead: for every hit with id == parent and mapq >= 10, mm_write_junc's
 * lines (format.c:263-300: tname \t start \t end \t qname \t score \t +|- per intron), each with its '\n'; nothing for other hits or for reads
 * without hits; the SAM / PAF flags play no part.  MM2AMD_EINVAL, and no text, for an index without names or without sequence, or when such a hit's
 * CIGAR breaks the reference's asserts (an intron shorter than 2, operations that do not end at re) or holds an operation code above 9. */
int mm_gpu_format_batch(int n_frag, const int *seg_off, const int *n_seg, MM2AMD_BSEQ_PTR seq, const int *n_reg, void *const *reg,
                        const int *rep_len, char **out, size_t *out_len);
/* The same text in a buffer the library owns and reuses: *out stays valid until the next mm_gpu_format_batch_view call (or mm_gpu_destroy);
 * the caller writes it out (fwrite / write) and does not free it.  For pipeline step 2, which one thread runs at a time: a gigabyte of
 * records per mini-batch is then formatted into memory that is already mapped, instead of into a fresh block whose page faults cost more
 * than the formatting. */
int mm_gpu_format_batch_view(int n_frag, const int *seg_off, const int *n_seg, MM2AMD_BSEQ_PTR seq, const int *n_reg, void *const *reg,
                             const int *rep_len, const char **out, size_t *out_len);
/* The same text, byte for byte, with the records written on the device: one kernel (rec_text_kernel, one wavefront per record) writes what
 * mm_write_paf4 (format.c:425-458) and mm_write_sam3 (format.c:522-679) write for single-segment reads -- the fixed fields, the CIGAR with the
 * clips of write_sam_cigar (format.c:494-520), the tag block of write_tags (format.c:397-423), SA:Z: (format.c:638-664), cs (short and long) and
 * MD (format.c:171-254, :302-331) -- except SEQ and QUAL of a SAM record, which are copies of host bytes and are put in place by the host pool.
 * *out is a buffer the library owns, valid until the next mm_gpu_format_batch_dev call (or mm_gpu_destroy); the index and flags are the live
 * context's; with several replicas the first one's device does the work; the call may run beside mm_gpu_map_staged.  *path says who wrote the
 * text.  The whole batch goes to the host writer (MM2AMD_FMT_PATH_HOST -- still the right bytes) when a fragment has n_seg != 1, MM_F_OUT_DS is
 * set, MM_F_COPY_COMMENT is set and a comment is present, a record's CIGAR has to go into the CG:B:I tag (MM_F_LONG_CIGAR, more than 65535
 * operations), a de / dv value lies outside [0, 1], or cs / MD is asked of an index without sequence.  Everything else, an empty batch
 * included, is written by the device.  MM2AMD_DEVICE_TEXT=1 in the environment routes mm_gpu_format_batch and mm_gpu_format_batch_view
 * through the same path (unset or 0: the host writer, as ever).
 * With MM_F_OUT_JUNC the junction lines are written by junc_text_kernel (one wavefront per hit that prints), for fragments of one and of two
 * segments alike and whatever the other flags; the device is the path also for a batch that prints nothing. */
#define MM2AMD_FMT_PATH_DEVICE 0
#define MM2AMD_FMT_PATH_HOST   1
int mm_gpu_format_batch_dev(int n_frag, const int *seg_off, const int *n_seg, MM2AMD_BSEQ_PTR seq, const int *n_reg, void *const *reg,
                            const int *rep_len, const char **out, size_t *out_len, int *path);

/* free() every reg[i][j].p and reg[i] (what the reference's step 2 does, map.c:629-631); for non-C callers. */
void mm2amd_free_regs(int n_frag, int *n_reg, MM2AMD_REG_PP reg);

/* Hit records of a (shard of a) batch as one flat payload -- the unit of the multi-GPU hit gather.  pack returns the
 * number of bytes needed/written (call with buf == NULL to size it); unpack rebuilds libc-allocated reg[] arrays. */
int64_t mm2amd_pack_regs(int n_frag, const int *n_reg, void *const *reg, uint8_t *buf, int64_t cap);
int mm2amd_unpack_regs(const uint8_t *buf, int64_t size, int n_frag, int *n_reg, MM2AMD_REG_PP reg);

/* Releases the device mirror; call before mm_idx_destroy (main.c:501). */
void mm_gpu_destroy(void);
/* The mapping context is process-wide, like the reference's pipeline: a later mm_gpu_init* replaces it.  Bindings whose objects
 * can outlive each other (two Python Aligner objects) remember the generation their init produced and tear down only that one. */
uint64_t mm_gpu_context_generation(void);        /* of the live context; 0: none */
int mm_gpu_destroy_if(uint64_t generation);      /* 1: it was the live context and is gone now; 0: left alone */

/* Mapping against a multi-part index, minimap2's --split-prefix (splitidx.c, map.c:476-539, :589-600, :693-736).  First pass, once per index
 * part: map with opt->split_prefix set (the hits' dp_max is then left for the merge to rank, align.c:1114) and hand every mapped batch to a writer;
 * PREFIX.NNNN.tmp has the reference's layout byte for byte -- k, n_seq, per sequence name length, name and length; per read segment n_reg, rep_len,
 * frag_gap; per hit the raw mm_reg1_t, with MM_F_CIGAR (read from *opt at every write) followed by capacity and the mm_extra_t block of capacity
 * words -- except the eight bytes of mm_reg1_t::p, which are zero.  The reference's mm_split_merge reads these files.
 * Merge pass: mm2amd_split_merge_open does what mm_split_merge_prep does (the files' headers become an index of names and lengths, the rid shift
 * of every part, k); MM2AMD_EINVAL for MM_F_OUT_CS / _MD / _DS / _JUNC in opt->flag, as the reference refuses cs and MD.  _batch takes the next
 * mini-batch of reads IN FILE ORDER (seq: mm_bseq1_t records, l_seq is read) and returns per segment a libc block of mm_reg1_t (mm2amd_free_regs),
 * rep_len (the largest of the parts) and frag_gap (the first part's): the records of all parts in part order, mm_update_dp_max for long reads,
 * the hit-list rules (on hits_merge_kernel with MM2AMD_DEVICE_MERGE=1, on the host's routines with 0 and by default), mm_set_mapq2, mm_pair for
 * two-segment fragments.  _format gives the SAM / PAF text of a merged batch in a malloc'd block (the host writer over the names-only index),
 * _sq the "@SQ" lines of all parts in part order (malloc'd), _close ends the pass and with remove_tmp removes the files. */
void *mm2amd_split_open(const char *prefix, const mm2amd_index_t *idx, int part_no);
int mm2amd_split_write(void *w, const void *opt, int n_seq, const int *n_reg, void *const *reg, const int *rep_len, const int *frag_gap);
int mm2amd_split_close(void *w);
void *mm2amd_split_merge_open(const char *prefix, int n_parts, const void *opt);
int mm2amd_split_merge_batch(void *h, int n_frag, const int *seg_off, const int *n_seg, const void *seq, int *n_reg, void **reg, int *rep_len, int *frag_gap);
int mm2amd_split_merge_format(void *h, int n_frag, const int *seg_off, const int *n_seg, const void *seq, const int *n_reg, void *const *reg, const int *rep_len,
                              char **out, size_t *out_len);
int mm2amd_split_merge_sq(void *h, char **out, size_t *out_len);
int mm2amd_split_merge_close(void *h, int remove_tmp);

const char *mm2amd_backend_name(void);           /* "hip:gfx950" in the product library */
int mm2amd_format_fraction(double v, char *buf); /* diagnostics: the output stage's "%.4f" (de:f / dv:f tags; no printf: exact integer arithmetic) into buf[>= 16]; returns the length */
int mm2amd_last_stats(double *v, int n);         /* per-stage wall times of the last batch (diagnostics) */

/* Per-kernel timing (HIP events on the launch stream) and algorithmic bytes, accumulated while enabled. */
typedef struct { char name[48]; double ms; double alg_bytes; int64_t launches; double units; } mm2amd_kernel_stat_t; /* units: DP cells (DP kernels) */
void mm2amd_profile_enable(int on);              /* also clears the accumulated statistics */
int mm2amd_profile_get(mm2amd_kernel_stat_t *out, int cap); /* returns the number of kernels written */

#ifdef __cplusplus
}
#endif
#endif
