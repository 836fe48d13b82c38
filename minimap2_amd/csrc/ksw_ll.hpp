// The local (Smith-Waterman) score with end coordinates of ksw_ll_qinit + ksw_ll_i16 (ksw2_ll_sse.c:37-152), on the host and on the device.
//   ll_local_score (ksw_ll.cpp)    the scalar host routine: every input, the striped scan's saturation and lazy-F behaviour included;
//   ksw_ll_kernel (ksw_ll_dev.hpp) the plain affine recurrence with one 32-bit key per query column, for the jobs of the plain class below,
//                                   where both give the same (score, qe, te).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace mm2amd {

int ll_local_score(int qlen, const uint8_t *query, int tlen, const uint8_t *target, const int8_t mat[25], int gapo, int gape, int *qe, int *te);

// The plain class: the striped routine's matrix is the plain affine local matrix whenever opening a gap right after a gap of the other kind cannot
// beat a substitution, and nothing saturates (gapo >= 1: with a free gap opening the striped routine itself leaves the plain matrix --
// tests/cpucheck/ksw_ll_test.cpp shows both).  Lengths are those of a non-empty job.
inline bool ll_plain_class(int qlen, int tlen, const int8_t mat[25], int gapo, int gape)
{
	int worst = 0, best = 0;
	for (int k = 0; k < 25; ++k) worst = std::min<int>(worst, mat[k]), best = std::max<int>(best, mat[k]);
	return -worst <= 2 * (gapo + gape) && gapo >= 1 && gape > 0 && (long)best * std::min(qlen, tlen) < 32000 && static_cast<unsigned>(gapo + gape) < 16000u;
}

constexpr int kLlCols = 4;                  // query columns a lane owns
constexpr int kLlStrip = 64 * kLlCols;      // columns of a strip: one wavefront's width
constexpr int kLlWgWaves = 8;               // wavefronts of a workgroup in the wg class
constexpr int kLlBlock = 64;                // target rows per boundary block; the wg class has a block barrier after every block of steps
constexpr int kLlLagBlocks = 3;             // blocks a wave of the wg class runs behind its left neighbour
constexpr int kLlMaxLen = 65535;            // a row index has 16 bits of the key
constexpr int64_t kLlWgMinCells = 1 << 22;  // jobs of at least this many cells (and more than one strip) take the wg class
constexpr uint32_t kLlQRev = 1, kLlQComp = 2, kLlTRev = 4; // MM2AMD_LL_*

struct LlJob {
	uint64_t q_off, t_off;   // the job's codes in the byte pools, as the caller gave them (the flags are applied while reading)
	uint64_t bnd_off;        // the job's boundary columns in the work buffer (32-bit words): one per wave, ll_bnd_words(tlen) each
	int32_t qlen, tlen;
	uint32_t flag;
	uint32_t out;            // the record in res this job writes
};
struct LlRes { int32_t score, qe, te, pad; };

struct LlParams {
	const LlJob *jobs; int n_jobs;
	int n_waves;             // 1: the wave class; kLlWgWaves: the wg class
	const uint8_t *qpool, *tpool;
	uint32_t *bnd;
	LlRes *res;
	uint32_t sc_lo[5];       // per query code: the scores against target codes 0..3, one byte each
	int32_t sc_hi[5];        // ... and against target code 4
	int32_t goe, ge;
};

constexpr size_t ll_bnd_words(int tlen) { return ((size_t)tlen + 2 * kLlBlock + kLlBlock - 1) / kLlBlock * kLlBlock; } // whole blocks, one to spare for the read-ahead

void ksw_ll_launch(const LlParams &P, void *stream);

} // namespace mm2amd
