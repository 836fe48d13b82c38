// sdust_kernel (sdust_dev.hpp, compiled with seed_chain.hip): the masked regions of sdust() (sdust.h / sdust.c:134-175, W = 64) for a batch of reads,
// one wavefront per read -- DESIGN.md section 3e has the formulation and the bound of every loop.  Host-side declarations.
#pragma once
#include <cstdint>

namespace mm2amd {

// The list P of perfect intervals lives in LDS as packed dwords.  Narrow class: kSdustNarrowCap entries (4.5 KB per wavefront with the two
// 64-entry bucket arrays in front: 32 wavefronts, a CU's wave slots, fit its 160 KB of LDS).  A read whose list would grow beyond that stops and
// lists itself; the wide class scans the listed reads again from their first base with kSdustWideCap entries (16.5 KB: 9 wavefronts per CU), which
// no list exceeds: an entry lives at most 62 steps and a step adds at most 62 (SdustState::PCAP).
constexpr int kSdustNarrowCap = 1024;
constexpr int kSdustWideCap = 4096;
constexpr int kSdustMaxLen = 1 << 30;   // positions are int32 and a finish lies up to 66 beyond a start
constexpr int kSdustMaxT = 1 << 20;     // thresholds are clamped here: nothing is masked from 18 911 on (r <= 1891), and products with T stay in int32
constexpr int kSdustWideGrid = 2048;    // blocks of the wide launch when the list's length is not known on the host: block b takes entries b, b + grid, ...
constexpr int kSdustPathNarrow = 0, kSdustPathWide = 1; // MM2AMD_SDUST_PATH_*

struct SdustCounters {
	unsigned long long narrow_partial;  // bases the narrow class scanned of the reads it handed on
	unsigned long long wide_bases;      // bases of the reads the wide class scanned
	uint32_t n_wide;                    // entries of wide_list
	uint32_t err;                       // a list outgrew the wide capacity (cannot happen: see above)
};

struct SdustParams {
	const uint8_t *codes;   // read r's nt4 codes (anything >= 4 breaks the sequence): codes + code_mul * off[r], off[r + 1] - off[r] of them
	const uint64_t *off;    // n_reads + 1
	int code_mul;           // 1, or 2 for the mapper's query pool (forward | reverse complement per read)
	int n_reads, T, cap;    // cap: list entries in LDS
	int wide;               // 0: narrow class, read = block; 1: wide class from wide_list; 2: wide class, every read
	uint32_t *reg_n, *reg_s, *reg_e; // out, in the read's own slots: reg_n[off[r]] regions, region k = [reg_s[off[r] + k], reg_e[off[r] + k])
	uint32_t *wide_list;    // n_reads entries
	SdustCounters *cnt;
};

size_t sdust_lds_bytes(int cap);
// grid: blocks of a launch from the list (wide == 1); 0 = kSdustWideGrid or n_reads, whichever is smaller
void sdust_launch(const SdustParams &P, int grid, void *stream);
// the regions of a batch packed job by job: cnt_out[r] = regions of read r (0 for an empty read) / out[out_off[r] + k] = start << 32 | finish
void sdust_count_launch(const SdustParams &P, uint32_t *cnt_out, void *stream);
void sdust_pack_launch(const SdustParams &P, const uint64_t *out_off, uint64_t *out, void *stream);

} // namespace mm2amd
