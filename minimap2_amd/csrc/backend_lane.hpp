// HipBackend's state (backend_hip.cpp).  Between calls: the resident batch, and a lane's stream and work buffers grouped by the stage that fills them.
// Within a seed_chain() call: what its steps share (SeedCall, SortClasses).  Host code only: no .hip file includes this header.
#pragma once
#include <cstdint>
#include <vector>
#include "chain_dump.hpp"
#include "hip_util.hpp"
#include "kernel_prof.hpp"
#include "ksw_host.hpp"
#include "region_dev.hpp"
#include "sdust.hpp"
#include "seed_chain_dev.hpp"
#include "stage_run.hpp"

namespace mm2amd {

// The resident batch (shared by all lanes, read-only during run).  HipBackend holds two: begin_batch() fills the one that is NOT being mapped.
struct Resident {
	DevBuf<uint8_t> d_qpool;
	DevBuf<uint64_t> d_seq_off;
	PinBuf<char> h_ascii;
	std::vector<uint64_t> seq_off;
	// pairs: unit = one read of a pair (or a single read); see begin_batch
	bool has_pairs = false;
	size_t n_units = 0;
	std::vector<uint64_t> unit_off;
	std::vector<int32_t> unit_first;
	DevBuf<uint64_t> d_unit_off;
	DevBuf<int32_t> d_unit_first;
	// all-vs-all name rules: two ranks per read (see skip_hit in seed_chain.hip)
	bool have_read_names = false;
	std::vector<int32_t> name_key;
	DevBuf<int32_t> d_name_key;
	std::vector<const char *> read_names; // diagnostics: filled only under MM2AMD_SEED_DUMP or MM2AMD_CHAIN_DUMP, for the dumps' name columns
};

// What a chaining pass's backtrack leaves on the host (HipBackend::queue_pass_counts, queue_pass_chains)
struct ChainPassHost {
	PinBuf<unsigned long long> cursor; // [0] chained anchors, [1] chains, over the whole launch
	PinBuf<int32_t> nu, nv;            // per read: chains, chained anchors
	PinBuf<uint64_t> aoff, uoff;       // per read: where they start in `a` / `u` (and in the backtrack's device output)
	PinBuf<uint32_t> tie;              // per read: the RMQ kernel left it to the host
	PinBuf<Anchor> a;                  // the chained anchors (not copied while the chains stay on the device)
	PinBuf<uint64_t> u;                // the chains: score << 32 | anchors
	uint64_t n_v() const { return cursor.p[0]; }
	uint64_t n_u() const { return cursor.p[1]; }
};

struct Lane {
	int id = 0;
	int set = 0; // the resident set (HipBackend::res_) this lane's calls work on: Backend::bind_lane
	hipStream_t stream = nullptr;
	SeedChainBuffers B{};
	KswRunner ksw;
	DevBuf<uint8_t> d_tbytes; // ksw(): a call's composed targets

	// ---- seeding: minimizers, their seeds, the dust regions, the per-read counts
	DevBuf<uint32_t> d_mz_cnt;
	DevBuf<uint64_t> d_mz_x, d_mz_y;
	DevBuf<uint32_t> d_sd_n, d_sd_off, d_sd_aoff, d_sd_qpos, d_sd_info;
	DevBuf<uint32_t> d_sdust_list;
	DevBuf<SdustCounters> d_sdust_cnt;
	PinBuf<SdustCounters> h_sdust_cnt;
	PinBuf<uint32_t> h_dust_n, h_dust_s, h_dust_e;
	DevBuf<uint32_t> d_n_anchor, d_n_minipos, d_n_seedhit;
	DevBuf<int32_t> d_rep_len;
	PinBuf<uint32_t> h_na, h_nmp;
	PinBuf<int32_t> h_rep;
	std::vector<uint64_t> a_off, mp_off; // the reads' anchor / mini_pos offsets (mp_off: fetch_chains and align_regions read it too)
	PinBuf<uint64_t> h_off;
	DevBuf<uint64_t> d_a_off, d_mp_off;
	DevBuf<uint64_t> d_minipos;
	PinBuf<uint64_t> h_minipos;

	// ---- sort + chain: the anchors, the sort's scratch and work list, pruning, the chaining arrays, the backtrack's output
	DevBuf<Anchor> d_anchors;
	DevBuf<uint64_t> d_skey_in, d_sval_in, d_skey_out, d_sval_out;
	DevBuf<uint32_t> d_tie;
	DevBuf<uint32_t> d_sort_list;
	PinBuf<uint32_t> h_sort_list;
	DevBuf<uint32_t> d_nkept;
	PinBuf<uint32_t> h_nkept;
	DevBuf<Anchor> d_dump_anchors; // MM2AMD_CHAIN_DUMP with pruning: the unpruned sort's output, for the IN blocks
	DevBuf<int32_t> d_f, d_p, d_t;
	DevBuf<uint32_t> d_pieces;     // the chaining kernels' work list when a read of the launch is cut into pieces (make_pieces)
	PinBuf<uint32_t> h_pieces;
	DevBuf<unsigned long long> d_bt_cursor;
	DevBuf<Anchor> d_bt_out_a;
	DevBuf<uint64_t> d_bt_out_u, d_bt_aoff, d_bt_uoff;
	DevBuf<int32_t> d_bt_nu, d_bt_nv;
	DevBuf<int32_t> d_span; PinBuf<int32_t> h_span; // lazy chains: the first chain's ends, all that long_join needs of the anchors
	PinBuf<Anchor> h_redo;         // the sorted anchors of the reads the RMQ kernel handed back

	// ---- the two chaining passes' host copies.  (pass1.a also carries the anchors-only hand-over's sorted anchors.)
	ChainPassHost pass1, pass2;

	// ---- long-join: the re-chain's own buffers.  Its offsets, work list, tie flags and per-read backtrack counts go through the first pass's d_a_off, d_sort_list,
	// d_tie and d_bt_cursor / d_bt_nu / d_bt_nv / d_bt_aoff / d_bt_uoff, which are dead by then (copied out); only the first pass's CHAINS (d_bt_out_a, d_bt_out_u)
	// must survive, as the re-chain's input and for align_regions -- so the second backtrack writes its chains here
	DevBuf<uint64_t> d_lj_src;
	DevBuf<Anchor> d_lj_out_a;
	DevBuf<uint64_t> d_lj_out_u;
	PinBuf<uint64_t> h_lj_off;
	PinBuf<uint32_t> h_lj_list, h_lj_pieces;

	// ---- finish_regions (region_finish.hip)
	DevBuf<FinRegion> d_fin_regions; DevBuf<FinPiece> d_fin_pieces; DevBuf<uint32_t> d_fin_out; DevBuf<FinResult> d_fin_res;
	PinBuf<FinRegion> h_fin_regions; PinBuf<FinPiece> h_fin_pieces; PinBuf<uint32_t> h_fin_out; PinBuf<FinResult> h_fin_res;
	EqxBufs eqx_fin;

	// ---- pair_begin / pair_run (pair.hpp): the caller's tables in pinned memory, the launch's buffers
	PairBufs pair;
	PinBuf<mm2amd_pe_frag_t> h_pe_frag; PinBuf<mm2amd_pe_hit_t> h_pe_hits; PinBuf<mm2amd_pe_out_t> h_pe_out; PinBuf<mm2amd_pe_res_t> h_pe_res;

	// ---- align_regions (region_dev.hpp): the lane's last seed_chain() in device terms, the hit / window / piece arrays, the results' host copies
	long rg_lo = 0; size_t rg_n = 0; uint64_t rg_n_v = 0, rg_n_v2 = 0, rg_n_u = 0, rg_n_u2 = 0;
	bool rg_lazy = false;
	DevBuf<RgnRead> d_rg_reads; PinBuf<RgnRead> h_rg_reads;
	DevBuf<Anchor> d_rg_sq; DevBuf<ref::Reg1> d_rg_regs; DevBuf<RgnAux> d_rg_aux; DevBuf<RgnReadOut> d_rg_rout; DevBuf<unsigned int> d_rg_cur;
	DevBuf<RgnPlan> d_rg_plan; DevBuf<RgnWin> d_rg_win; DevBuf<KswJob> d_rg_jobs; DevBuf<int32_t> d_rg_sites; DevBuf<FinRegion> d_rg_fin; DevBuf<FinPiece> d_rg_pieces;
	DevBuf<FinResult> d_rg_finres; DevBuf<uint32_t> d_rg_out;
	PinBuf<ref::Reg1> h_rg_regs; PinBuf<RgnAux> h_rg_aux; PinBuf<RgnReadOut> h_rg_rout; PinBuf<unsigned int> h_rg_cur; PinBuf<RgnPlan> h_rg_plan; PinBuf<KswJob> h_rg_jobs;
	PinBuf<FinRegion> h_rg_fin; PinBuf<FinResult> h_rg_finres; PinBuf<uint32_t> h_rg_out;
	EqxBufs eqx_rg; // apart from eqx_fin: the views align_regions hands out live on while the hand-backs' rounds call finish_regions

	// ---- fetch_chains: device chains gathered for the host path
	DevBuf<RgnGather> d_gather; PinBuf<RgnGather> h_gather;
	DevBuf<Anchor> d_fetch_a; DevBuf<uint64_t> d_fetch_mp; PinBuf<Anchor> h_fetch_a; PinBuf<uint64_t> h_fetch_mp;

	~Lane() { if (stream) (void)hipStreamDestroy(stream); }
};

// One seed_chain() call: what its steps share.  n_a / n_mp are known once size_anchors() has the per-read counts.
struct SeedCall {
	const SeedChainParams &P;
	Lane &ln;
	const Resident &R;
	KernelProfiler &kp;
	const long lo, hi;
	const int lane_id, n_threads;
	hipStream_t st;
	SeedChainBuffers &B;        // the lane's: long_join starts from it
	const size_t n;             // reads (fragments)
	const size_t ulo, n_unit;   // the units encoding and sketching run over (see begin_batch); without pairs a unit is a fragment
	const uint64_t base0, cap_mz; // the sub-batch's first base and its bases: the minimizer arrays have a slot per base
	const double L, est_mz;     // bases as the byte counts take them; minimizers expected
	uint64_t n_a = 0, n_mp = 0; // anchors, minimizer positions
	SeedCall(const SeedChainParams &P_, Lane &ln_, const Resident &R_, KernelProfiler &kp_, long lo_, long hi_, int lane_id_, int n_threads_)
		: P(P_), ln(ln_), R(R_), kp(kp_), lo(lo_), hi(hi_), lane_id(lane_id_), n_threads(n_threads_), st(ln_.stream), B(ln_.B), n((size_t)(hi_ - lo_)),
		  ulo(R_.has_pairs ? (size_t)R_.unit_first[lo_] : (size_t)lo_), n_unit(R_.has_pairs ? (size_t)R_.unit_first[hi_] - ulo : n),
		  base0(R_.seq_off[lo_]), cap_mz(R_.seq_off[hi_] - base0), L((double)(R_.seq_off[hi_] - R_.seq_off[lo_])), est_mz(2.0 * L / (P_.w + 1)) {}
	int qlen(size_t i) const { return (int)(R.seq_off[lo + i + 1] - R.seq_off[lo + i]); }
	ChainDumpBlock dump_block(size_t i) const // what every chain-dump block of read i of this call says about the read
	{
		ChainDumpBlock b;
		b.name = R.read_names.empty() ? nullptr : R.read_names[lo + i];
		b.qlen = qlen(i), b.n_seg = R.has_pairs ? R.unit_first[lo + i + 1] - R.unit_first[lo + i] : 1;
		return b;
	}
};

// The per-read anchor sort's launch classes (by anchors per read) over the reads of one launch: the reads of a class are listed together
struct SortClasses {
	int n_class[kAnchorSortClasses] = { 0 }, class_first[kAnchorSortClasses + 1] = { 0 };
	double a_class[kAnchorSortClasses] = { 0 };
	int n_listed() const { return class_first[kAnchorSortClasses]; }
};

} // namespace mm2amd
