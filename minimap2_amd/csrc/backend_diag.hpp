// HipBackend's diagnostics (backend_hip.cpp calls each in one line behind its switch): the MM2AMD_TIE_COUNT report, the MM2AMD_SEED_DUMP writer, the
// chain-dump blocks (chain_dump.hpp) of the anchors-only hand-over, the first pass and the long-join pass, and the MM2AMD_FIN_CHECK walk.  Nothing here runs
// without its switch; what they write is parsed by the tests, byte for byte.  Host code only: no .hip file includes this header.
#pragma once
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>
#include "backend_lane.hpp"
#include "chain_dump.hpp"

namespace mm2amd {

// MM2AMD_TIE_COUNT: how many reads of this sub-batch had two anchors with the same x (the replayed ones)
inline void report_tie_count(const SeedCall &c, const SortClasses &cls)
{
	std::vector<uint32_t> tf(c.n);
	stream_wait(c.st);
	HIP_CHECK(hipMemcpy(tf.data(), c.ln.d_tie.p, c.n * 4, hipMemcpyDeviceToHost));
	size_t n_tied = 0;
	for (size_t i = 0; i < c.n; ++i) n_tied += tf[i] != 0;
	fprintf(stderr, "[mm2amd] anchor sort: %zu of %zu reads have duplicated keys (%d / %d / %d reads in the 7 k / 10 k / global classes)\n", n_tied, c.n, cls.n_class[3], cls.n_class[4], cls.n_class[5]);
}

// MM2AMD_SEED_DUMP=<file>: every read's sorted anchors, as the reference's --print-seeds prints them (map.c:255-260)
inline void write_seed_dump(const SeedCall &c, const char *dump, const std::vector<std::string> &ref_names)
{
	const std::vector<uint64_t> &a_off = c.ln.a_off;
	const std::vector<const char *> &names = c.R.read_names;
	std::vector<Anchor> all(c.n_a + 1);
	stream_wait(c.st);
	if (c.n_a) HIP_CHECK(hipMemcpy(all.data(), c.ln.d_anchors.p, c.n_a * sizeof(Anchor), hipMemcpyDeviceToHost));
	static std::mutex dump_mu;
	std::lock_guard<std::mutex> lk(dump_mu);
	const bool dump_flags = getenv("MM2AMD_SEED_DUMP_FLAGS") != nullptr; // one more column: the anchor's tandem flag
	FILE *fp = fopen(dump, "a");
	if (!fp) return;
	for (size_t i = 0; i < c.n; ++i) {
		fprintf(fp, "QR\t%s\t%d\nRS\t%d\n", names.empty() || !names[c.lo + i] ? "*" : names[c.lo + i], c.P.mid_occ, c.ln.h_rep.p[i]);
		for (uint64_t j = a_off[i]; j < a_off[i + 1]; ++j) {
			const Anchor &a = all[j];
			fprintf(fp, "SD\t%s\t%d\t%c\t%d\t%d\t%d", ref_names[a.x << 1 >> 33].c_str(), (int32_t)a.x, "+-"[a.x >> 63], (int32_t)a.y, (int32_t)(a.y >> 32 & 0xff),
			        j == a_off[i] ? 0 : ((int32_t)a.y - (int32_t)all[j - 1].y) - ((int32_t)a.x - (int32_t)all[j - 1].x));
			if (dump_flags) fprintf(fp, "\t%d", (int)(a.y >> 42 & 1)); // MM_SEED_TANDEM, which the reference's line leaves out
			fputc('\n', fp);
		}
	}
	fclose(fp);
}

// ---- the chain dump.  One builder (SeedCall::dump_block) says what every block says about its read; these add what a pass knows.
// a block's chains: read k of pass H, whose chained anchors are at `chained` (H.a, or a copy fetched for the dump)
inline void dump_block_chains(ChainDumpBlock &b, const ChainPassHost &H, size_t k, const Anchor *chained)
{
	b.u = H.u.p + H.uoff.p[k], b.n_u = H.nu.p[k], b.a = chained + H.aoff.p[k], b.n_a = H.nv.p[k];
}

// The anchors-only hand-over: every read is handed back, the caller's blocks (mapper.cpp) hold the chains.  ha: the sorted anchors on the host
inline void dump_anchors_only(const SeedCall &c, const char *cdump, const Anchor *ha)
{
	const std::vector<uint64_t> &a_off = c.ln.a_off;
	std::string txt;
	for (size_t i = 0; i < c.n; ++i) {
		ChainDumpBlock b = c.dump_block(i);
		b.handed_back = true, b.in = ha + a_off[i], b.n_in = (int64_t)(a_off[i + 1] - a_off[i]);
		chain_dump_format(txt, c.P, b);
	}
	chain_dump_flush(cdump, txt);
}

// The first pass: the sorted anchors that went in (dump_full: the unpruned sort's, from their own buffer) and the chains as the backtrack left them (with lazy
// chains the anchors are still on the device: copied here only).  tie: the reads the RMQ kernel handed back, or null
inline void dump_first_pass(const SeedCall &c, const char *cdump, const SortClasses &cls, bool prune, bool dump_full, bool lazy, const uint32_t *tie)
{
	Lane &ln = c.ln;
	const size_t n = c.n;
	const ChainPassHost &H = ln.pass1;
	const std::vector<uint64_t> &a_off = ln.a_off;
	const uint32_t *h_nkept = ln.h_nkept.p;
	std::vector<Anchor> all(c.n_a + 1), bt(lazy ? H.n_v() + 1 : 0);
	if (c.n_a) HIP_CHECK(hipMemcpyAsync(all.data(), dump_full ? ln.d_dump_anchors.p : ln.d_anchors.p, c.n_a * sizeof(Anchor), hipMemcpyDeviceToHost, c.st));
	if (lazy && H.n_v()) HIP_CHECK(hipMemcpyAsync(bt.data(), ln.d_bt_out_a.p, H.n_v() * sizeof(Anchor), hipMemcpyDeviceToHost, c.st));
	stream_wait(c.st);
	std::vector<bool> redone(n, false); // (pruning: class k's redo list starts where the class's reads start in the sort's work list)
	if (prune) for (int k = 0; k + 1 < kAnchorSortClasses; ++k) for (uint32_t q = 0; q < h_nkept[n + k]; ++q) redone[h_nkept[n + 8 + cls.class_first[k] + q]] = true;
	std::string txt;
	for (size_t i = 0; i < n; ++i) {
		ChainDumpBlock b = c.dump_block(i);
		b.in = all.data() + a_off[i], b.n_in = (int64_t)(a_off[i + 1] - a_off[i]);
		if (prune) b.n_kept = (int64_t)h_nkept[i], b.redone = redone[i]; // (KP line)
		b.handed_back = tie && tie[i];
		if (!b.handed_back) dump_block_chains(b, H, i, lazy ? bt.data() : H.a.p);
		chain_dump_format(txt, c.P, b);
	}
	chain_dump_flush(cdump, txt);
}

// The long-join pass: the second blocks of the re-chained reads `sel`
inline void dump_long_join(const SeedCall &c, const char *cdump, const std::vector<uint32_t> &sel, bool lazy)
{
	Lane &ln = c.ln;
	const ChainPassHost &H = ln.pass2;
	std::vector<Anchor> bt(lazy ? H.n_v() + 1 : 0);
	if (lazy && H.n_v()) {
		HIP_CHECK(hipMemcpyAsync(bt.data(), ln.d_lj_out_a.p, H.n_v() * sizeof(Anchor), hipMemcpyDeviceToHost, c.st));
		stream_wait(c.st);
	}
	std::string txt;
	for (size_t k = 0; k < sel.size(); ++k) {
		ChainDumpBlock b = c.dump_block(sel[k]); // (long-join runs without pairs: one segment)
		b.pass = 2, b.handed_back = H.tie.p[k] != 0;
		if (!b.handed_back) dump_block_chains(b, H, k, lazy ? bt.data() : H.a.p);
		chain_dump_format(txt, c.P, b);
	}
	chain_dump_flush(cdump, txt);
}

// MM2AMD_FIN_CHECK: every CIGAR finish_regions returns must cover its region's windows
inline void fin_check(int lane_id, const std::vector<FinRegion> &regions, const std::vector<FinResult> &results, const uint32_t *out_pool)
{
	const size_t n = regions.size();
	for (size_t i = 0; i < n; ++i) {
		const FinResult &f = results[i];
		long q = f.qshift, t = f.tshift;
		for (int k = 0; k < f.n_cigar; ++k) {
			const uint32_t c = out_pool[regions[i].out_off + k], op = c & 0xf, len = c >> 4;
			if (op == 0 || op == 7 || op == 8) q += len, t += len;
			else if (op == 1) q += len;
			else if (op == 2 || op == 3) t += len;
		}
		if (f.n_cigar < 0 || q != regions[i].q_len || t != regions[i].t_len)
			fprintf(stderr, "[mm2amd] FIN_CHECK lane %d region %zu of %zu: n_cigar %d qshift %d tshift %d covers %ld/%ld of %d/%d (pieces %u from %u, out_off %u)\n", lane_id, i, n,
			        f.n_cigar, f.qshift, f.tshift, q, t, regions[i].q_len, regions[i].t_len, regions[i].n_pieces, regions[i].piece0, regions[i].out_off);
	}
}

} // namespace mm2amd
