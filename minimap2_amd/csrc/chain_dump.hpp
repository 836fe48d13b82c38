// MM2AMD_CHAIN_DUMP=<file>: every read's chains as the chaining step left them, one block per read and chaining pass -- the twin of
// MM2AMD_SEED_DUMP one stage later (tests/test_gpu_chains.py compares the blocks with the reference's CN lines and with mg_lchain_dp /
// mg_lchain_rmq run on the dumped anchors).  Diagnostics only: the variable is read once per seed_chain() call, and nothing here runs without it.
//
// A block (tab-separated fields; 64-bit words as hexadecimal, separated by blanks):
//   CH  name  qlen  pass  side  state     pass: 1 = the first chaining, 2 = the long-join re-chain (map.c:283-292); side: dev | host;
//                                         state: chained | handed-back (the RMQ kernel left the read to the host: no chains in this block)
//   PR  gap_ref gap_qry bw max_chain_skip max_chain_iter min_cnt min_chain_score chn_pen_gap chn_pen_skip is_cdna n_seg rmq rmq_inner_dist
//       rmq_size_cap bw_long mid_occ      the parameters of the call (the two penalties as %a: the floats round-trip)
//   IN  n  x y x y ...                    the sorted anchors that entered the pass ("IN -": not recorded -- the re-chain's input is the sorted first pass)
//   KP  n  redone                         only with MM2AMD_CHAIN_DUMP_KEPT=1, and only where isolated anchors were pruned before the sort (seed_chain.hip:
//                                         anchor_sort_prune_kernel): how many of the IN anchors the chaining kernels were given; 1 = the read was sorted unpruned after all
//   U   n  u u ...                        the chains, in order: score << 32 | anchors
//   A   n  x y x y ...                    the chained anchors, chain by chain
//   END
#pragma once
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>

#include "backend.hpp"

namespace mm2amd {

inline const char *chain_dump_path() { return getenv("MM2AMD_CHAIN_DUMP"); }

struct ChainDumpBlock {
	const char *name = nullptr;
	int qlen = 0, n_seg = 1, pass = 1;
	bool host = false, handed_back = false;
	const Anchor *in = nullptr; // null: not recorded
	int64_t n_in = 0;
	int64_t n_kept = -1;        // >= 0: the call pruned isolated anchors, and this many of the read's went on to the chaining
	bool redone = false;        // ... after the unpruned sort took the read over (duplicated keys, too many survivors): n_kept == n_in
	const uint64_t *u = nullptr;
	int32_t n_u = 0;
	const Anchor *a = nullptr;
	int64_t n_a = 0;
};

inline void chain_dump_words(std::string &s, const char *tag, int64_t n, const uint64_t *w, int64_t n_words)
{
	char buf[40];
	snprintf(buf, sizeof(buf), "%s\t%lld\t", tag, (long long)n);
	s += buf;
	for (int64_t i = 0; i < n_words; ++i) {
		snprintf(buf, sizeof(buf), i ? " %llx" : "%llx", (unsigned long long)w[i]);
		s += buf;
	}
	s += '\n';
}

// formats blocks into `s`; chain_dump_flush() appends them to the file under the one mutex both writers share
inline void chain_dump_format(std::string &s, const SeedChainParams &P, const ChainDumpBlock &b)
{
	static_assert(sizeof(Anchor) == 16, "an anchor is two 64-bit words");
	char buf[512];
	int gap_ref, gap_qry;
	chain_gaps(P, b.qlen, &gap_ref, &gap_qry);
	snprintf(buf, sizeof(buf), "CH\t%s\t%d\t%d\t%s\t%s\n", b.name ? b.name : "*", b.qlen, b.pass, b.host ? "host" : "dev", b.handed_back ? "handed-back" : "chained");
	s += buf;
	snprintf(buf, sizeof(buf), "PR\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%a\t%a\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", gap_ref, gap_qry, P.bw, P.max_chain_skip, P.max_chain_iter, P.min_cnt,
	         P.min_chain_score, (double)P.chn_pen_gap, (double)P.chn_pen_skip, P.is_cdna, b.n_seg, P.rmq || P.anchors_only ? 1 : 0, P.rmq_inner_dist, P.rmq_size_cap, P.bw_long, P.mid_occ);
	s += buf;
	if (b.in) chain_dump_words(s, "IN", b.n_in, (const uint64_t *)b.in, 2 * b.n_in);
	else s += "IN\t-\n";
	static const bool kept_lines = getenv("MM2AMD_CHAIN_DUMP_KEPT") != nullptr;
	if (kept_lines && b.n_kept >= 0) { snprintf(buf, sizeof(buf), "KP\t%lld\t%d\n", (long long)b.n_kept, b.redone ? 1 : 0); s += buf; }
	int64_t n_a = 0;
	for (int32_t k = 0; k < b.n_u; ++k) n_a += (int32_t)b.u[k];
	if (n_a != b.n_a) { snprintf(buf, sizeof(buf), "ERR\tchains of %lld anchors, %lld anchors\n", (long long)n_a, (long long)b.n_a); s += buf; n_a = n_a < b.n_a ? n_a : b.n_a; }
	chain_dump_words(s, "U", b.n_u, b.u, b.n_u);
	chain_dump_words(s, "A", n_a, (const uint64_t *)b.a, 2 * n_a);
	s += "END\n";
}

inline void chain_dump_flush(const char *path, const std::string &s)
{
	static std::mutex mu;
	std::lock_guard<std::mutex> lk(mu);
	if (FILE *fp = fopen(path, "a")) {
		fwrite(s.data(), 1, s.size(), fp);
		fclose(fp);
	}
}

} // namespace mm2amd
