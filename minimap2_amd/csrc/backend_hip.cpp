// The product's Backend: the host side of the hand-written gfx950 kernels, and the buffer management around them.  There is deliberately no CPU
// path here: constructing it without a usable HIP device throws.  What it drives, stage by stage:
//   seed_chain()      seed_chain.hip: encode, sketch, sdust (-T on the device) and the dust filter, seed collect / expand, the per-read anchor sort
//                     (device_sort.hip under it) with pruning, chain fill / RMQ, backtrack, the long-join re-chain
//   align_regions()   region_dev.hip (chains -> hits, window plan, consume); the DP kernels through KswRunner (ksw_host.cpp: ksw_order.hip and the
//                     ksw_extd2 / ksw_ext / ksw_extq / ksw_stream / ksw_band / ksw_gapfill / ksw_splice .hip launch classes); region_finish.hip's
//                     region_finish_kernel and cigar_eqx_kernel
//   ksw(), finish_regions(), fetch_chains()   the same DP, finish and =/X kernels for the host path's rounds, and the device chains a hand-back needs
//   rec_text_*(), junc_text_*()               region_finish.hip's record and junction text kernels, on a stream of their own
// The index tables are index_build.hip's (built by the caller, or mirrored here from a flattened reference index).
//
// A batch's sequences are made resident once (begin_batch).  The mapper then runs sub-batches of reads through the stage methods on independent
// LANES (backend_lane.hpp): each lane owns a HIP stream and its device/pinned work buffers, so several host driver threads can keep different
// sub-batches in flight and the GPU stages of one overlap the host stages of another.  The stage methods read as a list of steps; the steps are
// private members next to them, and what only a diagnostic switch runs is in backend_diag.hpp.
#include <atomic>
#include <condition_variable>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <numeric>
#include <stdexcept>
#include <thread>
#include "backend.hpp"
#include "backend_diag.hpp"
#include "backend_lane.hpp"
#include "capi_internal.hpp"
#include "chain_dump.hpp"
#include "chain_host.hpp"
#include "device_ctx.hpp"
#include "ksw_host.hpp"
#include "seed_chain_dev.hpp"
#include "index_build.hpp"
#include "kernel_prof.hpp"
#include "threads.hpp"
#include "trace.hpp"
#include "sdust_core.hpp"
#include "sdust.hpp"
#include "stage_run.hpp"
#include "tables.hpp"

namespace mm2amd {

namespace {

bool env_on(const char *name) { const char *e = getenv(name); return e && *e && strcmp(e, "0") != 0; }

// chains -> ReadChains: read k of pass H (dev_src 0: the first pass, 1: long-join); lazy: the anchors stayed on the device
void set_chains(ReadChains &c, const ChainPassHost &H, size_t k, bool lazy, int8_t dev_src)
{
	c.u_p = H.u.p + H.uoff.p[k], c.n_u = H.nu.p[k];
	c.a_p = lazy ? nullptr : H.a.p + H.aoff.p[k], c.n_a = H.nv.p[k];
	c.dev_src = dev_src, c.dev_a_off = H.aoff.p[k], c.dev_u_off = H.uoff.p[k];
}

class HipBackend : public Backend {
public:
	// `tables` may be null: the backend then mirrors the host tables of `fi` (an index flattened from a reference mm_idx_t)
	// `device` < 0: the process's default device.  `tables_device`: where `tables` live; a replica on another device copies them
	// (hipMemcpyPeer over xGMI), one on the same device shares them.
	HipBackend(const FlatIndex &fi, DeviceIndexTables *tables, int n_threads, int device, int replica, int tables_device) : T_(tables)
	{
		replica_ = replica;
		DeviceScope scope(device); DeviceCtx &d = scope.dc;
		dev_ = d.device_id;
		stream_ = d.stream;
		n_cu_ = d.n_cu;
		n_threads_ = n_threads > 0 ? n_threads : (int)std::max(1u, std::thread::hardware_concurrency());
		if (!T_) { own_.upload(fi, stream_); T_ = &own_; }
		else if (tables_device >= 0 && tables_device != dev_) { own_.clone_from(*T_, tables_device, dev_); T_ = &own_; }
		I_.bucket_start = T_->bucket_start.p, I_.keys = T_->keys.p, I_.val_off = T_->val_off.p, I_.slots = T_->slots.p, I_.first = getenv("MM2AMD_NO_FIRST_SLOT") ? nullptr : T_->first.p, I_.pos = T_->pos.p, I_.S = T_->S.p;
		I_.bucket_bits = T_->bucket_bits, I_.key_shift = T_->key_shift;
		I_.name_rank = nullptr, I_.seq_len = nullptr;
		fi_names_ = &fi.names, fi_seq_len_ = &fi.seq_len, fi_seq_off_ = &fi.seq_off; // fi outlives the backend (it is the mapper's index)
		while ((1ull << rid_bits_) < fi.n_seq) ++rid_bits_;
		n_lanes_ = 8; // sub-batches in flight.  Rounds 1-3: 5 (more made no difference while the lanes' waits spun on the CPU quota); with the lanes starting
		              // on the next batch early, 8-10 keep seeding, sorting and DP kernels of different sub-batches on the GPU together: +3-4 % (profiles/r04, call 16)
		if (const char *e = getenv("MM2AMD_LANES")) n_lanes_ = std::max(1, std::min(kMaxProfLanes - 1, atoi(e))); // (the last profiler slot is the record formatter's)
		for (int i = 0; i < n_lanes_; ++i) {
			lanes_.emplace_back(new Lane);
			lanes_.back()->id = i;
			HIP_CHECK(hipStreamCreateWithFlags(&lanes_.back()->stream, hipStreamNonBlocking));
			lanes_.back()->ksw.n_cu = n_cu_;
			lanes_.back()->ksw.disable_fast = getenv("MM2AMD_KSW_EXACT_ONLY") != nullptr;
		}
		// the lanes' work buffers come out of arenas (hip_util.hpp): the first chunks are taken now, before any batch, by a thread of its own -- the index tables are
		// still on their way to the device, and what a 100 000-read batch of long reads settles at (116 GB in eight lanes' buffers, 30 ms per GB of hipMalloc, 185 ms
		// per GB of pinned memory) is seconds of allocation that the first batch would otherwise pay for; never more than half of what the device has free
		{
			size_t free_b = 0, total_b = 0, want = arena_env_gb("MM2AMD_ARENA_DEV_GB", 112) << 30;
			if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) want = std::min(want, free_b / 2);
			const size_t want_pin = arena_env_gb("MM2AMD_ARENA_PIN_GB", 4) << 30;
			const int dev = dev_;
			if (MemArena::enabled() && (want || want_pin)) std::thread([dev, want, want_pin] {
				if (hipSetDevice(dev) != hipSuccess) return;
				try { pin_arena().reserve(want_pin); dev_arena().reserve(want); } catch (...) {} // (a reservation that fails leaves the buffers to allocate as they grow)
			}).detach();
		}
	}

	~HipBackend() override
	{
		(void)hipSetDevice(dev_);
		if (stage_stream_) (void)hipStreamDestroy(stage_stream_);
		for (int l = 0; l < n_lanes_; ++l) kernel_profiler(l, replica_).drop_events();
		kernel_profiler(kMaxProfLanes - 1, replica_).drop_events(); // (the record formatter's slot)
	}
	int n_lanes() const override { return n_lanes_; }
	void enable_name_rules() override
	{
		HIP_CHECK(hipSetDevice(dev_)); // HIP's current device is per thread, and the mapper drives every lane from a thread of its own
		if (name_rules_ || fi_names_->empty()) return;
		const std::vector<std::string> &nm = *fi_names_;
		sorted_names_ = nm;
		std::sort(sorted_names_.begin(), sorted_names_.end());
		sorted_names_.erase(std::unique(sorted_names_.begin(), sorted_names_.end()), sorted_names_.end());
		std::vector<int32_t> rank(nm.size());
		for (size_t i = 0; i < nm.size(); ++i) rank[i] = (int32_t)(std::lower_bound(sorted_names_.begin(), sorted_names_.end(), nm[i]) - sorted_names_.begin());
		d_name_rank_.ensure(nm.size()), d_ref_len_.ensure(nm.size());
		HIP_CHECK(hipMemcpyAsync(d_name_rank_.p, rank.data(), nm.size() * 4, hipMemcpyHostToDevice, stream_));
		HIP_CHECK(hipMemcpyAsync(d_ref_len_.p, fi_seq_len_->data(), nm.size() * 4, hipMemcpyHostToDevice, stream_));
		stream_wait(stream_);
		I_.name_rank = d_name_rank_.p, I_.seq_len = d_ref_len_.p;
		name_rules_ = true;
	}
	void enable_seq_len() override
	{
		HIP_CHECK(hipSetDevice(dev_)); // HIP's current device is per thread, and the mapper drives every lane from a thread of its own
		if (I_.seq_len) return;
		d_ref_len_.ensure(fi_seq_len_->size());
		HIP_CHECK(hipMemcpyAsync(d_ref_len_.p, fi_seq_len_->data(), fi_seq_len_->size() * 4, hipMemcpyHostToDevice, stream_));
		stream_wait(stream_);
		I_.seq_len = d_ref_len_.p;
	}
	bool supports_rmq() const override { return getenv("MM2AMD_RMQ_ON_HOST") == nullptr; } // chain_rmq_kernel; MM2AMD_RMQ_ON_HOST=1: A/B against rmq_chain.cpp
	void set_active_lanes(int n) override { active_lanes_ = std::max(1, std::min(n, n_lanes_)); }

	void begin_batch(const std::vector<ReadView> &reads, std::vector<uint64_t> &qpool_off) override
	{
		HIP_CHECK(hipSetDevice(dev_)); // HIP's current device is per thread, and the mapper drives every lane from a thread of its own
		Resident &R = res_[1 - cur_]; // the set that is not being mapped
		if (!stage_stream_) HIP_CHECK(hipStreamCreateWithFlags(&stage_stream_, hipStreamNonBlocking));
		const size_t n = reads.size();
		// fragment-level offsets (what seeding and chaining see: a pair is one query, the concatenation of its two reads) ...
		R.seq_off.resize(n + 1);
		R.seq_off[0] = 0;
		R.has_pairs = false;
		for (size_t i = 0; i < n; ++i) R.seq_off[i + 1] = R.seq_off[i] + (uint64_t)reads[i].total(), R.has_pairs |= reads[i].paired();
		const uint64_t total = R.seq_off[n];
		qpool_off.resize(n);
		for (size_t i = 0; i < n; ++i) qpool_off[i] = 2 * R.seq_off[i];
		char *h = R.h_ascii.ensure(total + 1);
		parallel_for_side(n_threads_, (long)n, [&](long i, int) {
			memcpy(h + R.seq_off[i], reads[i].seq, reads[i].len);
			if (reads[i].paired()) memcpy(h + R.seq_off[i] + reads[i].len, reads[i].seq2, reads[i].len2);
		}, 64);
		// The ASCII bases stay in the pinned host buffer: encode_kernel reads them from there, once, sub-batch by sub-batch (zero-copy
		// over PCIe, spread over the mapping step).  A bulk H2D copy of the next batch beside the mapping of the current one made the
		// mapping's own small, latency-critical copies queue behind it (profiles/r03: mapping calls 25 % slower in the pipeline).
		R.d_qpool.ensure(2 * total + 16);
		R.d_seq_off.ensure(n + 1);
		// ... and unit-level offsets (what encoding and sketching see: every read of a pair on its own, so that no k-mer spans the
		// two and each has its own forward | reverse-complement block in the query pool)
		R.n_units = n;
		if (R.has_pairs) {
			R.unit_first.resize(n + 1);
			R.unit_first[0] = 0;
			for (size_t i = 0; i < n; ++i) R.unit_first[i + 1] = R.unit_first[i] + (reads[i].paired() ? 2 : 1);
			R.n_units = (size_t)R.unit_first[n];
			R.unit_off.resize(R.n_units + 1);
			for (size_t i = 0; i < n; ++i) {
				R.unit_off[R.unit_first[i]] = R.seq_off[i];
				if (reads[i].paired()) R.unit_off[R.unit_first[i] + 1] = R.seq_off[i] + (uint64_t)reads[i].len;
			}
			R.unit_off[R.n_units] = total;
			R.d_unit_off.ensure(R.n_units + 1), R.d_unit_first.ensure(n + 1);
			HIP_CHECK(hipMemcpyAsync(R.d_unit_off.p, R.unit_off.data(), (R.n_units + 1) * 8, hipMemcpyHostToDevice, stage_stream_));
			HIP_CHECK(hipMemcpyAsync(R.d_unit_first.p, R.unit_first.data(), (n + 1) * 4, hipMemcpyHostToDevice, stage_stream_));
		}
		HIP_CHECK(hipMemcpyAsync(R.d_seq_off.p, R.seq_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, stage_stream_));
		R.read_names.clear();
		if (getenv("MM2AMD_SEED_DUMP") || chain_dump_path()) for (size_t i = 0; i < n; ++i) R.read_names.push_back(reads[i].name);
		R.have_read_names = false;
		if (name_rules_ && n > 0) { // strcmp(qname, target name) as two ranks per read (see skip_hit in seed_chain.hip)
			R.have_read_names = true;
			for (size_t i = 0; i < n; ++i) if (!reads[i].name) { R.have_read_names = false; break; } // the reference skips the rules without a name (map.c:81)
		}
		if (R.have_read_names) {
			R.name_key.resize(2 * n);
			parallel_for_side(n_threads_, (long)n, [&](long i, int) {
				const std::string q(reads[i].name);
				const size_t lb = (size_t)(std::lower_bound(sorted_names_.begin(), sorted_names_.end(), q) - sorted_names_.begin());
				R.name_key[i] = (int32_t)lb;
				R.name_key[n + i] = lb < sorted_names_.size() && sorted_names_[lb] == q ? (int32_t)lb : -1;
			}, 256);
			R.d_name_key.ensure(2 * n);
			HIP_CHECK(hipMemcpyAsync(R.d_name_key.p, R.name_key.data(), 2 * n * 4, hipMemcpyHostToDevice, stage_stream_));
		}
		stream_wait(stage_stream_); // the batch is resident; everything after this is the hot path
	}
	void activate_batch() override { cur_ = 1 - cur_; }
	int current_set() const override { return cur_; }
	void bind_lane(int lane, int set) override { lanes_.at(lane)->set = set; }
	bool stages_beside_mapping() const override { return true; }

	// One sub-batch of reads through seeding and chaining.  The steps are private members below, in this order; what they share travels in SeedCall.
	void seed_chain(const SeedChainParams &P, long lo, long hi, int lane_id, int n_threads, std::vector<ReadChains> &out) override
	{
		HIP_CHECK(hipSetDevice(dev_)); // HIP's current device is per thread, and the mapper drives every lane from a thread of its own
		Lane &ln = *lanes_.at(lane_id);
		out.clear();
		out.resize((size_t)(hi - lo));
		if (out.empty()) return;
		SeedCall c(P, ln, res_[ln.set], kernel_profiler(lane_id, replica_), lo, hi, lane_id, n_threads);
		double tt = Trace::now();
		const SeedChainBuffers Bu = encode_sketch(c);
		// -T: drop minimizers in low-complexity regions.  MM2AMD_DEVICE_SDUST=1: the regions come from sdust_kernel on the encoded reads, on this stream; otherwise from the host threads
		const bool dev_sdust = P.sdust_thres > 0 && env_on("MM2AMD_DEVICE_SDUST"), sdust_no_narrow = sdust_env_no_narrow();
		if (dev_sdust) dust_on_device(c, Bu, sdust_no_narrow);
		else if (P.sdust_thres > 0) dust_on_host(c);
		collect_seeds(c);
		stream_wait(c.st);
		if (dev_sdust) account_sdust(c, sdust_no_narrow);
		Trace::get().add(lane_id, "gpu:sketch+collect", tt, Trace::now()); tt = Trace::now();
		size_anchors(c);
		const bool prune = decide_prune(c);
		ln.d_sort_list.ensure(c.n + 1);
		const SortClasses cls = list_sort_classes(ln.h_sort_list, ln.d_sort_list.p, c.n, [&](size_t i) { return (uint64_t)ln.h_na.p[i]; }, c.st);
		const bool dump_full = prune && P.chain_dump && chain_dump_path(); // diagnostics: the chain dump's IN block is the read's WHOLE sorted list (the reference's seed list)
		expand_sort(c, cls, dump_full);
		if (getenv("MM2AMD_TIE_COUNT")) report_tie_count(c, cls);
		if (const char *dump = getenv("MM2AMD_SEED_DUMP")) write_seed_dump(c, dump, *fi_names_);
		const char *cdump = P.chain_dump ? chain_dump_path() : nullptr; // diagnostics: every read's chains (chain_dump.hpp)
		if (P.anchors_only) { hand_over_anchors(c, cdump, tt, out); return; } // the caller chains (RMQ)
		chain_backtrack(c, prune);
		const bool lazy = P.lazy_chains != 0; // the chains stay on the device for align_regions()
		ln.rg_lazy = lazy;
		queue_first_pass(c, prune, lazy);
		stream_wait(c.st);
		Trace::get().add(lane_id, "gpu:expand..backtrack", tt, Trace::now()); tt = Trace::now();
		if (prune) account_pruning(c);
		queue_pass_chains(ln.pass1, ln.d_bt_out_a.p, ln.d_bt_out_u.p, !lazy, c.st);
		const uint32_t *tie = P.rmq ? ln.pass1.tie.p : nullptr; // the reads the RMQ kernel left to the host
		const std::vector<std::pair<size_t, size_t>> redo = queue_handbacks(c, tie, lazy);
		stream_wait(c.st);
		if (cdump) dump_first_pass(c, cdump, cls, prune, dump_full, lazy, tie);
		Trace::get().add(lane_id, "d2h:chains", tt, Trace::now());
		c.kp.collect();
		TraceScope ts(lane_id, "host:chains->vectors");
		assemble_chains(c, lazy, redo, out);
		if (P.long_join && !c.R.has_pairs && !getenv("MM2AMD_LONG_JOIN_ON_HOST")) long_join(c, lazy, cdump, out); // (the diagnostic switch: every re-chain through rmq_chain.cpp)
	}

private:
	// ---- seed_chain's steps
	// Encode + sketch.  Returns the unit view of the lane's buffers: what the two kernels (and sdust_kernel) run over; without pairs a unit is a fragment
	SeedChainBuffers encode_sketch(SeedCall &c)
	{
		Lane &ln = c.ln;
		SeedChainBuffers &B = c.B;
		const Resident &R = c.R;
		B = SeedChainBuffers();
		B.n_reads = (int)c.n, B.seq_off = R.d_seq_off.p + c.lo, B.ascii = R.h_ascii.p, B.qpool = R.d_qpool.p; // (pinned host memory, device-visible)
		if (R.have_read_names) B.name_lb = R.d_name_key.p + c.lo, B.name_eq = R.d_name_key.p + R.seq_off.size() - 1 + c.lo;
		SeedChainBuffers Bu = B;
		if (R.has_pairs) Bu.n_reads = (int)c.n_unit, Bu.seq_off = R.d_unit_off.p + c.ulo;
		c.kp.begin(c.st); launch_encode(Bu, c.st); c.kp.end(c.st, "encode_kernel", 3 * c.L);
		// minimizers, written from slot seq_off[r] of the minimizer arrays (at most one per base)
		const uint64_t base0 = c.base0, cap_mz = c.cap_mz;
		ln.d_mz_cnt.ensure(c.n_unit);
		ln.d_mz_x.ensure(cap_mz + 1), ln.d_mz_y.ensure(cap_mz + 1);
		ln.d_sd_n.ensure(cap_mz + 1), ln.d_sd_off.ensure(cap_mz + 1), ln.d_sd_aoff.ensure(cap_mz + 1), ln.d_sd_qpos.ensure(cap_mz + 1), ln.d_sd_info.ensure(cap_mz + 1);
		// the per-read slot offsets are the batch-wide base offsets; shifting the array bases by the sub-batch's first offset makes them local
		B.mz_cnt = ln.d_mz_cnt.p, B.mz_off = B.seq_off, B.mz_x = ln.d_mz_x.p - base0, B.mz_y = ln.d_mz_y.p - base0;
		B.sd_n = ln.d_sd_n.p - base0, B.sd_off = ln.d_sd_off.p - base0, B.sd_aoff = ln.d_sd_aoff.p - base0, B.sd_qpos = ln.d_sd_qpos.p - base0, B.sd_info = ln.d_sd_info.p - base0;
		Bu.mz_cnt = B.mz_cnt, Bu.mz_off = Bu.seq_off, Bu.mz_x = B.mz_x, Bu.mz_y = B.mz_y;
		int max_len = 0; // sizes the sketch kernel's LDS tile
		for (size_t u = 0; u < c.n_unit; ++u) {
			const uint64_t l_u = R.has_pairs ? R.unit_off[c.ulo + u + 1] - R.unit_off[c.ulo + u] : R.seq_off[c.lo + u + 1] - R.seq_off[c.lo + u];
			max_len = (int)std::max<uint64_t>((uint64_t)max_len, l_u);
		}
		c.kp.begin(c.st); launch_sketch(Bu, c.P, max_len, c.st); c.kp.end(c.st, "sketch_kernel", c.L + 16.0 * c.est_mz);
		if (R.has_pairs) // seed_collect joins the minimizer lists of a pair's two units (collect_minimizers, map.c:59-72); indices are batch-wide
			B.unit_first = R.d_unit_first.p + c.lo, B.unit_off = R.d_unit_off.p, B.unit_cnt = ln.d_mz_cnt.p - c.ulo, B.mz_cnt = nullptr;
		return Bu;
	}
	// Dust, on the device: sdust_kernel's two launch classes (sdust.hpp) leave the regions in the seed arrays, which are still unused; dust_filter_kernel drops
	// the minimizers inside them.  The counters' copy is read after the caller's wait (account_sdust).
	void dust_on_device(SeedCall &c, const SeedChainBuffers &Bu, bool no_narrow)
	{
		Lane &ln = c.ln;
		const SeedChainBuffers &B = c.B;
		ln.d_sdust_list.ensure(c.n_unit), ln.d_sdust_cnt.ensure(1);
		HIP_CHECK(hipMemsetAsync(ln.d_sdust_cnt.p, 0, sizeof(SdustCounters), c.st));
		SdustParams S;
		S.codes = B.qpool, S.off = Bu.seq_off, S.code_mul = 2, S.n_reads = (int)c.n_unit, S.T = c.P.sdust_thres < kSdustMaxT ? c.P.sdust_thres : kSdustMaxT;
		S.reg_n = B.sd_n, S.reg_s = B.sd_off, S.reg_e = B.sd_aoff, S.wide_list = ln.d_sdust_list.p, S.cnt = ln.d_sdust_cnt.p;
		if (no_narrow) sdust_run_class(S, 2, 0, c.kp, 0.0, c.st);
		else {
			sdust_run_class(S, 0, 0, c.kp, 0.0, c.st);
			sdust_run_class(S, 1, 0, c.kp, 0.0, c.st); // the reads that stopped: the launch reads the list's length on the device
		}
		HIP_CHECK(hipMemcpyAsync(ln.h_sdust_cnt.ensure(1), ln.d_sdust_cnt.p, sizeof(SdustCounters), hipMemcpyDeviceToHost, c.st));
		c.kp.begin(c.st); launch_dust_filter(B, c.st); c.kp.end(c.st, "dust_filter_kernel", 16.0 * c.est_mz);
	}
	// bases each sdust class scanned: a read that stopped counts up to there for the narrow class and whole for the wide one
	void account_sdust(SeedCall &c, bool no_narrow)
	{
		const SdustCounters &cnt = *c.ln.h_sdust_cnt.p;
		if (cnt.err) throw HipError("[mm2amd] sdust_kernel: a list of perfect intervals outgrew the wide capacity");
		c.kp.add_units("sdust_kernel[wide]", (double)cnt.wide_bases);
		if (!no_narrow) c.kp.add_units("sdust_kernel[narrow]", c.L - (double)cnt.wide_bases + (double)cnt.narrow_partial);
	}
	// Dust, on the host: sdust_scan (sdust_core.hpp) per unit on the host threads while the sketch kernel runs, the regions go up, then dust_filter_kernel
	void dust_on_host(SeedCall &c)
	{
		Lane &ln = c.ln;
		const Resident &R = c.R;
		const uint64_t base0 = c.base0, cap_mz = c.cap_mz;
		const int T = c.P.sdust_thres;
		uint32_t *h_n = ln.h_dust_n.ensure(cap_mz + 1), *h_s = ln.h_dust_s.ensure(cap_mz + 1), *h_e = ln.h_dust_e.ensure(cap_mz + 1);
		const char *asc = R.h_ascii.p;
		parallel_for(c.n_threads, (long)c.n_unit, [&](long u, int) {
			const uint64_t o = R.has_pairs ? R.unit_off[c.ulo + u] : R.seq_off[c.lo + u];
			const int len = (int)((R.has_pairs ? R.unit_off[c.ulo + u + 1] : R.seq_off[c.lo + u + 1]) - o);
			thread_local std::vector<SdustState::Perf> perf(SdustState::PCAP);
			thread_local std::vector<uint8_t> codes;
			codes.resize((size_t)len + 1);
			for (int j = 0; j < len; ++j) codes[j] = kNt4Table[(uint8_t)asc[o + j]];
			SdustState S;
			S.P = perf.data();
			uint32_t k = 0;
			sdust_scan(codes.data(), len, T, S, [&](int s0, int e0) { h_s[o - base0 + k] = (uint32_t)s0, h_e[o - base0 + k] = (uint32_t)e0; ++k; });
			if (len > 0) h_n[o - base0] = k;
		}, 16);
		HIP_CHECK(hipMemcpyAsync(ln.d_sd_n.p, h_n, cap_mz * 4, hipMemcpyHostToDevice, c.st));
		HIP_CHECK(hipMemcpyAsync(ln.d_sd_off.p, h_s, cap_mz * 4, hipMemcpyHostToDevice, c.st));
		HIP_CHECK(hipMemcpyAsync(ln.d_sd_aoff.p, h_e, cap_mz * 4, hipMemcpyHostToDevice, c.st));
		c.kp.begin(c.st); launch_dust_filter(c.B, c.st); c.kp.end(c.st, "dust_filter_kernel", 16.0 * c.est_mz);
	}
	// Seeds: probe, filter, count anchors.  The per-read counts' copies (ln.h_na, h_nmp, h_rep) are queued; the caller waits
	void collect_seeds(SeedCall &c)
	{
		Lane &ln = c.ln;
		SeedChainBuffers &B = c.B;
		const size_t n = c.n;
		ln.d_n_anchor.ensure(n), ln.d_n_minipos.ensure(n), ln.d_n_seedhit.ensure(n), ln.d_rep_len.ensure(n);
		B.n_anchor = ln.d_n_anchor.p, B.n_minipos = ln.d_n_minipos.p, B.n_seedhit = ln.d_n_seedhit.p, B.rep_len = ln.d_rep_len.p;
		c.kp.begin(c.st); launch_seed_collect(B, I_, c.P, c.st); c.kp.end(c.st, "seed_collect_kernel", 36.0 * c.est_mz); // per minimizer: 16 B record + 8 key + 8 val + 4 flags
		HIP_CHECK(hipMemcpyAsync(ln.h_na.ensure(n), ln.d_n_anchor.p, n * 4, hipMemcpyDeviceToHost, c.st));
		HIP_CHECK(hipMemcpyAsync(ln.h_nmp.ensure(n), ln.d_n_minipos.p, n * 4, hipMemcpyDeviceToHost, c.st));
		HIP_CHECK(hipMemcpyAsync(ln.h_rep.ensure(n), ln.d_rep_len.p, n * 4, hipMemcpyDeviceToHost, c.st));
	}
	// Counts -> ln.a_off / ln.mp_off (queued to the device) and c.n_a / c.n_mp; everything that is sized by them, wired into the lane's buffers
	void size_anchors(SeedCall &c)
	{
		Lane &ln = c.ln;
		SeedChainBuffers &B = c.B;
		const size_t n = c.n;
		std::vector<uint64_t> &a_off = ln.a_off, &mp_off = ln.mp_off;
		a_off.resize(n + 1), mp_off.resize(n + 1);
		a_off[0] = mp_off[0] = 0;
		for (size_t i = 0; i < n; ++i) a_off[i + 1] = a_off[i] + ln.h_na.p[i], mp_off[i + 1] = mp_off[i] + ln.h_nmp.p[i];
		const uint64_t n_a = c.n_a = a_off[n], n_mp = c.n_mp = mp_off[n];
		uint64_t *h_off = ln.h_off.ensure(2 * (n + 1));
		memcpy(h_off, a_off.data(), (n + 1) * 8), memcpy(h_off + n + 1, mp_off.data(), (n + 1) * 8);
		ln.d_a_off.ensure(n + 1), ln.d_mp_off.ensure(n + 1);
		HIP_CHECK(hipMemcpyAsync(ln.d_a_off.p, h_off, (n + 1) * 8, hipMemcpyHostToDevice, c.st));
		HIP_CHECK(hipMemcpyAsync(ln.d_mp_off.p, h_off + n + 1, (n + 1) * 8, hipMemcpyHostToDevice, c.st));
		ln.d_anchors.ensure(n_a + 1), ln.d_minipos.ensure(n_mp + 1), ln.d_f.ensure(n_a + 1), ln.d_p.ensure(n_a + 1), ln.d_t.ensure(n_a + 1);
		ln.d_skey_in.ensure(n_a + 1), ln.d_sval_in.ensure(n_a + 1), ln.d_skey_out.ensure(n_a + 1), ln.d_sval_out.ensure(n_a + 1), ln.d_tie.ensure(2 * n + 1);
		B.sort_key_in = ln.d_skey_in.p, B.sort_val_in = ln.d_sval_in.p, B.sort_key_out = ln.d_skey_out.p, B.sort_val_out = ln.d_sval_out.p, B.tie_flag = ln.d_tie.p;
		B.tie_list = ln.d_tie.p + n, B.tie_count = ln.d_tie.p + 2 * n;
		B.rid_bits = rid_bits_;
		B.a_off = ln.d_a_off.p, B.mp_off = ln.d_mp_off.p, B.anchors = ln.d_anchors.p, B.mini_pos = ln.d_minipos.p;
		B.f = ln.d_f.p, B.p = ln.d_p.p, B.t = ln.d_t.p;
	}
	// Where most reads give up -- accurate reads against a small reference: nearly every anchor is at the true locus and survives -- the filter pass is wasted:
	// after a sub-batch that redid more than half of its reads the next 15 go unpruned, then one tries again.  (Not with the tests' knobs, which force give-ups.)
	static bool prune_adapt() { static const bool on = !getenv("MM2AMD_PRUNE_BINS") && !getenv("MM2AMD_PRUNE_CAP"); return on; }
	// The pruning decision.  Anchors with no other anchor of their strand and target inside the chaining window go before the sort (seed_chain.hip: anchor_sort_prune_kernel)
	// where that is exact: mg_lchain_dp's fill (not the RMQ chainer, not a caller that wants every sorted anchor), one segment per read, every span = k (no HPC)
	// below min_chain_score (an isolated anchor is no chain end), the radix sort's order (not the heap merge's), and no seed dump, which is the reference's
	// full list.  MM2AMD_ANCHOR_PRUNE=0: the A/B switch.  MM2AMD_PRUNE_BINS / MM2AMD_PRUNE_CAP (tests): a smaller presence table / survivor capacity.
	bool decide_prune(SeedCall &c)
	{
		const SeedChainParams &P = c.P;
		static const bool prune_env = !(getenv("MM2AMD_ANCHOR_PRUNE") && atoi(getenv("MM2AMD_ANCHOR_PRUNE")) == 0);
		const bool adapt = prune_adapt();
		const bool prune_can = prune_env && !P.rmq && !P.anchors_only && !c.R.has_pairs && !P.is_hpc && P.k < P.min_chain_score && !(P.flag & ref::F_HEAP_SORT) && !getenv("MM2AMD_SEED_DUMP");
		const bool prune = prune_can && !(adapt && prune_rest_.load() > 0 && prune_rest_.fetch_sub(1) > 0);
		if (prune) {
			const size_t n = c.n;
			c.ln.d_nkept.ensure(2 * n + 8); // the kept counts, the classes' redo counters (8 words), the classes' redo lists
			c.B.n_kept = c.ln.d_nkept.p, c.B.redo_count = c.ln.d_nkept.p + n, c.B.redo_list = c.ln.d_nkept.p + n + 8;
			static const int bins_env = getenv("MM2AMD_PRUNE_BINS") ? atoi(getenv("MM2AMD_PRUNE_BINS")) : 0, cap_env = getenv("MM2AMD_PRUNE_CAP") ? atoi(getenv("MM2AMD_PRUNE_CAP")) : 0;
			c.B.prune_bins = bins_env, c.B.prune_cap = cap_env;
		}
		return prune;
	}
	// The anchor sort's work list for a launch of n reads with count(i) anchors each: the reads that have anchors, class by class, filled into h_list and queued to d_list
	template <class Count>
	SortClasses list_sort_classes(PinBuf<uint32_t> &h_list, uint32_t *d_list, size_t n, Count count, hipStream_t st) const
	{
		SortClasses s;
		for (size_t i = 0; i < n; ++i) if (const uint64_t a = count(i)) { const int k = anchor_sort_class(a, rid_bits_); ++s.n_class[k], s.a_class[k] += (double)a; }
		for (int k = 0; k < kAnchorSortClasses; ++k) s.class_first[k + 1] = s.class_first[k] + s.n_class[k];
		uint32_t *h = h_list.ensure(n + 1);
		int fill[kAnchorSortClasses];
		for (int k = 0; k < kAnchorSortClasses; ++k) fill[k] = s.class_first[k];
		for (size_t i = 0; i < n; ++i) if (const uint64_t a = count(i)) h[fill[anchor_sort_class(a, rid_bits_)]++] = (uint32_t)i;
		if (s.n_listed()) HIP_CHECK(hipMemcpyAsync(d_list, h, (size_t)s.n_listed() * 4, hipMemcpyHostToDevice, st));
		return s;
	}
	// Anchors: expand, then the per-read sort.  dump_full: sorted unpruned into a buffer of its own first, for the chain dump's IN blocks
	void expand_sort(SeedCall &c, const SortClasses &cls, bool dump_full)
	{
		Lane &ln = c.ln;
		c.kp.begin(c.st); launch_seed_expand(c.B, I_, c.P, c.st); c.kp.end(c.st, "seed_expand_kernel", 24.0 * c.n_a);
		if (dump_full) {
			SeedChainBuffers Bd = c.B;
			Bd.anchors = ln.d_dump_anchors.ensure(c.n_a + 1), Bd.n_kept = nullptr, Bd.redo_list = Bd.redo_count = nullptr;
			launch_anchor_sort(Bd, I_, c.P, ln.d_sort_list.p, cls.n_class, cls.a_class, c.st, nullptr);
		}
		launch_anchor_sort(c.B, I_, c.P, ln.d_sort_list.p, cls.n_class, cls.a_class, c.st, &c.kp);
	}
	// The anchors-only hand-over: the caller chains, so the sorted anchors travel as they are (in pass1.a; no first pass follows)
	void hand_over_anchors(SeedCall &c, const char *cdump, double tt, std::vector<ReadChains> &out)
	{
		Lane &ln = c.ln;
		const std::vector<uint64_t> &a_off = ln.a_off, &mp_off = ln.mp_off;
		Anchor *ha = ln.pass1.a.ensure(c.n_a + 1);
		uint64_t *hmp = ln.h_minipos.ensure(c.n_mp + 1);
		if (c.n_a) HIP_CHECK(hipMemcpyAsync(ha, ln.d_anchors.p, c.n_a * sizeof(Anchor), hipMemcpyDeviceToHost, c.st));
		if (c.n_mp) HIP_CHECK(hipMemcpyAsync(hmp, ln.d_minipos.p, c.n_mp * 8, hipMemcpyDeviceToHost, c.st));
		stream_wait(c.st);
		Trace::get().add(c.lane_id, "gpu:expand+sort, d2h:anchors", tt, Trace::now());
		c.kp.collect();
		if (cdump) dump_anchors_only(c, cdump, ha);
		const int32_t *h_rep = ln.h_rep.p;
		parallel_for(c.n_threads, (long)c.n, [&](long i, int) {
			ReadChains &r = out[i];
			r.rep_len = h_rep[i];
			r.mp_p = hmp + mp_off[i], r.n_mp = (int32_t)(mp_off[i + 1] - mp_off[i]);
			r.u_p = nullptr, r.n_u = 0, r.chained = false;
			r.a_p = ha + a_off[i], r.n_a = (int64_t)(a_off[i + 1] - a_off[i]);
		}, 64);
	}
	// Fill (mg_lchain_dp) or RMQ, then the backtrack: it compacts the chains on the device, so that only the chained anchors travel to the host
	void chain_backtrack(SeedCall &c, bool prune)
	{
		Lane &ln = c.ln;
		SeedChainBuffers &B = c.B;
		const SeedChainParams &P = c.P;
		const size_t n = c.n;
		const uint64_t n_a = c.n_a;
		make_pieces(B, ln, ln.h_pieces, n, [&](size_t i) { return (uint64_t)ln.h_na.p[i]; }, P.rmq ? rmq_piece_len() : fill_piece_len(), c.st);
		if (P.rmq) { c.kp.begin(c.st); launch_chain_rmq(B, P, c.st); c.kp.end(c.st, "chain_rmq_kernel", 32.0 * n_a); }
		else { c.kp.begin(c.st); launch_chain_fill(B, P, c.st); c.kp.end(c.st, "chain_fill_kernel", prune ? 0.0 : 24.0 * n_a); } // (pruned: per kept anchor, added by account_pruning)
		B.pieces = nullptr, B.n_pieces = 0;
		ln.d_bt_cursor.ensure(2), ln.d_bt_out_a.ensure(n_a + 1), ln.d_bt_out_u.ensure((P.min_cnt >= 2 ? n_a / 2 : n_a) + n + 1); // a chain has at least max(1, min_cnt) anchors (lchain.c:66)
		ln.d_bt_nu.ensure(n), ln.d_bt_nv.ensure(n), ln.d_bt_aoff.ensure(n), ln.d_bt_uoff.ensure(n);
		B.bt_cursor = ln.d_bt_cursor.p, B.bt_out_a = ln.d_bt_out_a.p, B.bt_out_u = ln.d_bt_out_u.p;
		B.bt_nu = ln.d_bt_nu.p, B.bt_nv = ln.d_bt_nv.p, B.bt_aoff = ln.d_bt_aoff.p, B.bt_uoff = ln.d_bt_uoff.p;
		c.kp.begin(c.st); launch_chain_backtrack(B, P, c.st); c.kp.end(c.st, "chain_backtrack_kernel", prune ? 0.0 : 8.0 * n_a);
	}

	// ---- the download of a chaining pass, in two stages around the caller's wait.  Both routines queue only: the caller adds its own copies before it waits.
	// Stage one: the backtrack's cursors and per-read counts and offsets for the n reads of the pass, and (with_tie) the reads the RMQ kernel handed back.  Both passes
	// leave them in the same device arrays (see Lane).
	static void queue_pass_counts(Lane &ln, ChainPassHost &H, size_t n, bool with_tie, hipStream_t st)
	{
		HIP_CHECK(hipMemcpyAsync(H.cursor.ensure(2), ln.d_bt_cursor.p, 16, hipMemcpyDeviceToHost, st));
		HIP_CHECK(hipMemcpyAsync(H.nu.ensure(n), ln.d_bt_nu.p, n * 4, hipMemcpyDeviceToHost, st));
		HIP_CHECK(hipMemcpyAsync(H.nv.ensure(n), ln.d_bt_nv.p, n * 4, hipMemcpyDeviceToHost, st));
		HIP_CHECK(hipMemcpyAsync(H.aoff.ensure(n), ln.d_bt_aoff.p, n * 8, hipMemcpyDeviceToHost, st));
		HIP_CHECK(hipMemcpyAsync(H.uoff.ensure(n), ln.d_bt_uoff.p, n * 8, hipMemcpyDeviceToHost, st));
		if (with_tie) HIP_CHECK(hipMemcpyAsync(H.tie.ensure(n), ln.d_tie.p, n * 4, hipMemcpyDeviceToHost, st));
	}
	// Stage two, once the cursors have landed: the chains, and the chained anchors unless they stay on the device
	static void queue_pass_chains(ChainPassHost &H, const Anchor *d_a, const uint64_t *d_u, bool with_anchors, hipStream_t st)
	{
		const uint64_t n_v = H.n_v(), n_u = H.n_u();
		Anchor *ha = H.a.ensure(n_v + 1);
		uint64_t *hu = H.u.ensure(n_u + 1);
		if (n_v && with_anchors) HIP_CHECK(hipMemcpyAsync(ha, d_a, n_v * sizeof(Anchor), hipMemcpyDeviceToHost, st));
		if (n_u) HIP_CHECK(hipMemcpyAsync(hu, d_u, n_u * 8, hipMemcpyDeviceToHost, st));
	}
	// What the first pass queues before the wait: its counts, the kept counts of a pruned launch, and the first chains' ends (lazy: of the anchors only what the
	// long-join question needs comes back) or the minimizer positions
	void queue_first_pass(SeedCall &c, bool prune, bool lazy)
	{
		Lane &ln = c.ln;
		const size_t n = c.n;
		queue_pass_counts(ln, ln.pass1, n, c.P.rmq != 0, c.st);
		uint64_t *hmp = ln.h_minipos.ensure(c.n_mp + 1);
		// the kept counts and the redo counters; the redo lists only for the dump's KP lines
		if (prune) HIP_CHECK(hipMemcpyAsync(ln.h_nkept.ensure(2 * n + 8), ln.d_nkept.p, ((c.P.chain_dump && chain_dump_path() ? 2 * n : n) + 8) * 4, hipMemcpyDeviceToHost, c.st));
		if (lazy) {
			ln.d_span.ensure(2 * n);
			int32_t *h_span = ln.h_span.ensure(2 * n);
			launch_first_chain_span((int)n, ln.d_bt_out_a.p, ln.d_bt_out_u.p, ln.d_bt_aoff.p, ln.d_bt_uoff.p, ln.d_bt_nu.p, ln.d_span.p, c.st);
			HIP_CHECK(hipMemcpyAsync(h_span, ln.d_span.p, 2 * n * 4, hipMemcpyDeviceToHost, c.st));
		} else if (c.n_mp) HIP_CHECK(hipMemcpyAsync(hmp, ln.d_minipos.p, c.n_mp * 8, hipMemcpyDeviceToHost, c.st));
	}
	// What the pruning did: the process-wide counters, the adaptive pause, and the bytes the three kernels moved for the anchors they were given
	void account_pruning(SeedCall &c)
	{
		const size_t n = c.n;
		const uint32_t *h_na = c.ln.h_na.p, *h_nkept = c.ln.h_nkept.p;
		double kept_class[kAnchorSortClasses] = { 0 }, kept = 0;
		unsigned long long n_redone = 0;
		for (int k = 0; k + 1 < kAnchorSortClasses; ++k) n_redone += h_nkept[n + k];
		for (size_t i = 0; i < n; ++i) if (h_na[i]) kept_class[anchor_sort_class(h_na[i], rid_bits_)] += h_nkept[i], kept += h_nkept[i];
		size_t n_sorted = 0;
		for (size_t i = 0; i < n; ++i) n_sorted += h_na[i] != 0;
		if (prune_adapt() && n_redone * 2 > n_sorted) prune_rest_.store(15);
		prune_counters().n_in += c.n_a, prune_counters().n_kept += (unsigned long long)kept, prune_counters().n_redo += n_redone;
		for (int k = 0; k + 1 < kAnchorSortClasses; ++k) if (kept_class[k] > 0) c.kp.add_bytes(kAnchorSortNames[k], 24.0 * kept_class[k]);
		c.kp.add_bytes("chain_fill_kernel", 24.0 * kept), c.kp.add_bytes("chain_backtrack_kernel", 8.0 * kept);
	}
	// The RMQ hand-backs: reads the RMQ kernel left to the host (a tie in a range minimum, an over-full neighbourhood, a whole contig).  Their sorted anchors
	// travel as they are, into ln.h_redo; the mapper chains them with rmq_chain.cpp.  Returns (read, offset into h_redo) pairs; the copies are queued only.
	std::vector<std::pair<size_t, size_t>> queue_handbacks(SeedCall &c, const uint32_t *tie, bool lazy)
	{
		Lane &ln = c.ln;
		const std::vector<uint64_t> &a_off = ln.a_off, &mp_off = ln.mp_off;
		std::vector<std::pair<size_t, size_t>> redo;
		size_t redo_total = 0;
		if (tie) for (size_t i = 0; i < c.n; ++i) if (tie[i]) redo.emplace_back(i, redo_total), redo_total += (size_t)(a_off[i + 1] - a_off[i]);
		Anchor *h_redo = redo_total ? ln.h_redo.ensure(redo_total + 1) : nullptr;
		for (const auto &rd : redo) {
			const size_t cnt = (size_t)(a_off[rd.first + 1] - a_off[rd.first]);
			if (cnt) HIP_CHECK(hipMemcpyAsync(h_redo + rd.second, ln.d_anchors.p + a_off[rd.first], cnt * sizeof(Anchor), hipMemcpyDeviceToHost, c.st));
			// with the chains left on the device the minimizer positions stay there too -- but a handed-back read is chained and finished by the
			// host path, whose mm_est_err walks them: its slice comes along
			const size_t n_pos = (size_t)(mp_off[rd.first + 1] - mp_off[rd.first]);
			if (lazy && n_pos) HIP_CHECK(hipMemcpyAsync(ln.h_minipos.p + mp_off[rd.first], ln.d_minipos.p + mp_off[rd.first], n_pos * 8, hipMemcpyDeviceToHost, c.st));
		}
		return redo;
	}
	// chains -> ReadChains: views into the lane's pinned buffers, and where the chains are on the device (align_regions)
	void assemble_chains(SeedCall &c, bool lazy, const std::vector<std::pair<size_t, size_t>> &redo, std::vector<ReadChains> &out)
	{
		Lane &ln = c.ln;
		const std::vector<uint64_t> &a_off = ln.a_off, &mp_off = ln.mp_off;
		const uint64_t *hmp = ln.h_minipos.p;
		const int32_t *h_rep = ln.h_rep.p;
		parallel_for(c.n_threads, (long)c.n, [&](long i, int) {
			ReadChains &r = out[i];
			r.rep_len = h_rep[i];
			r.mp_p = lazy ? nullptr : hmp + mp_off[i], r.n_mp = (int32_t)(mp_off[i + 1] - mp_off[i]);
			set_chains(r, ln.pass1, (size_t)i, lazy, 0);
			r.chained = true;
		}, 64);
		ln.rg_lo = c.lo, ln.rg_n = c.n, ln.rg_n_v = ln.pass1.n_v(), ln.rg_n_u = ln.pass1.n_u(), ln.rg_n_v2 = ln.rg_n_u2 = 0;
		for (const auto &rd : redo) {
			ReadChains &r = out[rd.first];
			r.u_p = nullptr, r.n_u = 0, r.chained = false, r.dev_src = -1;
			r.mp_p = hmp + mp_off[rd.first];
			r.a_p = ln.h_redo.p + rd.second, r.n_a = (int64_t)(a_off[rd.first + 1] - a_off[rd.first]);
		}
	}

	// The chaining kernels give a wavefront to a read.  A read with far more anchors than the others (it crosses a multi-copy element of the reference) makes the whole
	// launch wait for its wavefront, so when a read has more than `len` anchors the launch gets a work list instead: every read's ceil(anchors / len) pieces (seed_chain.hip:
	// chain_piece_bounds moves the cuts to cluster heads, where the sequential rules restart), the reads with several pieces first.  Launches without such a read
	// keep the plain read-per-wavefront grid; the benchmark's reads, ~7 k anchors each against a cut at 4 096, do get lists.  The list is made from the counts BEFORE
	// pruning (the kept counts never come to the host in time): a piece that starts beyond a read's kept anchors returns at once.  MM2AMD_CHAIN_PIECE / MM2AMD_RMQ_PIECE: the piece lengths (tests set small ones; 0 = never cut).
	static int fill_piece_len() { const char *e = getenv("MM2AMD_CHAIN_PIECE"); return e ? atoi(e) : 4096; }
	static int rmq_piece_len() { const char *e = getenv("MM2AMD_RMQ_PIECE"); return e ? atoi(e) : 512; }
	template <class Count>
	static void make_pieces(SeedChainBuffers &B, Lane &ln, PinBuf<uint32_t> &hbuf, size_t n, Count count, int len, hipStream_t st)
	{
		B.pieces = nullptr, B.n_pieces = 0, B.piece_len = len;
		{ const char *e = getenv("MM2AMD_RMQ_RANK_MAX"); B.rmq_rank_max = e ? std::min(256, std::max(0, atoi(e))) : 256; }
		{ const char *e = getenv("MM2AMD_RMQ_DENSE"); B.piece_dense = e ? atoi(e) : 1024; } // (the RMQ kernel's long clusters go to workgroups: seed_chain.hip chain_rmq_wide_kernel; tests set it low, 0 = off)
		if (len <= 0) return;
		size_t n_p = 0;
		bool any = false;
		for (size_t i = 0; i < n; ++i) { const uint64_t c = count(i); n_p += (size_t)((c + len - 1) / len); any |= c > (uint64_t)len; }
		if (!any || n_p > (size_t)INT32_MAX) return;
		uint32_t *h = hbuf.ensure(2 * n_p);
		size_t k = 0;
		for (int pass = 0; pass < 2; ++pass) // reads with several pieces first: their wavefronts start with the launch
			for (size_t i = 0; i < n; ++i) {
				const uint64_t c = count(i), m = (c + len - 1) / len;
				if (m == 0 || (m > 1) != (pass == 0)) continue;
				for (uint64_t q = 0; q < m; ++q) h[2 * k] = (uint32_t)i, h[2 * k + 1] = (uint32_t)q, ++k;
			}
		ln.d_pieces.ensure(2 * n_p);
		HIP_CHECK(hipMemcpyAsync(ln.d_pieces.p, h, 2 * n_p * 4, hipMemcpyHostToDevice, st));
		B.pieces = ln.d_pieces.p, B.n_pieces = (int)n_p;
		if (getenv("MM2AMD_PIECE_DEBUG")) fprintf(stderr, "[mm2amd] chaining work list: %zu reads in %zu pieces of %d anchors\n", n, n_p, len);
	}

	// ---- long-join: map.c:283-292 on the device.  Which reads re-chain is decided from the first chains (long_join_reads); their CHAINED anchors -- still in
	// the backtrack's device output -- go through the per-read sort, chain_rmq_kernel with bw_long, and the backtrack again (rechain).  A read the RMQ kernel
	// hands back (a range minimum that is not unique, an over-full neighbourhood) keeps its first chains and long_join_done unset: the caller re-chains it with rmq_chain.cpp.
	void long_join(SeedCall &c, bool lazy, const char *cdump, std::vector<ReadChains> &out)
	{
		Lane &ln = c.ln;
		const std::vector<uint32_t> sel = long_join_reads(c, lazy, out);
		const size_t n2 = sel.size();
		if (n2 == 0) return;
		rechain(c, sel);
		ChainPassHost &H = ln.pass2;
		queue_pass_counts(ln, H, n2, true, c.st);
		stream_wait(c.st);
		queue_pass_chains(H, ln.d_lj_out_a.p, ln.d_lj_out_u.p, !lazy, c.st);
		ln.rg_n_v2 = H.n_v(), ln.rg_n_u2 = H.n_u();
		stream_wait(c.st);
		c.kp.collect();
		if (cdump) dump_long_join(c, cdump, sel, lazy);
		for (size_t k = 0; k < n2; ++k) {
			ReadChains &r = out[sel[k]];
			if (H.tie.p[k]) { r.long_join_done = false; continue; } // the host's tie-exact tree does this one
			set_chains(r, H, k, lazy, 1);
			r.long_joined = true;
		}
	}
	// The reference's two conditions on a read's first chain; marks the question settled for every chained read.  lazy: the chained anchors stayed on the device
	// and the first chain's ends came back on their own (ln.h_span)
	std::vector<uint32_t> long_join_reads(const SeedCall &c, bool lazy, std::vector<ReadChains> &out) const
	{
		const ChainPassHost &H = c.ln.pass1;
		const int32_t *h_span = c.ln.h_span.p;
		std::vector<uint32_t> sel;
		for (size_t i = 0; i < c.n; ++i) {
			ReadChains &r = out[i];
			if (!r.chained) continue; // (an RMQ preset's hand-back: the caller chains it first and asks the question itself)
			r.long_join_done = true;
			if (H.nu.p[i] <= 1) continue;
			const int qlen = c.qlen(i);
			const Anchor *a = H.a.p + H.aoff.p[i];
			const int32_t a0 = lazy ? h_span[2 * i] : (int32_t)a[0].y, a1 = lazy ? h_span[2 * i + 1] : (int32_t)a[(uint64_t)((int32_t)H.u.p[H.uoff.p[i]] - 1)].y;
			if (qlen - (a1 - a0) > c.P.rmq_rescue_size || a1 - a0 > qlen * c.P.rmq_rescue_ratio) sel.push_back((uint32_t)i);
		}
		return sel;
	}
	// The re-chain of the reads `sel` as a batch of its own, through the second backtrack; what it reuses of the first pass's device buffers: see Lane
	void rechain(SeedCall &c, const std::vector<uint32_t> &sel)
	{
		Lane &ln = c.ln;
		hipStream_t st = c.st;
		const size_t n2 = sel.size();
		const int32_t *h_nv = ln.pass1.nv.p;
		uint64_t *h_off = ln.h_lj_off.ensure(2 * (n2 + 1));
		uint64_t *h_src = h_off + n2 + 1;
		h_off[0] = 0;
		for (size_t k = 0; k < n2; ++k) h_off[k + 1] = h_off[k] + (uint64_t)h_nv[sel[k]], h_src[k] = ln.pass1.aoff.p[sel[k]];
		const uint64_t n_a2 = h_off[n2];
		SeedChainBuffers B2 = ln.B;
		B2.n_reads = (int)n2, B2.seq_off = nullptr, B2.mz_cnt = nullptr, B2.unit_first = nullptr;
		B2.n_kept = nullptr, B2.redo_list = B2.redo_count = nullptr; // (the re-chain takes every chained anchor)
		ln.d_lj_src.ensure(n2 + 1), ln.d_lj_out_a.ensure(n_a2 + 1);
		HIP_CHECK(hipMemcpyAsync(ln.d_a_off.p, h_off, (n2 + 1) * 8, hipMemcpyHostToDevice, st));
		HIP_CHECK(hipMemcpyAsync(ln.d_lj_src.p, h_src, n2 * 8, hipMemcpyHostToDevice, st));
		B2.a_off = ln.d_a_off.p;
		const auto count = [&](size_t k) { return (uint64_t)h_nv[sel[k]]; }; // (never 0: a re-chained read has two chains or more)
		const SortClasses cls = list_sort_classes(ln.h_lj_list, ln.d_sort_list.p, n2, count, st);
		c.kp.begin(st); launch_rechain_gather(B2, ln.d_bt_out_a.p, ln.d_lj_src.p, st); c.kp.end(st, "rechain_gather_kernel", 32.0 * n_a2);
		SeedChainParams P2 = c.P;
		P2.rmq = 1, P2.bw = c.P.bw_long, P2.flag &= ~(int64_t)ref::F_HEAP_SORT; // (the heap-merge order belongs to the seeding; this sort is radix_sort_128x)
		launch_anchor_sort(B2, I_, P2, ln.d_sort_list.p, cls.n_class, cls.a_class, st, &c.kp);
		make_pieces(B2, ln, ln.h_lj_pieces, n2, count, rmq_piece_len(), st);
		c.kp.begin(st); launch_chain_rmq(B2, P2, st); c.kp.end(st, "chain_rmq_kernel[long-join]", 32.0 * n_a2);
		ln.d_lj_out_u.ensure((P2.min_cnt >= 2 ? n_a2 / 2 : n_a2) + n2 + 1);
		B2.bt_out_a = ln.d_lj_out_a.p, B2.bt_out_u = ln.d_lj_out_u.p; // (the first pass's chains stay for align_regions; counts and offsets reuse its arrays)
		c.kp.begin(st); launch_chain_backtrack(B2, P2, st); c.kp.end(st, "chain_backtrack_kernel[long-join]", 8.0 * n_a2);
	}

public:

	void ksw(const std::vector<KswJob> &jobs, const KswScoring &sc, int lane_id, int n_threads, std::vector<KswRes> &res, const uint32_t **cigar) override
	{
		HIP_CHECK(hipSetDevice(dev_)); // HIP's current device is per thread, and the mapper drives every lane from a thread of its own
		Lane &ln = *lanes_.at(lane_id);
		res.resize(jobs.size());
		size_t n_cig = 0;
		ksw_setup(ln, n_threads);
		const uint8_t *d_tbytes = nullptr;
		if (sc.n_tbytes) { // composed targets (mm_align_sr_rna): a small byte pool per call
			ln.d_tbytes.ensure(sc.n_tbytes + 1);
			HIP_CHECK(hipMemcpyAsync(ln.d_tbytes.p, sc.tbytes, sc.n_tbytes, hipMemcpyHostToDevice, ln.stream));
			d_tbytes = ln.d_tbytes.p;
		}
		ln.ksw.run(jobs, res_[ln.set].d_qpool.p, d_tbytes, T_->S.p, sc, res.data(), cigar, &n_cig, ln.stream);
		kernel_profiler(lane_id, replica_).collect();
	}

	void fetch_chains(int lane_id, const std::vector<long> &reads, std::vector<ReadChains> &chains) override
	{
		if (reads.empty()) return;
		HIP_CHECK(hipSetDevice(dev_));
		Lane &ln = *lanes_.at(lane_id);
		hipStream_t st = ln.stream;
		RgnGather *g = ln.h_gather.ensure(reads.size());
		uint64_t na = 0, nmp = 0;
		for (size_t k = 0; k < reads.size(); ++k) {
			const ReadChains &c = chains[reads[k]];
			RgnGather &G = g[k];
			G.a_src = c.dev_a_off, G.a_dst = na, G.mp_src = ln.mp_off[reads[k]], G.mp_dst = nmp;
			G.n_a = (int32_t)c.n_a, G.n_mp = c.n_mp, G.src = c.dev_src == 1 ? 1u : 0u, G.pad = 0;
			na += (uint64_t)c.n_a, nmp += (uint64_t)c.n_mp;
		}
		ln.d_gather.ensure(reads.size()), ln.d_fetch_a.ensure(na + 1), ln.d_fetch_mp.ensure(nmp + 1);
		Anchor *ha = ln.h_fetch_a.ensure(na + 1);
		uint64_t *hmp = ln.h_fetch_mp.ensure(nmp + 1);
		HIP_CHECK(hipMemcpyAsync(ln.d_gather.p, g, reads.size() * sizeof(RgnGather), hipMemcpyHostToDevice, st));
		launch_gather_chains((int)reads.size(), ln.d_gather.p, ln.d_bt_out_a.p, ln.d_lj_out_a.p, ln.d_minipos.p, ln.d_fetch_a.p, ln.d_fetch_mp.p, st);
		if (na) HIP_CHECK(hipMemcpyAsync(ha, ln.d_fetch_a.p, na * sizeof(Anchor), hipMemcpyDeviceToHost, st));
		if (nmp) HIP_CHECK(hipMemcpyAsync(hmp, ln.d_fetch_mp.p, nmp * 8, hipMemcpyDeviceToHost, st));
		stream_wait(st);
		for (size_t k = 0; k < reads.size(); ++k) {
			ReadChains &c = chains[reads[k]];
			c.a_p = ha + g[k].a_dst, c.mp_p = hmp + g[k].mp_dst;
		}
	}

	// region_dev.hpp: chains -> hits -> windows -> DP -> consume -> finish on the device, for the reads of this lane's last seed_chain()
	bool aligns_regions() const override
	{
		const char *e = getenv("MM2AMD_DEVICE_REGIONS"); // =0: the host's chains -> hits, window planning and consumption (A/B checks)
		return !(e && *e == '0');
	}
	void align_regions(int lane_id, const RgnOpts &O, const KswScoring &sc, bool log_gap, const std::vector<ReadChains> &chains, const std::vector<RegionReadIn> &in, int n_threads,
	                   RegionBatchOut &out) override
	{
		HIP_CHECK(hipSetDevice(dev_));
		Lane &ln = *lanes_.at(lane_id);
		hipStream_t st = ln.stream;
		const Resident &R = res_[ln.set];
		const size_t n = ln.rg_n;
		out = RegionBatchOut();
		if (n == 0 || chains.size() < n || in.size() < n) return;
		upload_ref_layout_once(st);
		KernelProfiler &kp = kernel_profiler(lane_id, replica_);
		double tt = Trace::now();
		const RgnSizes Z = describe_reads(ln, R, chains, in);
		RgnBuffers B = wire_regions(ln, R, Z, st);
		kp.begin(st); launch_chain_regs(B, O, st); kp.end(st, "chain_regs_kernel", 32.0 * (double)Z.sq + 80.0 * (double)Z.n_chain);
		kp.begin(st); launch_region_plan(B, O, st); kp.end(st, "region_plan_kernel", 16.0 * (double)Z.sq);
		unsigned int *cur = ln.h_rg_cur.ensure(RGN_CUR_N);
		HIP_CHECK(hipMemcpyAsync(cur, ln.d_rg_cur.p, RGN_CUR_N * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
		stream_wait(st);
		const uint32_t n_regs = std::min<uint32_t>(cur[RGN_CUR_REGS], Z.max_regs);
		const size_t n_jobs = std::min<size_t>(cur[RGN_CUR_JOBS], (size_t)Z.max_jobs);
		Trace::get().add(lane_id, "gpu:regs+plan", tt, Trace::now());
		const uint32_t *d_cigar = n_jobs ? run_region_dp(ln, R, sc, n_jobs, n_threads, out) : nullptr;
		tt = Trace::now();
		B.res = ln.ksw.d_res.p, B.perm = ln.ksw.d_perm.p;
		kp.begin(st); launch_region_consume(B, O, d_cigar, st); kp.end(st, "region_consume_kernel", 68.0 * (double)n_jobs);
		HIP_CHECK(hipMemcpyAsync(cur, ln.d_rg_cur.p, RGN_CUR_N * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
		stream_wait(st);
		const size_t out_words = cur[RGN_CUR_OUT];
		ln.d_rg_out.ensure(out_words + 1);
		if (n_regs && cur[RGN_CUR_N_FIN]) {
			finish_run(ln.d_rg_fin.p, (int)n_regs, ln.d_rg_pieces.p, d_cigar, ln.d_rg_out.p, ln.d_rg_finres.p, R.d_qpool.p, T_->S.p, sc.mat, sc.q, sc.e, log_gap, cur[RGN_CUR_MAX_OPS], st, &kp,
			           (double)out_words * 8.0 + (double)cur[RGN_CUR_N_FIN] * (sizeof(FinRegion) + sizeof(FinResult)), (double)cur[RGN_CUR_N_FIN]);
			if (O.flag & ref::F_EQX) out.eqx = eqx_pass(ln, ln.eqx_rg, kp, ln.d_rg_fin.p, n_regs, ln.d_rg_finres.p, ln.d_rg_out.p, out_words, R.d_qpool.p);
		}
		queue_region_results(ln, n * (size_t)Z.stride, n_regs, out_words, out);
		stream_wait(st);
		Trace::get().add(lane_id, "gpu:consume+finish, d2h:hits", tt, Trace::now());
		eqx_sequence_bytes(kp, out.eqx, out.fin, out.fin_res, n_regs);
		kp.collect();
		out.n_regs = n_regs, out.n_jobs = n_jobs, out.rout_stride = Z.stride;
	}

private:
	// ---- align_regions' steps
	// what a sub-batch's chains come to: anchors in the per-segment slices, chains, the most chains of one read; the bounds they put on hits and DP jobs
	struct RgnSizes { uint64_t sq = 0, n_chain = 0, max_jobs = 0; uint32_t max_regs = 0; int max_nu = 1, stride = 1; };
	// once: the reference sequences' offsets and lengths (the flag is set after the copies have landed)
	void upload_ref_layout_once(hipStream_t st)
	{
		if (ref_ready_.load(std::memory_order_acquire)) return;
		std::lock_guard<std::mutex> lk(ref_mu_);
		if (ref_ready_.load(std::memory_order_relaxed)) return;
		d_ref_off_.ensure(fi_seq_off_->size() + 1), d_ref_len2_.ensure(fi_seq_len_->size() + 1);
		HIP_CHECK(hipMemcpyAsync(d_ref_off_.p, fi_seq_off_->data(), fi_seq_off_->size() * 8, hipMemcpyHostToDevice, st));
		HIP_CHECK(hipMemcpyAsync(d_ref_len2_.p, fi_seq_len_->data(), fi_seq_len_->size() * 4, hipMemcpyHostToDevice, st));
		stream_wait(st);
		ref_ready_.store(true, std::memory_order_release);
	}
	// The reads of the lane's last seed_chain() in device terms (ln.h_rg_reads), made from what the host knows anyway
	static RgnSizes describe_reads(Lane &ln, const Resident &R, const std::vector<ReadChains> &chains, const std::vector<RegionReadIn> &in)
	{
		const size_t n = ln.rg_n;
		RgnRead *hr = ln.h_rg_reads.ensure(n);
		RgnSizes Z;
		Z.stride = R.has_pairs ? 2 : 1; // two-segment fragments: their chains are cut per segment on the device (chain_regs_kernel), a segment is a read of its own from there on
		for (size_t i = 0; i < n; ++i) {
			const ReadChains &c = chains[i];
			RgnRead &r = hr[i];
			const bool skip = in[i].skip || c.dev_src < 0 || !c.chained;
			r.a_off = c.dev_a_off, r.u_off = c.dev_u_off, r.sq_off = Z.sq, r.mp_off = ln.mp_off[i];
			r.qpool_fwd = 2 * R.seq_off[ln.rg_lo + i];
			r.n_u = skip ? 0 : c.n_u, r.n_a = skip ? 0 : (int32_t)c.n_a, r.n_mp = (int32_t)(ln.mp_off[i + 1] - ln.mp_off[i]);
			r.qlen = (int32_t)(R.seq_off[ln.rg_lo + i + 1] - R.seq_off[ln.rg_lo + i]);
			r.qlen2 = 0, r.gap_ref = in[i].gap_ref;
			if (R.has_pairs) {
				const int32_t u0 = R.unit_first[ln.rg_lo + i];
				if (R.unit_first[ln.rg_lo + i + 1] - u0 == 2) r.qlen = (int32_t)(R.unit_off[u0 + 1] - R.unit_off[u0]), r.qlen2 = (int32_t)(R.unit_off[u0 + 2] - R.unit_off[u0 + 1]);
			}
			r.hash = in[i].hash, r.src = skip ? RGN_SRC_SKIP : (c.dev_src == 1 ? RGN_SRC_LJ : 0);
			if (!skip) {
				const uint64_t k = r.qlen2 > 0 ? 2 : 1; // (a chain can have anchors on both segments: each segment's slice is as long as the fragment's chained anchors)
				Z.sq += k * (uint64_t)c.n_a, Z.n_chain += k * (uint64_t)c.n_u, Z.max_nu = std::max(Z.max_nu, (int)c.n_u);
			}
		}
		if (Z.n_chain >= (1ull << 31)) throw std::runtime_error("[mm2amd] align_regions: a sub-batch with more than 2^31 chains");
		Z.max_regs = (uint32_t)Z.n_chain;
		Z.max_jobs = std::max<uint64_t>(Z.sq + 2 * Z.n_chain + 1, 3 * Z.n_chain + 1); // (one window per anchor at most, two extensions; short reads: three pieces per hit)
		if (Z.max_jobs >= (1ull << 31)) throw std::runtime_error("[mm2amd] align_regions: a sub-batch with more than 2^31 anchors");
		return Z;
	}
	// The hit / window / piece arrays sized and wired; the reads go up and the cursors are cleared (queued)
	RgnBuffers wire_regions(Lane &ln, const Resident &R, const RgnSizes &Z, hipStream_t st) const
	{
		const size_t n = ln.rg_n;
		RgnBuffers B{};
		B.n_reads = (int)n;
		B.rout_stride = Z.stride;
		ln.d_rg_reads.ensure(n), ln.d_rg_rout.ensure(n * (size_t)Z.stride), ln.d_rg_cur.ensure(RGN_CUR_N);
		ln.d_rg_sq.ensure(Z.sq + 1), ln.d_rg_sites.ensure(Z.sq + 1);
		ln.d_rg_regs.ensure(Z.max_regs + 1), ln.d_rg_aux.ensure(Z.max_regs + 1), ln.d_rg_plan.ensure(Z.max_regs + 1), ln.d_rg_fin.ensure(Z.max_regs + 1), ln.d_rg_finres.ensure(Z.max_regs + 1);
		ln.d_rg_win.ensure(Z.max_jobs), ln.d_rg_jobs.ensure(Z.max_jobs), ln.d_rg_pieces.ensure(Z.max_jobs);
		HIP_CHECK(hipMemcpyAsync(ln.d_rg_reads.p, ln.h_rg_reads.p, n * sizeof(RgnRead), hipMemcpyHostToDevice, st));
		HIP_CHECK(hipMemsetAsync(ln.d_rg_cur.p, 0, RGN_CUR_N * sizeof(unsigned int), st));
		B.reads = ln.d_rg_reads.p;
		B.a_src[0] = ln.d_bt_out_a.p, B.a_src[1] = ln.d_lj_out_a.p, B.u_src[0] = ln.d_bt_out_u.p, B.u_src[1] = ln.d_lj_out_u.p;
		B.mini_pos = ln.d_minipos.p, B.sq_a = ln.d_rg_sq.p, B.regs = ln.d_rg_regs.p, B.aux = ln.d_rg_aux.p, B.rout = ln.d_rg_rout.p, B.cursors = ln.d_rg_cur.p;
		B.ref_len = d_ref_len2_.p, B.ref_off = d_ref_off_.p, B.max_regs = Z.max_regs;
		B.qpool = R.d_qpool.p, B.S = T_->S.p;
		B.lds_chains = std::min(256, (Z.max_nu + 63) / 64 * 64);
		B.plan = ln.d_rg_plan.p, B.win = ln.d_rg_win.p, B.jobs = ln.d_rg_jobs.p, B.gap_sites = ln.d_rg_sites.p, B.max_jobs = (uint32_t)Z.max_jobs;
		B.fin = ln.d_rg_fin.p, B.pieces = ln.d_rg_pieces.p;
		return B;
	}
	// The DP: the job records stay where region_plan_kernel wrote them; launch classes, order and sizes are made on the device (ksw_order.hip).  Returns the
	// device's CIGAR pool; adds the cells to out.dp_cells
	const uint32_t *run_region_dp(Lane &ln, const Resident &R, const KswScoring &sc, size_t n_jobs, int n_threads, RegionBatchOut &out)
	{
		hipStream_t st = ln.stream;
		const uint32_t *d_cigar = nullptr;
		size_t n_cig = 0;
		ksw_setup(ln, n_threads);
		static const bool host_order = getenv("MM2AMD_KSW_ORDER_ON_HOST") != nullptr; // A/B checks: the job records cross for the host's ordering
		if (host_order) {
			KswJob *hj = ln.h_rg_jobs.ensure(n_jobs);
			HIP_CHECK(hipMemcpyAsync(hj, ln.d_rg_jobs.p, n_jobs * sizeof(KswJob), hipMemcpyDeviceToHost, st));
			stream_wait(st);
			for (size_t j = 0; j < n_jobs; ++j) out.dp_cells += (double)hj[j].qlen * hj[j].tlen;
			ln.ksw.run_jobs(hj, n_jobs, R.d_qpool.p, nullptr, T_->S.p, sc, nullptr, &d_cigar, &n_cig, st);
		} else {
			{
				DpGate gate(*this); // at most MM2AMD_DP_GATE lanes (default 4) in their DP launches at once
				ln.ksw.run_jobs(nullptr, n_jobs, R.d_qpool.p, nullptr, T_->S.p, sc, nullptr, &d_cigar, &n_cig, st, ln.d_rg_jobs.p);
			}
			out.dp_cells += ln.ksw.last_cells;
		}
		return d_cigar;
	}
	// The results' host copies, queued; `out` views them once the caller has waited.  n_rout: per-read (per-segment) records
	static void queue_region_results(Lane &ln, size_t n_rout, uint32_t n_regs, size_t out_words, RegionBatchOut &out)
	{
		hipStream_t st = ln.stream;
		RgnReadOut *h_rout = ln.h_rg_rout.ensure(n_rout);
		ref::Reg1 *h_regs = ln.h_rg_regs.ensure(n_regs + 1);
		RgnAux *h_aux = ln.h_rg_aux.ensure(n_regs + 1);
		RgnPlan *h_plan = ln.h_rg_plan.ensure(n_regs + 1);
		FinRegion *h_fin = ln.h_rg_fin.ensure(n_regs + 1);
		FinResult *h_finres = ln.h_rg_finres.ensure(n_regs + 1);
		uint32_t *h_out = ln.h_rg_out.ensure(out_words + 1);
		HIP_CHECK(hipMemcpyAsync(h_rout, ln.d_rg_rout.p, n_rout * sizeof(RgnReadOut), hipMemcpyDeviceToHost, st));
		if (n_regs) {
			HIP_CHECK(hipMemcpyAsync(h_regs, ln.d_rg_regs.p, n_regs * sizeof(ref::Reg1), hipMemcpyDeviceToHost, st));
			HIP_CHECK(hipMemcpyAsync(h_aux, ln.d_rg_aux.p, n_regs * sizeof(RgnAux), hipMemcpyDeviceToHost, st));
			HIP_CHECK(hipMemcpyAsync(h_plan, ln.d_rg_plan.p, n_regs * sizeof(RgnPlan), hipMemcpyDeviceToHost, st));
			HIP_CHECK(hipMemcpyAsync(h_fin, ln.d_rg_fin.p, n_regs * sizeof(FinRegion), hipMemcpyDeviceToHost, st));
			HIP_CHECK(hipMemcpyAsync(h_finres, ln.d_rg_finres.p, n_regs * sizeof(FinResult), hipMemcpyDeviceToHost, st));
		}
		if (out_words) HIP_CHECK(hipMemcpyAsync(h_out, ln.d_rg_out.p, out_words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
		out.reads = h_rout, out.regs = h_regs, out.aux = h_aux, out.plan = h_plan, out.fin = h_fin, out.fin_res = h_finres, out.cigars = h_out;
	}

public:

	bool supports_long_join() const override { return true; }
	bool eqx_regions() const override
	{
		const char *e = getenv("MM2AMD_DEVICE_EQX"); // =0: --eqx reads take the host's rounds and the host's mm_update_cigar_eqx, as before cigar_eqx_kernel (A/B checks)
		return !(e && *e == '0');
	}
	// MM_F_EQX (cigar_eqx.hpp) for regions region_finish_kernel has just finished on the lane's stream: count, place (the host waits for the counts: the
	// pool is sized from their sum), write.  The copy of the pool is queued; the caller waits for the stream.
	EqxOut eqx_pass(Lane &ln, EqxBufs &B, KernelProfiler &kp, const FinRegion *d_regions, size_t n, const FinResult *d_res, const uint32_t *d_fin_pool, size_t fin_words, const uint8_t *d_qpool)
	{
		EqxParams P{};
		P.regions = d_regions, P.n_regions = (int)n, P.results = d_res, P.fin_pool = d_fin_pool, P.qpool = d_qpool, P.S = T_->S.p;
		const double rec_bytes = (double)n * (sizeof(FinRegion) + sizeof(FinResult) + 4); // (the sequences' share: eqx_sequence_bytes)
		const uint64_t total = eqx_count(B, P, kp, (double)fin_words * 4.0 + rec_bytes, ln.stream, stream_wait);
		return eqx_write(B, P, total, kp, ((double)fin_words + (double)total) * 4.0 + rec_bytes + (double)n * 8.0, ln.stream);
	}
	// the columns the two passes read, known once the regions' records are on the host: a query byte and half a byte of packed reference per
	// column, in both passes; a region relabelled in place is not read again by the writing pass
	void eqx_sequence_bytes(KernelProfiler &kp, const EqxOut &x, const FinRegion *regions, const FinResult *res, size_t n)
	{
		if (!x.n_ops || !KernelProfiler::enabled_flag()) return;
		double cnt = 0, wr = 0;
		for (size_t i = 0; i < n; ++i) {
			if (res[i].n_cigar <= 0) continue;
			const double b = (double)regions[i].q_len + 0.5 * (double)regions[i].t_len;
			cnt += b;
			if (x.n_ops[i] != (uint32_t)res[i].n_cigar) wr += 2.0 * b;
		}
		kp.add_bytes("cigar_eqx_kernel[count]", cnt), kp.add_bytes("cigar_eqx_kernel[write]", wr);
	}
	bool finishes_regions() const override
	{
		// On unless MM2AMD_DEVICE_FINISH=0 (the host's mm_update_extra: A/B checks); read at every call.  region_finish_kernel costs 18 ms of latency-bound launches
		// per 1-Gbase step and takes 1.5 host core-seconds per step off the host (5.5 -> 3.9): at 16 threads for one GPU the pipeline's rate is the same either
		// way, with fewer it is higher -- and a rank of a multi-GPU job that shares the node's CPU quota with seven others (two threads each under a 16-CPU
		// quota) is bounded by exactly those core-seconds.
		const char *e = getenv("MM2AMD_DEVICE_FINISH");
		if (e && *e) return *e != '0';
		return true;
	}
	void finish_regions(int lane_id, const std::vector<FinRegion> &regions, const std::vector<FinPiece> &pieces, size_t out_words, const int8_t *mat25, int q, int e, bool log_gap,
	                    std::vector<FinResult> &results, const uint32_t **cigars, EqxOut *eqx) override
	{
		HIP_CHECK(hipSetDevice(dev_));
		Lane &ln = *lanes_.at(lane_id);
		const size_t n = regions.size();
		results.resize(n);
		*cigars = nullptr;
		if (n == 0) return;
		memcpy(ln.h_fin_regions.ensure(n), regions.data(), n * sizeof(FinRegion));
		memcpy(ln.h_fin_pieces.ensure(pieces.size() + 1), pieces.data(), pieces.size() * sizeof(FinPiece));
		ln.d_fin_regions.ensure(n), ln.d_fin_pieces.ensure(pieces.size() + 1), ln.d_fin_out.ensure(out_words + 1), ln.d_fin_res.ensure(n);
		ln.h_fin_out.ensure(out_words + 1), ln.h_fin_res.ensure(n);
		HIP_CHECK(hipMemcpyAsync(ln.d_fin_regions.p, ln.h_fin_regions.p, n * sizeof(FinRegion), hipMemcpyHostToDevice, ln.stream));
		HIP_CHECK(hipMemcpyAsync(ln.d_fin_pieces.p, ln.h_fin_pieces.p, pieces.size() * sizeof(FinPiece), hipMemcpyHostToDevice, ln.stream));
		uint32_t longest = 1; // (a region's room in the output pool is the sum of its pieces: the next region's offset minus its own)
		for (size_t i = 0; i < n; ++i) longest = std::max<uint32_t>(longest, (uint32_t)((i + 1 < n ? regions[i + 1].out_off : (uint32_t)out_words) - regions[i].out_off));
		KernelProfiler &prof = kernel_profiler(lane_id, replica_);
		finish_run(ln.d_fin_regions.p, (int)n, ln.d_fin_pieces.p, ln.ksw.d_cigar.p, ln.d_fin_out.p, ln.d_fin_res.p, res_[ln.set].d_qpool.p, T_->S.p, mat25, (int8_t)q, (int8_t)e, log_gap, longest,
		           ln.stream, &prof, (double)out_words * 8.0 + (double)n * (sizeof(FinRegion) + sizeof(FinResult)), (double)n);
		if (eqx) *eqx = eqx_pass(ln, ln.eqx_fin, prof, ln.d_fin_regions.p, n, ln.d_fin_res.p, ln.d_fin_out.p, out_words, res_[ln.set].d_qpool.p);
		HIP_CHECK(hipMemcpyAsync(ln.h_fin_res.p, ln.d_fin_res.p, n * sizeof(FinResult), hipMemcpyDeviceToHost, ln.stream));
		HIP_CHECK(hipMemcpyAsync(ln.h_fin_out.p, ln.d_fin_out.p, out_words * sizeof(uint32_t), hipMemcpyDeviceToHost, ln.stream));
		stream_wait(ln.stream);
		memcpy(results.data(), ln.h_fin_res.p, n * sizeof(FinResult));
		*cigars = ln.h_fin_out.p;
		if (eqx) eqx_sequence_bytes(prof, *eqx, regions.data(), results.data(), n);
		static const bool check = getenv("MM2AMD_FIN_CHECK") != nullptr; // diagnostic: every returned CIGAR must cover its windows
		if (check) fin_check(lane_id, regions, results, ln.h_fin_out.p);
		prof.collect();
	}

	// ---- mm_pair on the device (pair.hpp) for the lane's sub-batch: the lane's stream and buffers, the lane's profiler slot
	bool pair_begin(int lane_id, size_t n_frag, size_t n_hits, PairTables &t) override
	{
		HIP_CHECK(hipSetDevice(dev_));
		Lane &ln = *lanes_.at(lane_id);
		t.frag = ln.h_pe_frag.ensure(n_frag + 1), t.hits = ln.h_pe_hits.ensure(n_hits + 1), t.out = ln.h_pe_out.ensure(n_hits + 1), t.res = ln.h_pe_res.ensure(n_frag + 1);
		return true;
	}
	void pair_run(int lane_id, size_t n_frag, const mm2amd_pe_opt_t &opt, int n_threads) override
	{
		HIP_CHECK(hipSetDevice(dev_));
		Lane &ln = *lanes_.at(lane_id);
		mm2amd::pair_run(ln.pair, (int)n_frag, ln.h_pe_frag.p, ln.h_pe_hits.p, opt, ln.h_pe_out.p, ln.h_pe_res.p, n_threads, kernel_profiler(lane_id, replica_), ln.stream, stream_wait);
	}

	// ---- the output stage on the device (rec_text.hpp).  Its stream, buffers and profiler slot are its own; of the backend it reads the device's ordinal, the
	// packed sequence's address and the index's name table, none of which changes after construction -- so it runs beside the lanes' mapping.
	bool writes_records() const override { return true; }
	RecTextBufs rec_text_begin(const RecTextSizes &sz) override
	{
		HIP_CHECK(hipSetDevice(dev_));
		RecText &R = rt_;
		if (!R.stream) HIP_CHECK(hipStreamCreateWithFlags(&R.stream, hipStreamNonBlocking));
		if (!R.targets_ready) { // target names and lengths: once per context, when the first batch is formatted here
			const size_t n_seq = fi_seq_len_->size();
			uint64_t tot = 0;
			for (size_t i = 0; i < n_seq; ++i) tot += (*fi_names_)[i].size();
			char *nm = R.h_tnames.ensure(tot + 1);
			uint64_t *to = R.h_tname_off.ensure(n_seq + 1);
			uint32_t *tl = R.h_tlen.ensure(n_seq + 1);
			tot = 0;
			for (size_t i = 0; i < n_seq; ++i) {
				to[i] = tot, tl[i] = (*fi_seq_len_)[i];
				memcpy(nm + tot, (*fi_names_)[i].data(), (*fi_names_)[i].size());
				tot += (*fi_names_)[i].size();
			}
			to[n_seq] = tot;
			R.d_tnames.ensure(tot + 1), R.d_tname_off.ensure(n_seq + 1), R.d_tlen.ensure(n_seq + 1);
			if (tot) HIP_CHECK(hipMemcpyAsync(R.d_tnames.p, nm, tot, hipMemcpyHostToDevice, R.stream));
			HIP_CHECK(hipMemcpyAsync(R.d_tname_off.p, to, (n_seq + 1) * 8, hipMemcpyHostToDevice, R.stream));
			if (n_seq) HIP_CHECK(hipMemcpyAsync(R.d_tlen.p, tl, n_seq * 4, hipMemcpyHostToDevice, R.stream));
			stream_wait(R.stream);
			R.targets_ready = true;
		}
		R.sz = sz;
		RecTextBufs b;
		b.jobs = R.h_jobs.ensure(sz.n_jobs + 1), b.hits = R.h_hits.ensure(sz.n_hits + 1), b.names = R.h_names.ensure(sz.name_bytes + 1);
		b.q = R.h_q.ensure(sz.q_bytes + 1), b.cigar = R.h_cigar.ensure(sz.cigar_words + 1), b.off = R.h_off.ensure(sz.n_jobs + 1);
		R.h_res.ensure(sz.n_jobs + 1);
		return b;
	}
	const RecRes *rec_text_size(int64_t flag) override { return text_size(flag, false); }
	const char *rec_text_write(uint64_t total) override { return text_write(total, false); }
	const RecRes *junc_text_size(int64_t flag) override { return text_size(flag, true); }
	const char *junc_text_write(uint64_t total) override { return text_write(total, true); }

private:
	// What a lane's KswRunner needs before a run: the caller's threads, the lane's profiler slot, and the lane's share of the HBM the lanes may spend on
	// direction matrices (1 B per DP cell, one slot per persistent wave: the big per-lane allocation; splice gap fills have matrices of tens of MB each, and
	// 288 GB of HBM is what lets thousands of them be in flight).  MM2AMD_DIR_BUDGET_GB: the budget, read at every call
	void ksw_setup(Lane &ln, int n_threads)
	{
		ln.ksw.n_threads = n_threads, ln.ksw.prof = &kernel_profiler(ln.id, replica_), ln.ksw.lane = ln.id;
		size_t dir_gb = 160;
		if (const char *e = getenv("MM2AMD_DIR_BUDGET_GB")) dir_gb = atol(e) > 0 ? (size_t)atol(e) : dir_gb;
		ln.ksw.dir_budget = std::min<size_t>((dir_gb << 30) / (size_t)active_lanes_, (size_t)96 << 30); // scratch only grows: keep one lane's share bounded
	}
	// the two passes of rec_text_kernel, or (junc) of junc_text_kernel, over the tables of rec_text_begin
	const RecRes *text_size(int64_t flag, bool junc)
	{
		HIP_CHECK(hipSetDevice(dev_));
		RecText &R = rt_;
		const RecTextSizes &sz = R.sz;
		if (sz.n_jobs == 0) return R.h_res.p;
		R.d_jobs.ensure(sz.n_jobs), R.d_hits.ensure(sz.n_hits + 1), R.d_names.ensure(sz.name_bytes + 1), R.d_q.ensure(sz.q_bytes + 1), R.d_cigar.ensure(sz.cigar_words + 1);
		R.d_res.ensure(sz.n_jobs), R.d_off.ensure(sz.n_jobs);
		HIP_CHECK(hipMemcpyAsync(R.d_jobs.p, R.h_jobs.p, sz.n_jobs * sizeof(RecJob), hipMemcpyHostToDevice, R.stream));
		if (sz.n_hits) HIP_CHECK(hipMemcpyAsync(R.d_hits.p, R.h_hits.p, sz.n_hits * sizeof(RecHit), hipMemcpyHostToDevice, R.stream));
		if (sz.name_bytes) HIP_CHECK(hipMemcpyAsync(R.d_names.p, R.h_names.p, sz.name_bytes, hipMemcpyHostToDevice, R.stream));
		if (sz.q_bytes) HIP_CHECK(hipMemcpyAsync(R.d_q.p, R.h_q.p, sz.q_bytes, hipMemcpyHostToDevice, R.stream));
		if (sz.cigar_words) HIP_CHECK(hipMemcpyAsync(R.d_cigar.p, R.h_cigar.p, sz.cigar_words * 4, hipMemcpyHostToDevice, R.stream));
		RecParams &P = R.P;
		P.jobs = R.d_jobs.p, P.n_jobs = (int)sz.n_jobs, P.hits = R.d_hits.p, P.flag = flag, P.names = R.d_names.p, P.qpool = R.d_q.p, P.S = T_->S.p, P.cigar = R.d_cigar.p;
		P.tnames = R.d_tnames.p, P.tname_off = R.d_tname_off.p, P.tlen = R.d_tlen.p, P.res = R.d_res.p, P.off = nullptr, P.out = nullptr;
		KernelProfiler &prof = kernel_profiler(kMaxProfLanes - 1, replica_);
		text_size_pass(P, junc ? junc_text_launch : rec_text_launch, R.h_res.p, prof, junc ? "junc_text_kernel[size]" : "rec_text_kernel[size]", (double)sz.cigar_words * 4.0 + (double)sz.q_bytes,
		          (double)sz.n_jobs, R.stream, stream_wait);
		prof.collect();
		return R.h_res.p;
	}
	const char *text_write(uint64_t total, bool junc)
	{
		HIP_CHECK(hipSetDevice(dev_));
		RecText &R = rt_;
		const RecTextSizes &sz = R.sz;
		R.h_out.ensure(total + 1);
		if (sz.n_jobs == 0 || total == 0) return R.h_out.p;
		R.d_out.ensure(total + 8);
		KernelProfiler &prof = kernel_profiler(kMaxProfLanes - 1, replica_);
		text_write_pass(R.P, junc ? junc_text_launch : rec_text_launch, R.h_off.p, R.d_off.p, R.d_out.p, R.h_out.p, total, prof, junc ? "junc_text_kernel[write]" : "rec_text_kernel[write]",
		           (double)total + (double)sz.cigar_words * 4.0 + (double)sz.q_bytes, (double)sz.n_jobs, R.stream, stream_wait);
		prof.collect();
		return R.h_out.p;
	}

	struct RecText {
		hipStream_t stream = nullptr;
		bool targets_ready = false;
		RecTextSizes sz;
		RecParams P{};
		PinBuf<char> h_tnames; PinBuf<uint64_t> h_tname_off; PinBuf<uint32_t> h_tlen;
		DevBuf<char> d_tnames; DevBuf<uint64_t> d_tname_off; DevBuf<uint32_t> d_tlen;
		PinBuf<RecJob> h_jobs; PinBuf<RecHit> h_hits; PinBuf<char> h_names; PinBuf<uint8_t> h_q; PinBuf<uint32_t> h_cigar; PinBuf<uint64_t> h_off; PinBuf<RecRes> h_res; PinBuf<char> h_out;
		DevBuf<RecJob> d_jobs; DevBuf<RecHit> d_hits; DevBuf<char> d_names; DevBuf<uint8_t> d_q; DevBuf<uint32_t> d_cigar; DevBuf<uint64_t> d_off; DevBuf<RecRes> d_res; DevBuf<char> d_out;
		~RecText() { if (stream) (void)hipStreamDestroy(stream); }
	};
	RecText rt_;
	// At most dp_gate_ lanes between the ordering of their DP batch and its last kernel (0: no limit).  The DP kernels are VALU-bound persistent launches: eight that
	// coincide share the SIMDs round-robin and ALL finish late; admitted four at a time the first ones finish early and their lanes go on to consume, finish and the next
	// sub-batch's seeding while the others compute.  Measured (calls 23-24, 8-step runs in one call each): no gate 2.24-2.28 Gbases/s with 47-52 ms per streaming
	// launch, four lanes 2.30 / 2.30 with 29-34 ms, two lanes 2.22-2.28 with 18-21 ms, one lane 2.08.  (Round 2's stage gates serialised ALL GPU stages of the lanes
	// and lost 7-18 %; this one leaves seeding, chaining and the region kernels free to run beside the DP.)
	struct DpGate {
		HipBackend &b;
		explicit DpGate(HipBackend &be) : b(be) { if (b.dp_gate_ > 0) { std::unique_lock<std::mutex> lk(b.gate_mu_); b.gate_cv_.wait(lk, [&] { return b.gate_in_ < b.dp_gate_; }); ++b.gate_in_; } }
		~DpGate() { if (b.dp_gate_ > 0) { { std::lock_guard<std::mutex> lk(b.gate_mu_); --b.gate_in_; } b.gate_cv_.notify_one(); } }
	};
	int dp_gate_ = getenv("MM2AMD_DP_GATE") ? atoi(getenv("MM2AMD_DP_GATE")) : 4, gate_in_ = 0;
	std::mutex gate_mu_;
	std::condition_variable gate_cv_;
	hipStream_t stream_ = nullptr;
	int n_threads_ = 1, n_cu_ = 256, n_lanes_ = 1, rid_bits_ = 1, dev_ = 0, replica_ = 0;
	std::atomic<int> active_lanes_{1};
	std::atomic<int> prune_rest_{0}; // sub-batches that still go unpruned because a recent one sent most of its reads to the unpruned sort anyway (seed_chain)
	DevIndex I_{};
	DeviceIndexTables own_;
	DeviceIndexTables *T_ = nullptr;
	std::vector<std::unique_ptr<Lane>> lanes_;
	// The resident batch (backend_lane.hpp).  Two sets: begin_batch() fills the one that is NOT being mapped, so the hand-over of batch k+1 (pack into
	// pinned memory, H2D) runs beside the mapping of batch k; activate_batch() swaps them.
	Resident res_[2];
	int cur_ = 0;
	hipStream_t stage_stream_ = nullptr; // the hand-over's copies (the device's shared stream serves set-up only)
	// all-vs-all name rules
	bool name_rules_ = false;
	const std::vector<std::string> *fi_names_ = nullptr;
	const std::vector<uint32_t> *fi_seq_len_ = nullptr;
	const std::vector<uint64_t> *fi_seq_off_ = nullptr;
	DevBuf<uint64_t> d_ref_off_;
	DevBuf<uint32_t> d_ref_len2_;
	std::mutex ref_mu_;
	std::atomic<bool> ref_ready_{false};
	std::vector<std::string> sorted_names_;
	DevBuf<int32_t> d_name_rank_;
	DevBuf<uint32_t> d_ref_len_;
};

} // namespace

Backend *make_backend(const FlatIndex &fi, void *device_tables, int n_threads, int device, int replica, int tables_device)
{
	return new HipBackend(fi, (DeviceIndexTables *)device_tables, n_threads, device, replica, tables_device);
}
int backend_device_count() { apply_hw_queue_default(); int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }

void *backend_build_index_tables(FlatIndex &fi, int device, int *on_device)
{
	DeviceScope scope(device); DeviceCtx &d = scope.dc;
	std::unique_ptr<DeviceIndexTables> T(new DeviceIndexTables);
	DeviceIndexBuilder::build_from_packed(fi, *T, d.stream);
	if (on_device) *on_device = d.device_id;
	return T.release();
}
void backend_free_index_tables(void *tables) { delete (DeviceIndexTables *)tables; }
const char *backend_name() { return "hip:gfx950"; }

} // namespace mm2amd
