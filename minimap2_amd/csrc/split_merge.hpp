// Mapping against a multi-part index (--split-prefix): the temp files of the first pass and the merge pass (splitidx.c, map.c:476-539,
// :589-600, :693-736).  Included by capi_kernels.cpp, which has the entry points' helpers; DESIGN.md section 3i.
//   writer   PREFIX.NNNN.tmp in the reference's layout: k, n_seq, per sequence (name length, name, length); per read segment n_reg, rep_len,
//            frag_gap and per hit the raw mm_reg1_t (its p field zeroed), with MM_F_CIGAR followed by capacity and the mm_extra_t block.
//   merger   opens the parts, keeps their names and lengths as an index without sequence or minimizers, and per mini-batch reads every
//            segment's records from all parts, shifts rid, and applies merge_hits' steps.  mm_update_dp_max before and mm_set_mapq2 / mm_pair after
//            are the host's (hits.cpp; with MM2AMD_DEVICE_PAIR=1 mm_pair goes to pair_kernel); the rules between them go to hits_merge_kernel or, with MM2AMD_DEVICE_MERGE=0 -- and by default, see the
//            measurement in DESIGN.md -- to hits.cpp's own routines.
#pragma once
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/mm2amd.h"
#include "flat_index.hpp"
#include "format.hpp"
#include "hits.hpp"
#include "hits_merge.hpp"
#include "pair.hpp"

namespace mm2amd {

inline std::string split_tmp_name(const std::string &prefix, int part)
{
	char buf[32];
	snprintf(buf, sizeof buf, ".%.4d.tmp", part);
	return prefix + buf;
}

struct SplitWriter {
	FILE *fp = nullptr;
	std::string fn;
	bool cigar = false;
	void put(const void *p, size_t n) { if (n && fwrite(p, 1, n, fp) != n) throw std::runtime_error("[mm2amd] split: cannot write to " + fn + ": " + strerror(errno)); }
	~SplitWriter() { if (fp) fclose(fp); }
};

inline SplitWriter *split_open(const std::string &prefix, const FlatIndex &fi, int part)
{
	SplitWriter *w = new SplitWriter;
	w->fn = split_tmp_name(prefix, part);
	if (!(w->fp = fopen(w->fn.c_str(), "wb"))) { const std::string e = "[mm2amd] split: cannot open " + w->fn + ": " + strerror(errno); delete w; throw std::runtime_error(e); }
	try {
		const uint32_t k = (uint32_t)fi.k;
		w->put(&k, 4), w->put(&fi.n_seq, 4);
		for (uint32_t i = 0; i < fi.n_seq; ++i) {
			const uint32_t l = (uint32_t)fi.names[i].size();
			w->put(&l, 4), w->put(fi.names[i].data(), l), w->put(&fi.seq_len[i], 4);
		}
	} catch (...) { delete w; throw; }
	return w;
}

inline void split_write(SplitWriter &w, int n_seq, const int *n_reg, void *const *reg, const int *rep_len, const int *frag_gap)
{
	for (int i = 0; i < n_seq; ++i) {
		w.put(&n_reg[i], 4), w.put(&rep_len[i], 4), w.put(&frag_gap[i], 4);
		const ref::Reg1 *r = (const ref::Reg1 *)reg[i];
		for (int j = 0; j < n_reg[i]; ++j) {
			ref::Reg1 t = r[j];
			t.p = nullptr; // (the reference writes the pointer's bytes; nothing reads them)
			w.put(&t, sizeof t);
			if (w.cigar) {
				if (!r[j].p) throw std::invalid_argument("[mm2amd] split: a hit without alignment in a run with MM_F_CIGAR");
				w.put(&r[j].p->capacity, 4), w.put(r[j].p, (size_t)r[j].p->capacity * 4);
			}
		}
	}
}

struct SplitMerger {
	std::string prefix;
	std::vector<FILE *> fp;
	std::vector<uint32_t> rid_shift;
	FlatIndex fi;          // names and lengths only
	ref::MapOpt opt;
	mm2amd_hm_opt_t hm;
	bool device = false;
	bool device_pair = false; // MM2AMD_DEVICE_PAIR=1: mm_pair through mm2amd_pair_batch, one call per mini-batch
	void get(int j, void *p, size_t n) { if (n && fread(p, 1, n, fp[(size_t)j]) != n) throw std::runtime_error("[mm2amd] split: " + split_tmp_name(prefix, j) + " ends early"); }
	~SplitMerger() { for (FILE *f : fp) if (f) fclose(f); }
};

inline bool split_device_default() { return false; } // the host route: DESIGN.md section 3i has the measurement
inline bool split_device_route()
{
	const char *e = getenv("MM2AMD_DEVICE_MERGE");
	return e && *e ? strcmp(e, "0") != 0 : split_device_default();
}

inline SplitMerger *split_merge_open(const std::string &prefix, int n_parts, const ref::MapOpt &opt)
{
	constexpr int64_t kNoText = 0x040LL | 0x1000000LL | 0x2000000000LL | 0x10000000000LL; // MM_F_OUT_CS, _MD, _DS, _JUNC
	if (n_parts < 1) throw std::invalid_argument("[mm2amd] split: no parts");
	if (opt.flag & kNoText) throw std::invalid_argument("[mm2amd] split: --cs, --MD, --ds and --write-junc do not work with --split-prefix (the merge pass has no sequence)");
	SplitMerger *m = new SplitMerger;
	try {
		m->prefix = prefix, m->opt = opt, m->opt.split_prefix = nullptr;
		for (int j = 0; j < n_parts; ++j) {
			FILE *f = fopen(split_tmp_name(prefix, j).c_str(), "rb");
			if (!f) throw std::runtime_error("[mm2amd] split: cannot open " + split_tmp_name(prefix, j) + ": " + strerror(errno));
			m->fp.push_back(f);
		}
		std::vector<uint32_t> n_seq_part((size_t)n_parts);
		for (int j = 0; j < n_parts; ++j) { uint32_t k; m->get(j, &k, 4), m->get(j, &n_seq_part[(size_t)j], 4); m->fi.k = (int)k; m->fi.n_seq += n_seq_part[(size_t)j]; }
		m->rid_shift.assign((size_t)n_parts, 0);
		for (int j = 1; j < n_parts; ++j) m->rid_shift[(size_t)j] = m->rid_shift[(size_t)j - 1] + n_seq_part[(size_t)j - 1];
		uint64_t off = 0;
		for (int j = 0; j < n_parts; ++j)
			for (uint32_t s = 0; s < n_seq_part[(size_t)j]; ++s) {
				uint32_t l, len;
				m->get(j, &l, 4);
				if (l > (1u << 20)) throw std::runtime_error("[mm2amd] split: bad header in " + split_tmp_name(prefix, j));
				std::string name(l, '\0');
				m->get(j, &name[0], l), m->get(j, &len, 4);
				m->fi.names.push_back(name), m->fi.seq_len.push_back(len), m->fi.seq_off.push_back(off), m->fi.is_alt.push_back(0);
				off += len;
			}
		m->fi.sum_len = off, m->fi.flag = ref::I_NO_SEQ;
		mm2amd_hm_opt_t &h = m->hm;
		h.mask_level = opt.mask_level, h.mask_len = opt.mask_len, h.pri_ratio = opt.pri_ratio, h.best_n = opt.best_n, h.alt_drop = opt.alt_drop;
		h.sub_diff = opt.a * 2 + opt.b, h.min_diff = m->fi.k * 2, h.min_strand_sc = (int)(opt.max_gap * 0.8); // (map.c:527-529)
		h.flags = (opt.flag & ref::F_HARD_MLEVEL ? MM2AMD_HM_HARD_MLEVEL : 0u) | (opt.flag & ref::F_ALL_CHAINS ? MM2AMD_HM_ALL_CHAINS : 0u);
	} catch (...) { delete m; throw; }
	return m;
}

// a segment's list after the kernel's (or the host twin's) answers: the kept hits in their final places, the alignments of the others freed
inline void split_apply(RegVec &regs, const mm2amd_hm_out_t *out, int n_kept)
{
	RegVec fin((size_t)n_kept);
	for (size_t k = 0; k < regs.size(); ++k) {
		const mm2amd_hm_out_t &o = out[k];
		if (o.pos < 0 || o.pos >= n_kept) { free(regs[k].p); continue; }
		Reg &r = fin[(size_t)o.pos];
		r = regs[k];
		r.id = o.id, r.parent = o.parent, r.subsc = o.subsc, r.n_sub = o.n_sub;
		r.sam_pri = o.flags & MM2AMD_HM_SAM_PRI ? 1 : 0, r.strand_retained = o.flags & MM2AMD_HM_STRAND_RETAINED ? 1 : 0;
		if (r.p) r.p->dp_max2 = o.dp_max2;
	}
	regs.swap(fin);
}

inline void split_flat_hit(mm2amd_hm_hit_t &h, const Reg &r)
{
	h.cnt = r.cnt, h.rid = r.rid, h.score = r.score, h.qs = r.qs, h.qe = r.qe, h.rs = r.rs, h.re = r.re, h.dp_max = r.p ? r.p->dp_max : 0, h.hash = r.hash;
	h.flags = (r.rev ? MM2AMD_HM_REV : 0u) | (r.inv ? MM2AMD_HM_INV : 0u) | (r.is_alt ? MM2AMD_HM_ALT : 0u) | (r.p ? MM2AMD_HM_ALIGNED : 0u) | (r.sam_pri ? MM2AMD_HM_SAM_PRI : 0u) |
	          (r.strand_retained ? MM2AMD_HM_STRAND_RETAINED : 0u);
}

// merge_hits (map.c:476-539) for the next n_frag fragments of the read files; reg[i]: one libc block per segment, as the mapping calls return them
inline void split_merge_batch(SplitMerger &m, int n_frag, const int *seg_off, const int *n_seg, const ref::Bseq1 *seq, int *n_reg, void **reg, int *rep_len, int *frag_gap)
{
	const ref::MapOpt &opt = m.opt;
	const int n_parts = (int)m.fp.size();
	int n_total = 0;
	for (int f = 0; f < n_frag; ++f) { const int e = (seg_off ? seg_off[f] : f) + (n_seg ? n_seg[f] : 1); n_total = e > n_total ? e : n_total; }
	std::vector<RegVec> all((size_t)n_total);
	std::vector<int> part_n((size_t)n_parts);
	const bool cigar = (opt.flag & ref::F_CIGAR) != 0;
	try {
		for (int f = 0; f < n_frag; ++f) { // the files hold the segments in this order
			const int st = seg_off ? seg_off[f] : f, ns = n_seg ? n_seg[f] : 1;
			for (int k = st; k < st + ns; ++k) {
				int rl = 0, fg0 = 0;
				for (int j = 0; j < n_parts; ++j) {
					int v[3];
					m.get(j, v, 12);
					if (v[0] < 0 || v[0] > kHmMaxHits) throw std::runtime_error("[mm2amd] split: bad record count in " + split_tmp_name(m.prefix, j));
					part_n[(size_t)j] = v[0], rl = rl < v[1] ? v[1] : rl;
					if (j == 0) fg0 = v[2];
				}
				rep_len[k] = rl, frag_gap[k] = fg0;
				RegVec &regs = all[(size_t)k];
				for (int j = 0; j < n_parts; ++j)
					for (int t = 0; t < part_n[(size_t)j]; ++t) {
						Reg r;
						m.get(j, &r, sizeof r);
						r.p = nullptr, r.rid += (int32_t)m.rid_shift[(size_t)j];
						regs.push_back(r);
						if (cigar) {
							uint32_t cap;
							m.get(j, &cap, 4);
							if (cap < sizeof(ref::Extra) / 4 || cap > (1u << 28)) throw std::runtime_error("[mm2amd] split: bad alignment block in " + split_tmp_name(m.prefix, j));
							ref::Extra *p = (ref::Extra *)calloc(cap, 4);
							if (!p) throw std::bad_alloc();
							regs.back().p = p;
							m.get(j, p, (size_t)cap * 4);
							if (p->capacity != cap || (uint64_t)p->n_cigar + sizeof(ref::Extra) / 4 > cap) throw std::runtime_error("[mm2amd] split: bad alignment block in " + split_tmp_name(m.prefix, j));
						}
					}
				if (!(opt.flag & ref::F_SR) && seq[k].l_seq >= opt.rank_min_len) update_dp_max(seq[k].l_seq, regs, opt.rank_frac, opt.a, opt.b);
				for (Reg &r : regs) { if (r.p) r.p->dp_max2 = 0; r.subsc = 0, r.n_sub = 0; }
			}
		}
		if (m.device) { // the rules between mm_update_dp_max and mm_set_mapq2 on hits_merge_kernel, the whole mini-batch in one call
			std::vector<uint64_t> off((size_t)n_total + 1, 0);
			for (int k = 0; k < n_total; ++k) off[(size_t)k + 1] = off[(size_t)k] + all[(size_t)k].size();
			std::vector<mm2amd_hm_hit_t> hits((size_t)off[(size_t)n_total] + 1);
			std::vector<mm2amd_hm_out_t> out(hits.size());
			std::vector<mm2amd_hm_seg_t> sg((size_t)n_total + 1);
			for (int k = 0; k < n_total; ++k) for (size_t t = 0; t < all[(size_t)k].size(); ++t) split_flat_hit(hits[(size_t)off[(size_t)k] + t], all[(size_t)k][t]);
			if (n_total > 0 && mm2amd_hits_merge_batch(n_total, off.data(), hits.data(), &m.hm, out.data(), sg.data()) != 0) throw std::runtime_error(mm2amd_last_error());
			for (int k = 0; k < n_total; ++k) split_apply(all[(size_t)k], out.data() + off[(size_t)k], sg[(size_t)k].n_kept);
		} else {
			for (int k = 0; k < n_total; ++k) {
				RegVec &regs = all[(size_t)k];
				hit_sort(regs, opt.alt_drop);
				set_parent(opt.mask_level, opt.mask_len, regs, m.hm.sub_diff, (opt.flag & ref::F_HARD_MLEVEL) != 0, opt.alt_drop);
				if (!(opt.flag & ref::F_ALL_CHAINS)) {
					select_sub(opt.pri_ratio, m.hm.min_diff, opt.best_n, false, m.hm.min_strand_sc, regs);
					set_sam_pri(regs);
				}
			}
		}
		for (int f = 0; f < n_frag; ++f) {
			const int st = seg_off ? seg_off[f] : f, ns = n_seg ? n_seg[f] : 1;
			for (int k = st; k < st + ns; ++k)
				set_mapq(all[(size_t)k], opt.min_chain_score, opt.a, rep_len[k], (opt.flag & (ref::F_SR | ref::F_SR_RNA)) != 0, (opt.flag & ref::F_SPLICE) != 0);
			if (ns == 2 && opt.pe_ori >= 0 && cigar && !m.device_pair) {
				const int qlens[2] = { seq[st].l_seq, seq[st + 1].l_seq };
				pair_hits(frag_gap[st + 1], opt.pe_bonus, opt.a * 2 + opt.b, opt.a, qlens, &all[(size_t)st]);
			}
		}
		if (m.device_pair && opt.pe_ori >= 0 && cigar) { // mm_pair on pair_kernel: the mini-batch's two-segment fragments flattened, one call, the answers put back
			std::vector<mm2amd_pe_frag_t> fr;
			std::vector<int> first_seg;
			uint64_t n_hits = 0;
			for (int f = 0; f < n_frag; ++f) {
				const int st = seg_off ? seg_off[f] : f, ns = n_seg ? n_seg[f] : 1;
				if (ns != 2) continue;
				mm2amd_pe_frag_t F;
				F.hit0 = n_hits, F.n[0] = (int32_t)all[(size_t)st].size(), F.n[1] = (int32_t)all[(size_t)st + 1].size();
				F.qlen[0] = seq[st].l_seq, F.qlen[1] = seq[st + 1].l_seq, F.max_gap_ref = frag_gap[st + 1], F.reserved = 0;
				n_hits += (uint64_t)F.n[0] + (uint64_t)F.n[1];
				fr.push_back(F), first_seg.push_back(st);
			}
			std::vector<mm2amd_pe_hit_t> hits((size_t)n_hits + 1);
			std::vector<mm2amd_pe_out_t> out(hits.size());
			std::vector<mm2amd_pe_res_t> res(fr.size() + 1);
			for (size_t k = 0; k < fr.size(); ++k) {
				size_t at = (size_t)fr[k].hit0;
				for (int s = 0; s < 2; ++s) for (const Reg &r : all[(size_t)first_seg[k] + s]) pe_flat_hit(hits[at++], r);
			}
			const mm2amd_pe_opt_t po = { opt.pe_bonus, opt.a * 2 + opt.b, opt.a, 0 };
			if (!fr.empty() && mm2amd_pair_batch((int)fr.size(), fr.data(), hits.data(), &po, out.data(), res.data()) != 0) throw std::runtime_error(mm2amd_last_error());
			for (size_t k = 0; k < fr.size(); ++k) {
				if (res[k].status != MM2AMD_PE_OK) throw std::runtime_error("[mm2amd] split: a hit's parent does not index its segment");
				size_t at = (size_t)fr[k].hit0;
				for (int s = 0; s < 2; ++s) for (Reg &r : all[(size_t)first_seg[k] + s]) pe_apply(r, out[at++]);
			}
		}
		for (int k = 0; k < n_total; ++k) {
			const RegVec &regs = all[(size_t)k];
			n_reg[k] = (int)regs.size(), reg[k] = nullptr;
			if (regs.empty()) continue;
			if (!(reg[k] = malloc(regs.size() * sizeof(Reg)))) throw std::bad_alloc();
			memcpy(reg[k], regs.data(), regs.size() * sizeof(Reg));
			all[(size_t)k].clear();
		}
	} catch (...) {
		for (RegVec &v : all) for (Reg &r : v) free(r.p);
		throw;
	}
}

inline std::string split_sq_lines(const SplitMerger &m)
{
	std::string s;
	for (uint32_t i = 0; i < m.fi.n_seq; ++i) s += "@SQ\tSN:" + m.fi.names[i] + "\tLN:" + std::to_string(m.fi.seq_len[i]) + "\n";
	return s;
}

} // namespace mm2amd
