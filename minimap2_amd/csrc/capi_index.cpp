// Index and option entry points of the C ABI (include/mm2amd.h): in-memory index construction on the device
// (mm_idx_str, index.c:421-470) and the option presets (options.c).
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "capi_internal.hpp"
#include "device_ctx.hpp"
#include "index_build.hpp"
#include "index_handle.hpp"
#include "options.hpp"
#include "aln_text.hpp"
#include "junc_text.hpp"
#include <map>

namespace mm2amd {
struct IndexHandle {
	FlatIndex fi;
	DeviceIndexTables T;
	int device = 0;
};
const FlatIndex &index_flat(const IndexHandle *h) { return h->fi; }
void *index_device_tables(const IndexHandle *h) { return (void *)&h->T; }
int index_device(const IndexHandle *h) { return h->device; }
}

using namespace mm2amd;

namespace {
int32_t handle_max_occ(const void *h, float f) { return ((const IndexHandle *)h)->T.cal_max_occ(f); }
}

extern "C" {

mm2amd_index_t *mm2amd_idx_str(int w, int k, int is_hpc, int bucket_bits, int n, const char **seq, const char **name)
{
	(void)bucket_bits; // the flat device table sizes its direct-address level from the number of distinct minimizers
	if (n <= 0 || !seq) { capi_fail(MM2AMD_EINVAL, "[mm2amd] mm2amd_idx_str: need n > 0 sequences"); return nullptr; }
	mm2amd_index_t *out = nullptr;
	guarded([&]() -> int {
		DeviceScope dev; DeviceCtx &dc = dev.dc;
		std::unique_ptr<IndexHandle> h(new IndexHandle);
		h->device = dc.device_id;
		std::vector<uint64_t> lens(n);
		for (int i = 0; i < n; ++i) lens[i] = seq[i] ? strlen(seq[i]) : 0;
		int flag = 0;
		if (is_hpc) flag |= ref::I_HPC;
		if (!name) flag |= ref::I_NO_NAME;
		DeviceIndexBuilder::build(h->fi, h->T, k, w, flag, n, seq, lens.data(), name, dc.stream);
		out = (mm2amd_index_t *)h.release();
		return 0;
	});
	return out;
}

void mm2amd_idx_destroy(mm2amd_index_t *idx) { delete (IndexHandle *)idx; }

int mm2amd_idx_stat(const mm2amd_index_t *idx, int *k, int *w, int *flag, uint32_t *n_seq, uint64_t *sum_len, uint64_t *n_distinct, uint64_t *n_minimizers)
{
	if (!idx) return capi_fail(MM2AMD_EINVAL, "[mm2amd] null index");
	const IndexHandle *h = (const IndexHandle *)idx;
	if (k) *k = h->fi.k;
	if (w) *w = h->fi.w;
	if (flag) *flag = h->fi.flag;
	if (n_seq) *n_seq = h->fi.n_seq;
	if (sum_len) *sum_len = h->fi.sum_len;
	if (n_distinct) *n_distinct = h->T.n_keys;
	if (n_minimizers) *n_minimizers = h->T.n_pos;
	return 0;
}

int32_t mm2amd_idx_cal_max_occ(const mm2amd_index_t *idx, float f)
{
	if (!idx) return capi_fail(MM2AMD_EINVAL, "[mm2amd] null index");
	try { return handle_max_occ(idx, f); } catch (const std::exception &e) { return capi_fail(MM2AMD_EINVAL, e.what()); }
}

// Copies the flat tables to host memory (any pointer may be null to skip it); sizes come from mm2amd_idx_stat and
// mm2amd_idx_table_shape.  Used by tests to compare the device-built index with the reference's mm_idx_t.
int mm2amd_idx_table_shape(const mm2amd_index_t *idx, int *bucket_bits, int *key_shift)
{
	if (!idx) return capi_fail(MM2AMD_EINVAL, "[mm2amd] null index");
	const IndexHandle *h = (const IndexHandle *)idx;
	if (bucket_bits) *bucket_bits = h->T.bucket_bits;
	if (key_shift) *key_shift = h->T.key_shift;
	return 0;
}

int mm2amd_idx_export(const mm2amd_index_t *idx, uint32_t *bucket_start, uint64_t *keys, uint32_t *val_off, uint64_t *pos, uint32_t *S)
{
	if (!idx) return capi_fail(MM2AMD_EINVAL, "[mm2amd] null index");
	const IndexHandle *h = (const IndexHandle *)idx;
	try {
		DeviceScope dev(h->device);
		if (bucket_start) HIP_CHECK(hipMemcpy(bucket_start, h->T.bucket_start.p, ((1ull << h->T.bucket_bits) + 1) * 4, hipMemcpyDeviceToHost));
		if (keys && h->T.n_keys) HIP_CHECK(hipMemcpy(keys, h->T.keys.p, h->T.n_keys * 8, hipMemcpyDeviceToHost));
		if (val_off) HIP_CHECK(hipMemcpy(val_off, h->T.val_off.p, (h->T.n_keys + 1) * 4, hipMemcpyDeviceToHost));
		if (pos && h->T.n_pos) HIP_CHECK(hipMemcpy(pos, h->T.pos.p, h->T.n_pos * 8, hipMemcpyDeviceToHost));
		if (S && h->fi.S) memcpy(S, h->fi.S, (h->fi.sum_len + 7) / 8 * 4); // (an index loaded from an MM_I_NO_SEQ file has none)
		return 0;
	} catch (const std::exception &e) {
		return capi_fail(MM2AMD_EHIP, e.what());
	}
}

/* ---- .mmi files (index_build.hip) ---- */

int mm2amd_idx_dump(const mm2amd_index_t *idx, const char *fn, int bucket_bits, int flags)
{
	if (!idx || !fn) return capi_fail(MM2AMD_EINVAL, "[mm2amd] mm2amd_idx_dump: null argument");
	const IndexHandle *h = (const IndexHandle *)idx;
	FILE *fp = nullptr;
	int rc = 0;
	try {
		DeviceScope dev(h->device); DeviceCtx &dc = dev.dc;
		// what the format cannot hold is refused before the file is touched
		if (bucket_bits <= 0) bucket_bits = 14;
		if (bucket_bits > 2 * h->fi.k || bucket_bits > 28) throw std::invalid_argument("[mm2amd] index dump: bucket_bits must be in [1, 2k] and at most 28");
		if (!(flags & MM2AMD_DUMP_NO_SEQ) && !h->fi.S) throw std::invalid_argument("[mm2amd] index dump: the index has no sequence (pass MM2AMD_DUMP_NO_SEQ)");
		for (const std::string &nm : h->fi.names)
			if (nm.size() > 255) throw std::invalid_argument("[mm2amd] index dump: sequence name longer than 255 bytes: " + nm.substr(0, 32) + "...");
		fp = fopen(fn, "wb");
		if (!fp) return capi_fail(MM2AMD_EIO, std::string("[mm2amd] index dump: cannot open ") + fn + ": " + strerror(errno));
		DeviceIndexBuilder::dump(h->fi, h->T, fp, bucket_bits, (flags & MM2AMD_DUMP_NO_SEQ) != 0, dc.stream);
		if (fclose(fp) != 0) { fp = nullptr; throw IdxIoError(std::string("[mm2amd] index dump: write failed: ") + strerror(errno)); }
		return 0;
	} catch (const IdxIoError &e) {
		rc = capi_fail(MM2AMD_EIO, e.what());
	} catch (const HipError &e) {
		rc = capi_fail(MM2AMD_EHIP, e.what());
	} catch (const std::exception &e) {
		rc = capi_fail(MM2AMD_EINVAL, e.what());
	}
	if (fp) fclose(fp), remove(fn); // no partial file
	else if (rc == MM2AMD_EIO) remove(fn);
	return rc;
}

int mm2amd_idx_is_idx(const char *fn)
{
	if (!fn) return capi_fail(MM2AMD_EINVAL, "[mm2amd] mm2amd_idx_is_idx: null file name");
	if (strcmp(fn, "-") == 0) return 0;
	const int fd = open(fn, O_RDONLY);
	if (fd < 0) return capi_fail(MM2AMD_EIO, std::string("[mm2amd] cannot open ") + fn + ": " + strerror(errno));
	char magic[4];
	const ssize_t r = read(fd, magic, 4);
	close(fd);
	return r == 4 && memcmp(magic, "MMI\2", 4) == 0 ? 1 : 0;
}

mm2amd_index_t *mm2amd_idx_load(const char *fn, int part, int *more)
{
	if (more) *more = 0;
	if (!fn || part < 0) { capi_fail(MM2AMD_EINVAL, "[mm2amd] mm2amd_idx_load: need a file name and part >= 0"); return nullptr; }
	const int fd = open(fn, O_RDONLY);
	if (fd < 0) { capi_fail(MM2AMD_EIO, std::string("[mm2amd] index load: cannot open ") + fn + ": " + strerror(errno)); return nullptr; }
	struct FdGuard { int fd; ~FdGuard() { close(fd); } } guard{fd};
	mm2amd_index_t *out = nullptr;
	guarded([&]() -> int {
		struct stat sb;
		if (fstat(fd, &sb) != 0) throw IdxIoError(std::string("[mm2amd] index load: cannot stat ") + fn + ": " + strerror(errno));
		const uint64_t file_size = (uint64_t)sb.st_size;
		uint64_t off = 0;
		for (int p = 0; p < part; ++p) off = DeviceIndexBuilder::skip_part(fd, file_size, off);
		DeviceScope dev; DeviceCtx &dc = dev.dc;
		std::unique_ptr<IndexHandle> h(new IndexHandle);
		h->device = dc.device_id;
		const uint64_t end = DeviceIndexBuilder::load(h->fi, h->T, fd, file_size, off, dc.stream);
		if (more) *more = end < file_size ? 1 : 0;
		out = (mm2amd_index_t *)h.release();
		return 0;
	});
	return out;
}

int mm2amd_idx_seq(const mm2amd_index_t *idx, uint32_t i, const char **name, uint32_t *len)
{
	if (!idx) return capi_fail(MM2AMD_EINVAL, "[mm2amd] null index");
	const IndexHandle *h = (const IndexHandle *)idx;
	if (i >= h->fi.n_seq) return capi_fail(MM2AMD_EINVAL, "[mm2amd] mm2amd_idx_seq: no such sequence");
	if (name) *name = (h->fi.flag & ref::I_NO_NAME) ? nullptr : h->fi.names[i].c_str();
	if (len) *len = h->fi.seq_len[i];
	return 0;
}

int mm2amd_idx_getseq(const mm2amd_index_t *idx, uint32_t rid, uint32_t st, uint32_t en, uint8_t *out)
{
	if (!idx) return capi_fail(MM2AMD_EINVAL, "[mm2amd] null index");
	const IndexHandle *h = (const IndexHandle *)idx;
	if ((h->fi.flag & ref::I_NO_SEQ) || !h->fi.S) return capi_fail(MM2AMD_EINVAL, "[mm2amd] mm2amd_idx_getseq: the index holds no sequence");
	if (rid >= h->fi.n_seq || st > en || en > h->fi.seq_len[rid] || (en > st && !out)) return capi_fail(MM2AMD_EINVAL, "[mm2amd] mm2amd_idx_getseq: no such sequence or range");
	h->fi.getseq(rid, st, en, out);
	return (int)(en - st);
}

int mm2amd_hits_text_batch(const mm2amd_index_t *idx, int n_hits, const void *const *hit, const char *const *qseq, const int32_t *qlen,
                           int what, int is_qstrand, mm2amd_txt_res_t *res, char *pool, size_t pool_cap)
{
	if (!idx) return capi_fail(MM2AMD_EINVAL, "[mm2amd] null index");
	if (n_hits < 0 || (n_hits > 0 && (!hit || !qseq || !qlen || !res)) || what < MM2AMD_TXT_CIGAR || what > MM2AMD_TXT_DS_LONG) return capi_fail(MM2AMD_EINVAL, "[mm2amd] hits_text_batch: bad arguments");
	const IndexHandle *h = (const IndexHandle *)idx;
	const FlatIndex &fi = h->fi;
	if ((fi.flag & ref::I_NO_SEQ) || !fi.S || !h->T.S.p) return capi_fail(MM2AMD_EINVAL, "[mm2amd] hits_text_batch: the index holds no sequence");
	if (n_hits == 0) return 0;
	return guarded([&]() -> int {
		std::vector<TxtJob> tj(n_hits);
		size_t qtot = 0, ctot = 0;
		for (int i = 0; i < n_hits; ++i) {
			const ref::Reg1 *r = (const ref::Reg1 *)hit[i];
			TxtJob &o = tj[i];
			memset(&o, 0, sizeof o);
			if (!r) return capi_fail(MM2AMD_EINVAL, "[mm2amd] hits_text_batch: null hit");
			if (!r->p) continue; // no base-level alignment: the reference writes nothing (format.c:339)
			if (r->rid < 0 || (uint32_t)r->rid >= fi.n_seq || r->rs < 0 || r->rs > r->re || (uint32_t)r->re > fi.seq_len[r->rid])
				return capi_fail(MM2AMD_EINVAL, "[mm2amd] hits_text_batch: a hit lies outside its reference sequence");
			if (r->qs < 0 || r->qs > r->qe || r->qe > qlen[i] || (r->qe > r->qs && !qseq[i])) return capi_fail(MM2AMD_EINVAL, "[mm2amd] hits_text_batch: a hit lies outside its read");
			const uint64_t so = fi.seq_off[r->rid];
			o.q_pos = qtot, o.cig_off = ctot, o.n_cigar = r->p->n_cigar, o.qlen = r->qe - r->qs, o.tlen = r->re - r->rs;
			if (is_qstrand) { // format.c:343-346: mm_idx_getseq2's window, the read as it is
				o.qsrc = (uint8_t)kTxtQAscii;
				o.tsrc = (uint8_t)(r->rev ? kTxtTPackedRev : kTxtTPacked);
				o.t_pos = r->rev ? so + (fi.seq_len[r->rid] - (uint32_t)r->re) : so + (uint32_t)r->rs;
			} else { // format.c:347-358
				o.qsrc = (uint8_t)(r->rev ? kTxtQAsciiRev : kTxtQAscii);
				o.tsrc = (uint8_t)kTxtTPacked, o.t_pos = so + (uint32_t)r->rs;
			}
			qtot += (size_t)o.qlen, ctot += (size_t)o.n_cigar;
		}
		std::vector<uint8_t> hq(qtot), ht;
		std::vector<uint32_t> cig(ctot);
		for (int i = 0; i < n_hits; ++i) {
			const ref::Reg1 *r = (const ref::Reg1 *)hit[i];
			if (!r->p) continue;
			if (tj[i].qlen) memcpy(&hq[tj[i].q_pos], qseq[i] + r->qs, (size_t)tj[i].qlen);
			if (tj[i].n_cigar) memcpy(&cig[tj[i].cig_off], r->p->cigar, (size_t)tj[i].n_cigar * 4);
		}
		DeviceScope dev(h->device);
		return aln_text_run(dev.dc, tj, what, hq, ht, h->T.S.p, cig, res, pool, pool_cap);
	});
}

int mm2amd_hits_junc_batch(const mm2amd_index_t *idx, int n_hits, const void *const *hit, const char *const *qname, mm2amd_txt_res_t *res, char *pool, size_t pool_cap)
{
	if (!idx) return capi_fail(MM2AMD_EINVAL, "[mm2amd] null index");
	if (n_hits < 0 || (n_hits > 0 && (!hit || !qname || !res))) return capi_fail(MM2AMD_EINVAL, "[mm2amd] hits_junc_batch: bad arguments");
	const IndexHandle *h = (const IndexHandle *)idx;
	const FlatIndex &fi = h->fi;
	if (fi.flag & ref::I_NO_NAME) return capi_fail(MM2AMD_EINVAL, "[mm2amd] hits_junc_batch: the index holds no sequence names");
	if ((fi.flag & ref::I_NO_SEQ) || !fi.S || !h->T.S.p) return capi_fail(MM2AMD_EINVAL, "[mm2amd] hits_junc_batch: the index holds no sequence");
	if (n_hits == 0) return 0;
	return guarded([&]() -> int {
		std::vector<RecJob> jobs;
		std::vector<RecHit> hits;
		std::vector<int> slot;
		std::vector<uint32_t> cig;
		std::string names, tnames;
		std::vector<uint64_t> tname_off(1, 0);
		std::map<int32_t, int32_t> tslot; // rid -> its name's place in tname_off
		for (int i = 0; i < n_hits; ++i) {
			const ref::Reg1 *r = (const ref::Reg1 *)hit[i];
			if (!r || !qname[i]) return capi_fail(MM2AMD_EINVAL, "[mm2amd] hits_junc_batch: null hit or name");
			if (!r->is_spliced || !r->p || (r->p->trans_strand != 1 && r->p->trans_strand != 2)) continue; // format.c:267-268
			if (r->rid < 0 || (uint32_t)r->rid >= fi.n_seq || r->rs < 0 || r->rs > r->re || (uint32_t)r->re > fi.seq_len[r->rid])
				return capi_fail(MM2AMD_EINVAL, "[mm2amd] hits_junc_batch: a hit lies outside its reference sequence");
			auto ts = tslot.find(r->rid);
			if (ts == tslot.end()) {
				ts = tslot.emplace(r->rid, (int32_t)tname_off.size() - 1).first;
				tnames += fi.names[r->rid], tname_off.push_back(tnames.size());
			}
			RecHit o;
			memset(&o, 0, sizeof o);
			o.rid = ts->second, o.rs = r->rs, o.re = r->re, o.qs = r->qs, o.qe = r->qe, o.n_cigar = r->p->n_cigar, o.cig_off = cig.size(), o.t_pos = fi.seq_off[r->rid];
			o.bits = r->mapq | (r->rev ? kRecRev : 0u) | kRecHasP | kRecIsSpliced | (r->id == r->parent ? kRecIsParent : 0u) | (uint32_t)r->p->trans_strand << kRecTransShift;
			RecJob J;
			memset(&J, 0, sizeof J);
			J.name_off = names.size(), J.name_len = (uint32_t)strlen(qname[i]), J.rep_len = -1, J.hit = (int32_t)hits.size(), J.hit0 = (uint32_t)hits.size(), J.n_hits = 1;
			names.append(qname[i], J.name_len);
			cig.insert(cig.end(), r->p->cigar, r->p->cigar + r->p->n_cigar);
			jobs.push_back(J), hits.push_back(o), slot.push_back(i);
		}
		DeviceScope dev(h->device);
		return junc_text_run(dev.dc, jobs, hits, slot, n_hits, names, tnames, tname_off, h->T.S.p, cig, res, pool, pool_cap);
	});
}

int mm2amd_idx_io_stats(double *v, int n)
{
	const IdxIoStats &s = idx_io_stats();
	const double a[] = { s.total_ms, s.regroup_ms, s.kernel_ms, s.copy_ms, s.file_ms, s.sort_ms, s.tables_ms, s.seq_ms, s.image_bytes, s.file_bytes, s.n_chunks, s.chunk_bytes };
	const int m = (int)(sizeof a / sizeof a[0]);
	for (int i = 0; i < n && i < m; ++i) v[i] = a[i];
	return m;
}

void mm2amd_idxopt_init(void *io) { idxopt_init((ref::IdxOpt *)io); }
void mm2amd_mapopt_init(void *mo) { mapopt_init((ref::MapOpt *)mo); }
int mm2amd_set_opt(const char *preset, void *io, void *mo)
{
	if (!io || !mo) return capi_fail(MM2AMD_EINVAL, "[mm2amd] mm2amd_set_opt: null option struct");
	return set_opt(preset, (ref::IdxOpt *)io, (ref::MapOpt *)mo);
}
int mm2amd_check_opt(const void *io, const void *mo)
{
	std::string why;
	const int rc = check_opt((const ref::IdxOpt *)io, (const ref::MapOpt *)mo, &why);
	if (rc != 0) capi_fail(rc, "[mm2amd] " + why);
	return rc;
}
int mm2amd_mapopt_update(void *mo, const mm2amd_index_t *idx)
{
	if (!mo || !idx) return capi_fail(MM2AMD_EINVAL, "[mm2amd] mm2amd_mapopt_update: null argument");
	try { mapopt_update((ref::MapOpt *)mo, handle_max_occ, idx); return 0; } catch (const std::exception &e) { return capi_fail(MM2AMD_EINVAL, e.what()); }
}

} // extern "C"
