// Device-side index construction: the GPU counterpart of mm_idx_gen's sketch -> bucket -> sort -> hash pipeline
// (index.c:226-278, :369-408), producing the flat tables of flat_index.hpp directly in HBM.
//
//   1. encode   : ASCII -> nt4 (1 B/base) and 4-bit packed S (mmpriv.h:34-35)
//   2. sketch   : mm_sketch (sketch.c:77-143) over fixed-size chunks.  The reference's window automaton is
//                 sequential, but its state after any stretch of w+k consecutive valid slots is a function of that
//                 stretch alone (hard part 7), so a lane that starts early enough before its
//                 chunk reaches the true state before its first owned position; each lane emits only minimizers
//                 whose position lies in its own chunk, which partitions the reference's output exactly.
//   3. sort     : (hash, position) pairs by hash, stably, so that positions stay ascending within a hash (device_sort.hip: a hand-written
//                 device-wide LSD radix sort over the 2k hash bits)
//   4. tables   : distinct keys, value offsets (heads of the runs of equal hashes, ranked by a tile count + prefix sum), top-bits direct table
#include <hip/hip_runtime.h>
#include <unistd.h>
#include <algorithm>
#include <cerrno>
#include <cstring>
#include <string>
#include <vector>
#include "hip_util.hpp"
#include "index_build.hpp"
#include "device_sort.hpp"
#include "device_sort_dev.hpp"
#include "sketch_dev.hpp"
#include "fastx_dev.hpp"     // the readers' kernels (fastx_lines_kernel, fastx_classify_kernel, fastx_copy_kernel) as well
#include "tables.hpp"

namespace mm2amd {

__constant__ uint8_t c_nt4_idx[256];

__global__ void __launch_bounds__(256) idx_encode_kernel(const char *ascii, uint8_t *nt4, uint32_t *S, uint64_t total)
{
	// one thread per packed word (8 bases)
	const uint64_t wi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint64_t b0 = wi * 8;
	if (b0 >= total) return;
	uint32_t word = 0;
	for (int j = 0; j < 8 && b0 + j < total; ++j) {
		const uint8_t c = c_nt4_idx[(uint8_t)ascii[b0 + j]];
		nt4[b0 + j] = c;
		word |= (uint32_t)c << (j << 2);
	}
	S[wi] = word;
}

// the reverse: 4-bit packed S (an index loaded from a .mmi or built by the reference carries it, index.c:242-246) -> nt4 bytes
__global__ void __launch_bounds__(256) idx_decode_kernel(const uint32_t *S, uint8_t *nt4, uint64_t total)
{
	const uint64_t wi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint64_t b0 = wi * 8;
	if (b0 >= total) return;
	const uint32_t word = S[wi];
	for (int j = 0; j < 8 && b0 + j < total; ++j) nt4[b0 + j] = (uint8_t)(word >> (j << 2) & 0xf);
}

struct ChunkDesc { uint32_t rid; uint32_t start; }; // chunk = [start, start + CHUNK) clipped to the sequence

// one lane per chunk (sketch_dev.hpp)
template <bool EMIT, int WMAX, bool HPC>
__global__ void __launch_bounds__(64) idx_sketch_kernel(const uint8_t *nt4, const uint64_t *seq_off, const uint32_t *seq_len, const ChunkDesc *chunks,
                                                         uint64_t n_chunks, int chunk_len, int w, int k, uint32_t *cnt, const uint64_t *out_off,
                                                         uint64_t *out_hash, uint64_t *out_pos)
{
	const uint64_t ci = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (ci >= n_chunks) return;
	const uint32_t rid = chunks[ci].rid;
	const int64_t cs = chunks[ci].start, len = seq_len[rid];
	const int64_t ce = cs + chunk_len < len ? cs + chunk_len : len;
	uint64_t bx[WMAX], by[WMAX];
	uint32_t n_out = 0;
	uint64_t *oh = nullptr, *op = nullptr;
	if (EMIT) oh = out_hash + out_off[ci], op = out_pos + out_off[ci];
	sketch_chunk<HPC>(nt4 + seq_off[rid], len, cs, ce, w, k, rid, bx, by, 1, [&](uint64_t x, uint64_t y) {
		if (EMIT) { oh[n_out] = x >> 8; op[n_out] = y; }
		++n_out;
	});
	if (!EMIT) cnt[ci] = n_out;
}

// A head is the first pair of a run of equal hashes: one per distinct minimizer, in sorted order.  Tiles of kSortTile pairs; wave w of
// a tile owns its pairs [1024 w, 1024 (w+1)) and visits them 64 at a time, so a ballot ranks the heads of a round.
__global__ void __launch_bounds__(kSortThreads) idx_count_heads_kernel(const uint64_t *hash, uint64_t n, uint32_t *tile_cnt)
{
	__shared__ uint32_t sh[4];
	const int tid = threadIdx.x;
	const uint64_t base = (uint64_t)blockIdx.x * kSortTile;
	uint32_t c = 0;
#pragma unroll
	for (int r = 0; r < kSortItems; ++r) {
		const uint64_t i = base + (uint64_t)(r * kSortThreads + tid);
		if (i < n && (i == 0 || hash[i] != hash[i - 1])) ++c;
	}
	uint32_t total;
	(void)block_exclusive_sum(c, sh, total);
	if (tid == 0) tile_cnt[blockIdx.x] = total;
}

// keys[] = the distinct hashes, val_off[] = where each one's run of positions starts; tile_off = exclusive prefix sum of the tiles' head counts
__global__ void __launch_bounds__(kSortThreads) idx_scatter_keys_kernel(const uint64_t *hash, uint64_t n, const uint32_t *tile_off, uint64_t *keys, uint32_t *val_off, uint64_t n_keys)
{
	__shared__ uint32_t sh[4];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	const uint64_t base = (uint64_t)blockIdx.x * kSortTile + (uint64_t)(w * (kSortItems * 64) + lane);
	uint64_t key[kSortItems];
	uint32_t heads = 0, wave_cnt = 0;
#pragma unroll
	for (int r = 0; r < kSortItems; ++r) {
		const uint64_t i = base + (uint64_t)(r * 64);
		key[r] = i < n ? hash[i] : 0;
		const bool head = i < n && (i == 0 || hash[i - 1] != key[r]);
		heads |= (uint32_t)head << r;
		wave_cnt += (uint32_t)__popcll(__ballot(head));
	}
	if (lane == 0) sh[w] = wave_cnt;
	__syncthreads();
	uint32_t run = tile_off[blockIdx.x];
	for (int i = 0; i < w; ++i) run += sh[i];
	const uint64_t below = (1ull << lane) - 1;
#pragma unroll
	for (int r = 0; r < kSortItems; ++r) {
		const bool head = heads >> r & 1;
		const uint64_t bal = __ballot(head);
		if (head) {
			const uint32_t rank = run + (uint32_t)__popcll(bal & below);
			keys[rank] = key[r];
			val_off[rank] = (uint32_t)(base + (uint64_t)(r * 64));
		}
		run += (uint32_t)__popcll(bal);
	}
	if (blockIdx.x == 0 && tid == 0) val_off[n_keys] = (uint32_t)n;
}

__global__ void __launch_bounds__(256) idx_bucket_start_kernel(const uint64_t *keys, uint64_t n_keys, int key_shift, uint64_t n_buckets, uint32_t *bucket_start)
{
	const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (b > n_buckets) return;
	// first key whose bucket id is >= b
	uint64_t lo = 0, hi = n_keys;
	while (lo < hi) {
		const uint64_t mid = (lo + hi) >> 1;
		if ((keys[mid] >> key_shift) < b) lo = mid + 1; else hi = mid;
	}
	bucket_start[b] = (uint32_t)lo;
}

__global__ void __launch_bounds__(256) idx_occ_hist_kernel(const uint32_t *val_off, uint64_t n_keys, unsigned long long *hist, int n_bins)
{
	// almost every minimizer occurs a handful of times: count the low bins per block in LDS, the tail with global atomics
	__shared__ unsigned int low[256];
	low[threadIdx.x] = 0;
	__syncthreads();
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_keys; i += stride) {
		uint32_t c = val_off[i + 1] - val_off[i];
		if (c < 256) atomicAdd(&low[c], 1u);
		else atomicAdd(&hist[c < (uint32_t)n_bins ? c : (uint32_t)n_bins - 1], 1ull);
	}
	__syncthreads();
	if (low[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)low[threadIdx.x]);
}

void DeviceIndexBuilder::build(FlatIndex &fi, DeviceIndexTables &T, int k, int w, int flag, int n_seq, const char *const *seqs, const uint64_t *lens,
                               const char *const *names, hipStream_t stream)
{
	if (w <= 0 || w >= 256 || k <= 0 || k > 28) throw std::invalid_argument("[mm2amd] index build: need 0<w<256 and 0<k<=28");
	HIP_CHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_nt4_idx), kNt4Table, 256, 0, hipMemcpyHostToDevice, stream));
	fi.k = k, fi.w = w, fi.flag = flag, fi.n_seq = (uint32_t)n_seq, fi.n_alt = 0;
	fi.names.resize(n_seq), fi.seq_off.resize(n_seq), fi.seq_len.resize(n_seq);
	uint64_t total = 0;
	for (int i = 0; i < n_seq; ++i) {
		if (lens[i] >= (1ull << 31)) throw std::invalid_argument("[mm2amd] reference sequences must be shorter than 2^31 bases");
		fi.names[i] = names && names[i] ? names[i] : "";
		fi.seq_off[i] = total, fi.seq_len[i] = (uint32_t)lens[i];
		total += lens[i];
	}
	fi.sum_len = total;
	const uint64_t n_words = (total + 7) / 8;
	// 1. upload + encode
	DevBuf<char> d_ascii;
	DevBuf<uint8_t> d_nt4;
	d_ascii.ensure(total + 8, 1.0), d_nt4.ensure(total + 8, 1.0);
	T.S.ensure(n_words + 1, 1.0);
	for (int i = 0; i < n_seq; ++i)
		if (lens[i]) HIP_CHECK(hipMemcpyAsync(d_ascii.p + fi.seq_off[i], seqs[i], lens[i], hipMemcpyHostToDevice, stream));
	if (n_words) hipLaunchKernelGGL(idx_encode_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, stream, d_ascii.p, d_nt4.p, T.S.p, total);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipStreamSynchronize(stream));
	d_ascii.release();
	fi.S_own.resize(n_words);
	if (n_words) HIP_CHECK(hipMemcpy(fi.S_own.data(), T.S.p, n_words * 4, hipMemcpyDeviceToHost));
	fi.S = fi.S_own.data();
	tables_from_nt4(fi, T, d_nt4, stream);
}

// The minimizer tables of an index whose sequence is already packed (fi.S; k, w, flag, the sequence table and sum_len set): what
// mm_gpu_init does with a reference mm_idx_t instead of walking its 2^14 hash tables on the host -- a 3 Gb index is rebuilt in
// about a second, and tools/e2e_wall.py checks once at full size that the result equals the reference's own mm_idx_gen.
void DeviceIndexBuilder::build_from_packed(FlatIndex &fi, DeviceIndexTables &T, hipStream_t stream)
{
	if (fi.w <= 0 || fi.w >= 256 || fi.k <= 0 || fi.k > 28) throw std::invalid_argument("[mm2amd] index build: need 0<w<256 and 0<k<=28");
	if (!fi.S) throw std::invalid_argument("[mm2amd] index without sequence");
	const uint64_t total = fi.sum_len, n_words = (total + 7) / 8;
	DevBuf<uint8_t> d_nt4;
	d_nt4.ensure(total + 8, 1.0);
	T.S.ensure(n_words + 1, 1.0);
	if (n_words) HIP_CHECK(hipMemcpyAsync(T.S.p, fi.S, n_words * 4, hipMemcpyHostToDevice, stream));
	if (n_words) hipLaunchKernelGGL(idx_decode_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, stream, T.S.p, d_nt4.p, total);
	HIP_CHECK(hipGetLastError());
	tables_from_nt4(fi, T, d_nt4, stream);
}

// steps 2-4: sketch -> sort -> tables, from the nt4 bytes of the concatenated sequences
void DeviceIndexBuilder::tables_from_nt4(FlatIndex &fi, DeviceIndexTables &T, DevBuf<uint8_t> &d_nt4, hipStream_t stream)
{
	const int k = fi.k, w = fi.w, flag = fi.flag, n_seq = (int)fi.n_seq;
	// 2. chunked sketch: count, scan, emit
	const int chunk_len = 2048;
	std::vector<ChunkDesc> chunks;
	for (int i = 0; i < n_seq; ++i)
		for (uint64_t s = 0; s < fi.seq_len[i]; s += chunk_len) chunks.push_back(ChunkDesc{(uint32_t)i, (uint32_t)s});
	const uint64_t n_chunks = chunks.size();
	DevBuf<ChunkDesc> d_chunks;
	DevBuf<uint64_t> d_seq_off, d_out_off;
	DevBuf<uint32_t> d_seq_len, d_cnt;
	d_chunks.ensure(n_chunks + 1, 1.0), d_seq_off.ensure(n_seq + 1, 1.0), d_seq_len.ensure(n_seq + 1, 1.0), d_cnt.ensure(n_chunks + 1, 1.0), d_out_off.ensure(n_chunks + 2, 1.0);
	if (n_chunks) HIP_CHECK(hipMemcpyAsync(d_chunks.p, chunks.data(), n_chunks * sizeof(ChunkDesc), hipMemcpyHostToDevice, stream));
	HIP_CHECK(hipMemcpyAsync(d_seq_off.p, fi.seq_off.data(), n_seq * 8, hipMemcpyHostToDevice, stream));
	HIP_CHECK(hipMemcpyAsync(d_seq_len.p, fi.seq_len.data(), n_seq * 4, hipMemcpyHostToDevice, stream));
	const dim3 sgrid((unsigned)((n_chunks + 63) / 64)), sblock(64);
	const bool hpc = flag & ref::I_HPC;
	auto run_sketch = [&](bool emit, uint64_t *oh, uint64_t *op) {
		if (n_chunks == 0) return;
#define MM2_IDX_SKETCH(E, W, H) hipLaunchKernelGGL((idx_sketch_kernel<E, W, H>), sgrid, sblock, 0, stream, d_nt4.p, d_seq_off.p, d_seq_len.p, d_chunks.p, n_chunks, chunk_len, w, k, d_cnt.p, d_out_off.p, oh, op)
		if (w <= 32) {
			if (hpc) { if (emit) MM2_IDX_SKETCH(true, 32, true); else MM2_IDX_SKETCH(false, 32, true); }
			else { if (emit) MM2_IDX_SKETCH(true, 32, false); else MM2_IDX_SKETCH(false, 32, false); }
		} else {
			if (hpc) { if (emit) MM2_IDX_SKETCH(true, 256, true); else MM2_IDX_SKETCH(false, 256, true); }
			else { if (emit) MM2_IDX_SKETCH(true, 256, false); else MM2_IDX_SKETCH(false, 256, false); }
		}
#undef MM2_IDX_SKETCH
		HIP_CHECK(hipGetLastError());
	};
	run_sketch(false, nullptr, nullptr);
	std::vector<uint32_t> h_cnt(n_chunks);
	if (n_chunks) HIP_CHECK(hipMemcpyAsync(h_cnt.data(), d_cnt.p, n_chunks * 4, hipMemcpyDeviceToHost, stream));
	HIP_CHECK(hipStreamSynchronize(stream));
	std::vector<uint64_t> h_off(n_chunks + 1);
	h_off[0] = 0;
	for (uint64_t i = 0; i < n_chunks; ++i) h_off[i + 1] = h_off[i] + h_cnt[i];
	const uint64_t n_mz = h_off[n_chunks];
	if (n_mz >= (1ull << 32)) throw std::invalid_argument("[mm2amd] more than 2^32 minimizers: split the reference (the reference's -I does the same)");
	HIP_CHECK(hipMemcpyAsync(d_out_off.p, h_off.data(), (n_chunks + 1) * 8, hipMemcpyHostToDevice, stream));
	DevBuf<uint64_t> d_hash, d_pos, d_hash2, d_pos2;
	d_hash.ensure(n_mz + 1, 1.0), d_pos.ensure(n_mz + 1, 1.0), d_hash2.ensure(n_mz + 1, 1.0), d_pos2.ensure(n_mz + 1, 1.0);
	run_sketch(true, d_hash.p, d_pos.p);
	d_nt4.release();
	// 3. sort by (hash, pos): positions are already ascending within a chunk and chunks are in (rid, start) order, so the
	//    pairs are sorted by pos; one stable sort by hash finishes the job (index.c:236 + :265 yield the same order).
	if (device_sort_pairs_u64(d_hash.p, d_pos.p, d_hash2.p, d_pos2.p, n_mz, 2 * k, stream) == 1)
		std::swap(d_hash.p, d_hash2.p), std::swap(d_hash.cap, d_hash2.cap), std::swap(d_pos.p, d_pos2.p), std::swap(d_pos.cap, d_pos2.cap);
	d_hash2.release(), d_pos2.release();
	// 4. tables
	tables_from_sorted(fi, T, d_hash, d_pos, n_mz, k, stream);
}

// step 4: the tables from the pairs sorted by (hash, position).  Shared by the build above and by the .mmi loader below.
uint64_t DeviceIndexBuilder::tables_from_sorted(FlatIndex &fi, DeviceIndexTables &T, DevBuf<uint64_t> &d_hash, DevBuf<uint64_t> &d_pos, uint64_t n_mz, int k, hipStream_t stream)
{
	const uint64_t n_tiles = (n_mz + kSortTile - 1) / kSortTile;
	DevBuf<uint32_t> d_tile;
	d_tile.ensure(n_tiles + 2, 1.0);
	uint64_t n_keys = 0;
	if (n_mz) {
		hipLaunchKernelGGL(idx_count_heads_kernel, dim3((unsigned)n_tiles), dim3(kSortThreads), 0, stream, d_hash.p, n_mz, d_tile.p);
		HIP_CHECK(hipGetLastError());
		device_exclusive_sum_u32(d_tile.p, d_tile.p, n_tiles, stream);
		uint32_t total = 0;
		HIP_CHECK(hipMemcpyAsync(&total, d_tile.p + n_tiles, 4, hipMemcpyDeviceToHost, stream));
		HIP_CHECK(hipStreamSynchronize(stream));
		n_keys = total;
	}
	T.keys.ensure(n_keys + 1, 1.0), T.val_off.ensure(n_keys + 2, 1.0);
	if (n_mz) hipLaunchKernelGGL(idx_scatter_keys_kernel, dim3((unsigned)n_tiles), dim3(kSortThreads), 0, stream, d_hash.p, n_mz, (const uint32_t *)d_tile.p, T.keys.p, T.val_off.p, n_keys);
	else HIP_CHECK(hipMemsetAsync(T.val_off.p, 0, 4, stream));
	HIP_CHECK(hipGetLastError());
	// hand the sorted positions over
	T.pos.release();
	T.pos.p = d_pos.p, T.pos.cap = d_pos.cap, d_pos.p = nullptr, d_pos.cap = 0;
	int hash_bits = 2 * k, want = 1;
	while ((1ull << want) < n_keys && want < 28) ++want;
	T.bucket_bits = std::min(hash_bits, std::max(8, want));
	T.key_shift = hash_bits - T.bucket_bits;
	const uint64_t n_buckets = 1ull << T.bucket_bits;
	T.bucket_start.ensure(n_buckets + 2, 1.0);
	hipLaunchKernelGGL(idx_bucket_start_kernel, dim3((unsigned)((n_buckets + 1 + 255) / 256)), dim3(256), 0, stream, T.keys.p, n_keys, T.key_shift, n_buckets, T.bucket_start.p);
	HIP_CHECK(hipGetLastError());
	T.n_keys = n_keys, T.n_pos = n_mz;
	// occurrence histogram for mm_idx_cal_max_occ (index.c:198-220)
	const int n_bins = 1 << 16;
	DevBuf<unsigned long long> d_hist;
	d_hist.ensure(n_bins, 1.0);
	HIP_CHECK(hipMemsetAsync(d_hist.p, 0, n_bins * 8, stream));
	if (n_keys) hipLaunchKernelGGL(idx_occ_hist_kernel, dim3((unsigned)std::min<uint64_t>((n_keys + 255) / 256, 4096)), dim3(256), 0, stream, T.val_off.p, n_keys, d_hist.p, n_bins);
	T.occ_hist.resize(n_bins);
	HIP_CHECK(hipMemcpyAsync(T.occ_hist.data(), d_hist.p, n_bins * 8, hipMemcpyDeviceToHost, stream));
	HIP_CHECK(hipStreamSynchronize(stream));
	fi.bucket_bits = T.bucket_bits, fi.key_shift = T.key_shift;
	T.make_slots(stream);
	return n_keys;
}

__global__ void __launch_bounds__(256) idx_make_slots_kernel(const uint64_t *keys, const uint32_t *val_off, uint64_t n_keys, IdxSlot *slots)
{
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_keys; i += stride) {
		IdxSlot s;
		s.key = keys[i], s.off = val_off[i], s.cnt = val_off[i + 1] - val_off[i];
		slots[i] = s;
	}
}
__global__ void __launch_bounds__(256) idx_make_first_kernel(const uint32_t *bucket_start, const IdxSlot *slots, uint64_t n_buckets, IdxSlot *first)
{
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_buckets; b += stride) {
		const uint32_t s = bucket_start[b], e = bucket_start[b + 1];
		IdxSlot f;
		f.key = kIdxNoKey, f.off = 0, f.cnt = 0;
		if (s < e) { f = slots[s]; if (e - s > 1) f.cnt |= kIdxMoreKeys; }
		first[b] = f;
	}
}
void DeviceIndexTables::make_slots(hipStream_t stream)
{
	slots.ensure(n_keys + 1, 1.0);
	if (n_keys) hipLaunchKernelGGL(idx_make_slots_kernel, dim3((unsigned)std::min<uint64_t>((n_keys + 255) / 256, 16384)), dim3(256), 0, stream, keys.p, val_off.p, n_keys, slots.p);
	const uint64_t n_buckets = 1ull << bucket_bits;
	first.ensure(n_buckets + 1, 1.0);
	hipLaunchKernelGGL(idx_make_first_kernel, dim3((unsigned)std::min<uint64_t>((n_buckets + 255) / 256, 16384)), dim3(256), 0, stream, bucket_start.p, slots.p, n_buckets, first.p);
	HIP_CHECK(hipGetLastError());
	stream_wait(stream);
}

void DeviceIndexTables::upload(const FlatIndex &fi, hipStream_t stream)
{
	auto up32 = [&](DevBuf<uint32_t> &d, const std::vector<uint32_t> &h) { d.ensure(h.size() + 1, 1.0); if (!h.empty()) HIP_CHECK(hipMemcpyAsync(d.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, stream)); };
	auto up64 = [&](DevBuf<uint64_t> &d, const std::vector<uint64_t> &h) { d.ensure(h.size() + 1, 1.0); if (!h.empty()) HIP_CHECK(hipMemcpyAsync(d.p, h.data(), h.size() * 8, hipMemcpyHostToDevice, stream)); };
	up32(bucket_start, fi.bucket_start), up32(val_off, fi.val_off), up64(keys, fi.keys), up64(pos, fi.pos);
	const size_t s_words = (fi.sum_len + 7) / 8;
	S.ensure(s_words + 1, 1.0);
	if (s_words && fi.S) HIP_CHECK(hipMemcpyAsync(S.p, fi.S, s_words * 4, hipMemcpyHostToDevice, stream)); // an index without sequence (MM_I_NO_SEQ) only serves chain-level mapping
	HIP_CHECK(hipStreamSynchronize(stream));
	n_keys = fi.keys.size(), n_pos = fi.pos.size(), bucket_bits = fi.bucket_bits, key_shift = fi.key_shift;
	occ_hist.assign(1 << 16, 0);
	for (size_t i = 0; i < fi.keys.size(); ++i) { uint32_t c = fi.val_off[i + 1] - fi.val_off[i]; ++occ_hist[c < occ_hist.size() ? c : occ_hist.size() - 1]; }
	make_slots(stream);
}

void DeviceIndexTables::clone_from(const DeviceIndexTables &src, int src_device, int dst_device)
{
	n_keys = src.n_keys, n_pos = src.n_pos, bucket_bits = src.bucket_bits, key_shift = src.key_shift, occ_hist = src.occ_hist;
	auto cp = [&](void *dst, const void *from, size_t bytes) { if (bytes) HIP_CHECK(hipMemcpyPeer(dst, dst_device, from, src_device, bytes)); };
	bucket_start.ensure(((size_t)1 << bucket_bits) + 2, 1.0), cp(bucket_start.p, src.bucket_start.p, (((size_t)1 << bucket_bits) + 1) * 4);
	keys.ensure(n_keys + 1, 1.0), cp(keys.p, src.keys.p, n_keys * 8);
	val_off.ensure(n_keys + 2, 1.0), cp(val_off.p, src.val_off.p, (n_keys + 1) * 4);
	pos.ensure(n_pos + 1, 1.0), cp(pos.p, src.pos.p, n_pos * 8);
	const size_t s_words = src.S.cap; // the packed reference as allocated (its exact length lives in the host index)
	S.ensure(s_words + 1, 1.0), cp(S.p, src.S.p, s_words * 4);
	slots.ensure(n_keys + 1, 1.0), cp(slots.p, src.slots.p, n_keys * sizeof(IdxSlot));
	first.ensure(((size_t)1 << bucket_bits) + 1, 1.0), cp(first.p, src.first.p, ((size_t)1 << bucket_bits) * sizeof(IdxSlot));
	HIP_CHECK(hipDeviceSynchronize());
}

int32_t DeviceIndexTables::cal_max_occ(float f) const
{
	if (f <= 0.f || n_keys == 0) return INT32_MAX;
	const uint64_t kk = (uint32_t)((1. - f) * n_keys); // 0-based rank of the wanted occurrence count
	uint64_t acc = 0;
	for (size_t c = 0; c < occ_hist.size(); ++c) {
		acc += occ_hist[c];
		if (acc > kk) {
			if (c + 1 == occ_hist.size()) throw std::runtime_error("[mm2amd] occurrence count beyond histogram range");
			return (int32_t)c + 1;
		}
	}
	return INT32_MAX;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// .mmi files: mm_idx_dump / mm_idx_load (index.c:475-569) from and to the flat device tables.
//
// The file keeps one record per reference bucket (the low b bits of the hash), n | p[n] | size | pairs[size]: p holds the position lists of
// the keys that occur more than once, pairs one (key, value) per distinct key -- key = hash >> b << 1 | single, value = the position of a
// single occurrence or start_p << 32 | count.  The flat tables are sorted by the whole hash, i.e. by its HIGH bits first: a bucket's keys
// are spread evenly over keys[], and so are their position runs over pos[].
//
//   dump: a stable sort of (hash, key index) by the low b bits puts the keys in (bucket, ascending hash) order -- the order worker_post
//         (index.c:239-271) lays p out in.  With pcum = the exclusive sum of cnt > 1 ? cnt : 0 over the keys in that order, bucket bk's
//         record starts at word 2 bk + 2 pcum[first key] + 4 (first key): no second scan.  idx_serialise_kernel then writes the image, one
//         thread per 32-bit word of output, a chunk of whole buckets at a time; the chunks leave through two pinned buffers, the copy of one
//         beside the fwrite of the other.
//   load: the bucket section comes in through the same two buffers; idx_unpack_pairs_kernel (one thread per pair) turns it back into
//         (hash, position) pairs, checking every start_p + count against the bucket's n; one stable sort over the 2k hash bits and step 4 of
//         the build (tables_from_sorted) follow.
// ---------------------------------------------------------------------------------------------------------------------------------------
IdxIoStats &idx_io_stats() { static IdxIoStats s; return s; }

static size_t idx_io_chunk_bytes()
{
	// 64 MiB: a chunk's copy stays well below its fwrite, two pinned buffers stay at 128 MiB (not yet measured against other sizes).
	// MM2AMD_IDX_IO_CHUNK: tests force many chunks on small inputs.
	const char *e = getenv("MM2AMD_IDX_IO_CHUNK");
	long long v = e ? atoll(e) : 0;
	if (v <= 0) v = 64ll << 20;
	if (v < 64) v = 64;
	return (size_t)v & ~(size_t)7;
}

static void event_wait(hipEvent_t ev) // as stream_wait: poll between short sleeps instead of spinning in the runtime
{
	long ns = 20000;
	for (int it = 0;; ++it) {
		const hipError_t e = hipEventQuery(ev);
		if (e == hipSuccess) return;
		if (e != hipErrorNotReady) HIP_CHECK(e);
		if (it < 4) continue;
		timespec ts = { 0, ns };
		nanosleep(&ts, nullptr);
		if (ns < 500000) ns += ns / 2;
	}
}

// the two pinned chunks and their device twins; events: [i] the copy of buffer i is done, t*: timing
struct IdxIoBuffers {
	uint32_t *pin[2] = { nullptr, nullptr }, *dev[2] = { nullptr, nullptr };
	hipEvent_t done[2] = { nullptr, nullptr }, t0[2] = { nullptr, nullptr }, t1[2] = { nullptr, nullptr }, t2[2] = { nullptr, nullptr };
	void alloc(size_t bytes)
	{
		for (int i = 0; i < 2; ++i) {
			HIP_CHECK(hipHostMalloc((void **)&pin[i], bytes + 16, hipHostMallocDefault));
			HIP_CHECK(hipMalloc((void **)&dev[i], bytes + 16));
			HIP_CHECK(hipEventCreate(&done[i])), HIP_CHECK(hipEventCreate(&t0[i])), HIP_CHECK(hipEventCreate(&t1[i])), HIP_CHECK(hipEventCreate(&t2[i]));
		}
	}
	~IdxIoBuffers()
	{
		for (int i = 0; i < 2; ++i) {
			if (pin[i]) (void)hipHostFree(pin[i]);
			if (dev[i]) (void)hipFree(dev[i]);
			for (hipEvent_t e : { done[i], t0[i], t1[i], t2[i] }) if (e) (void)hipEventDestroy(e);
		}
	}
};

static double wall_ms() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }

// ---- dump ----

__global__ void __launch_bounds__(256) idx_dump_iota_kernel(const uint64_t *keys, uint64_t n_keys, uint64_t *hs, uint64_t *kidx)
{
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_keys; i += stride) hs[i] = keys[i], kidx[i] = i;
}

// per key, in file order: how often it occurs, where its positions start in pos[], and what it adds to its bucket's p array
__global__ void __launch_bounds__(256) idx_dump_gather_kernel(const uint64_t *kidx, const uint32_t *val_off, uint64_t n_keys, uint32_t *cnt, uint32_t *voff, uint32_t *contrib)
{
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_keys; i += stride) {
		const uint64_t id = kidx[i];
		const uint32_t o = val_off[id], c = val_off[id + 1] - o;
		cnt[i] = c, voff[i] = o, contrib[i] = c > 1 ? c : 0;
	}
}

// bk_key[bk] = the first key (file order) of bucket bk, bk_p[bk] = pcum there; nb + 1 entries each
__global__ void __launch_bounds__(256) idx_dump_buckets_kernel(const uint64_t *hs, uint64_t n_keys, uint64_t mask, uint64_t nb, const uint32_t *pcum, uint32_t *bk_key, uint32_t *bk_p)
{
	const uint64_t bk = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (bk > nb) return;
	uint64_t lo = 0, hi = n_keys;
	while (lo < hi) {
		const uint64_t mid = (lo + hi) >> 1;
		if ((hs[mid] & mask) < bk) lo = mid + 1; else hi = mid;
	}
	bk_key[bk] = (uint32_t)lo, bk_p[bk] = pcum[lo];
}

__device__ __forceinline__ uint64_t idx_rec_word(const uint32_t *bk_key, const uint32_t *bk_p, uint64_t bk) { return 2 * bk + 2 * (uint64_t)bk_p[bk] + 4 * (uint64_t)bk_key[bk]; }

// the last bucket in [lo, hi] whose record starts at or before word g
__device__ __forceinline__ uint32_t idx_rec_find(const uint32_t *bk_key, const uint32_t *bk_p, uint32_t lo, uint32_t hi, uint64_t g)
{
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo + 1) / 2;
		if (idx_rec_word(bk_key, bk_p, mid) <= g) lo = mid; else hi = mid - 1;
	}
	return lo;
}

// Words [w0, w0 + n_words) of the bucket section's image, which belong to buckets [bk0, bk1): one thread per word, so that a key of 10^5
// positions costs what 10^5 keys of one do and every store of a wavefront is one contiguous 256 bytes.  The 8-byte items sit on odd word
// boundaries inside a record (n is one word), hence words.  A block first brackets the buckets its 256 words fall into -- one at the size
// of a real index, hundreds where most buckets are empty --, then each thread finds its own among them.
__global__ void __launch_bounds__(256) idx_serialise_kernel(const uint64_t *hs, const uint32_t *cnt, const uint32_t *voff, const uint32_t *pcum, const uint64_t *pos,
                                                            const uint32_t *bk_key, const uint32_t *bk_p, uint32_t bk0, uint32_t bk1, uint64_t w0, uint64_t n_words, int b, uint32_t *img)
{
	__shared__ uint32_t s_bk[2];
	const uint64_t t0 = (uint64_t)blockIdx.x * 256;
	if (threadIdx.x < 2) {
		uint64_t g = t0 + (threadIdx.x ? 255 : 0);
		if (g >= n_words) g = n_words - 1;
		s_bk[threadIdx.x] = idx_rec_find(bk_key, bk_p, bk0, bk1 - 1, w0 + g);
	}
	__syncthreads();
	const uint64_t t = t0 + threadIdx.x;
	if (t >= n_words) return;
	const uint64_t g = w0 + t;
	const uint32_t bk = idx_rec_find(bk_key, bk_p, s_bk[0], s_bk[1], g);
	const uint32_t k0 = bk_key[bk], k1 = bk_key[bk + 1], p0 = bk_p[bk];
	const uint32_t n = bk_p[bk + 1] - p0, size = k1 - k0;
	const uint64_t r = g - idx_rec_word(bk_key, bk_p, bk);
	const uint32_t *pos32 = (const uint32_t *)pos;
	uint32_t out;
	if (r == 0) out = n;
	else if (r <= 2 * (uint64_t)n) { // p: the last key at or before this entry owns it (keys that add nothing share their successor's pcum)
		const uint32_t P = p0 + (uint32_t)((r - 1) >> 1);
		uint32_t lo = k0, hi = k1 - 1;
		while (lo < hi) {
			const uint32_t mid = lo + (hi - lo + 1) / 2;
			if (pcum[mid] <= P) lo = mid; else hi = mid - 1;
		}
		out = pos32[2 * ((uint64_t)voff[lo] + (P - pcum[lo])) + ((r - 1) & 1)];
	} else if (r == 2 * (uint64_t)n + 1) out = size;
	else {
		const uint64_t q = r - (2 * (uint64_t)n + 2);
		const uint32_t i = k0 + (uint32_t)(q >> 2), c = cnt[i];
		const int sel = (int)(q & 3);
		if (sel < 2) { const uint64_t key = hs[i] >> b << 1 | (c == 1 ? 1 : 0); out = (uint32_t)(key >> (sel << 5)); }
		else if (c == 1) out = pos32[2 * (uint64_t)voff[i] + (sel & 1)];
		else out = sel == 2 ? c : pcum[i] - p0;
	}
	img[t] = out;
}

static void write_all(FILE *fp, const void *p, size_t bytes)
{
	if (bytes && fwrite(p, 1, bytes, fp) != bytes) throw IdxIoError(std::string("[mm2amd] index dump: write failed: ") + strerror(errno));
}

void DeviceIndexBuilder::dump(const FlatIndex &fi, const DeviceIndexTables &T, FILE *fp, int b, bool no_seq, hipStream_t stream)
{
	IdxIoStats &st = idx_io_stats();
	st = IdxIoStats();
	const double wall0 = wall_ms();
	if (b <= 0) b = 14;
	if (b > 2 * fi.k || b > 28) throw std::invalid_argument("[mm2amd] index dump: bucket_bits must be in [1, 2k] and at most 28");
	if (!no_seq && !fi.S) throw std::invalid_argument("[mm2amd] index dump: the index has no sequence (pass MM2AMD_DUMP_NO_SEQ)");
	for (const std::string &nm : fi.names)
		if (nm.size() > 255) throw std::invalid_argument("[mm2amd] index dump: sequence name longer than 255 bytes: " + nm.substr(0, 32) + "...");
	const uint64_t n_keys = T.n_keys, nb = 1ull << b;
	// 1. regroup: keys in (bucket, ascending hash) order, their counts, the running p offsets, the buckets' first keys
	hipEvent_t e0, e1;
	HIP_CHECK(hipEventCreate(&e0)), HIP_CHECK(hipEventCreate(&e1));
	struct EvGuard { hipEvent_t a, b; ~EvGuard() { (void)hipEventDestroy(a), (void)hipEventDestroy(b); } } evg{e0, e1};
	HIP_CHECK(hipEventRecord(e0, stream));
	DevBuf<uint64_t> d_hs, d_kidx, d_hs2, d_kidx2;
	DevBuf<uint32_t> d_cnt, d_voff, d_pcum, d_bk_key, d_bk_p;
	d_hs.ensure(n_keys + 1, 1.0), d_kidx.ensure(n_keys + 1, 1.0), d_hs2.ensure(n_keys + 1, 1.0), d_kidx2.ensure(n_keys + 1, 1.0);
	const dim3 kgrid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_keys + 255) / 256, 16384)));
	if (n_keys) {
		hipLaunchKernelGGL(idx_dump_iota_kernel, kgrid, dim3(256), 0, stream, (const uint64_t *)T.keys.p, n_keys, d_hs.p, d_kidx.p);
		HIP_CHECK(hipGetLastError());
		if (device_sort_pairs_u64(d_hs.p, d_kidx.p, d_hs2.p, d_kidx2.p, n_keys, b, stream) == 1)
			std::swap(d_hs.p, d_hs2.p), std::swap(d_hs.cap, d_hs2.cap), std::swap(d_kidx.p, d_kidx2.p), std::swap(d_kidx.cap, d_kidx2.cap);
	}
	d_hs2.release(), d_kidx2.release();
	d_cnt.ensure(n_keys + 1, 1.0), d_voff.ensure(n_keys + 1, 1.0), d_pcum.ensure(n_keys + 2, 1.0);
	if (n_keys) {
		hipLaunchKernelGGL(idx_dump_gather_kernel, kgrid, dim3(256), 0, stream, (const uint64_t *)d_kidx.p, (const uint32_t *)T.val_off.p, n_keys, d_cnt.p, d_voff.p, d_pcum.p);
		HIP_CHECK(hipGetLastError());
		device_exclusive_sum_u32(d_pcum.p, d_pcum.p, n_keys, stream);
	} else HIP_CHECK(hipMemsetAsync(d_pcum.p, 0, 4, stream));
	d_kidx.release();
	d_bk_key.ensure(nb + 2, 1.0), d_bk_p.ensure(nb + 2, 1.0);
	hipLaunchKernelGGL(idx_dump_buckets_kernel, dim3((unsigned)((nb + 1 + 255) / 256)), dim3(256), 0, stream, (const uint64_t *)d_hs.p, n_keys, nb - 1, nb, (const uint32_t *)d_pcum.p, d_bk_key.p, d_bk_p.p);
	HIP_CHECK(hipGetLastError());
	std::vector<uint32_t> bk_key(nb + 1), bk_p(nb + 1);
	HIP_CHECK(hipMemcpyAsync(bk_key.data(), d_bk_key.p, (nb + 1) * 4, hipMemcpyDeviceToHost, stream));
	HIP_CHECK(hipMemcpyAsync(bk_p.data(), d_bk_p.p, (nb + 1) * 4, hipMemcpyDeviceToHost, stream));
	HIP_CHECK(hipEventRecord(e1, stream));
	stream_wait(stream);
	float ms = 0;
	HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
	st.regroup_ms = ms;
	auto rec_word = [&](uint64_t bk) { return 2 * bk + 2 * (uint64_t)bk_p[bk] + 4 * (uint64_t)bk_key[bk]; };
	uint64_t max_rec = 0;
	for (uint64_t bk = 0; bk < nb; ++bk) {
		if (bk_p[bk + 1] - bk_p[bk] >= (1u << 31)) throw std::invalid_argument("[mm2amd] index dump: a bucket holds 2^31 positions or more; use more bucket bits");
		max_rec = std::max(max_rec, rec_word(bk + 1) - rec_word(bk));
	}
	const uint64_t total_words = rec_word(nb);
	// 2. header and names
	const double f0 = wall_ms();
	uint32_t x[5] = { (uint32_t)fi.w, (uint32_t)fi.k, (uint32_t)b, fi.n_seq, (uint32_t)(no_seq ? fi.flag | ref::I_NO_SEQ : fi.flag & ~ref::I_NO_SEQ) };
	write_all(fp, "MMI\2", 4), write_all(fp, x, 20);
	for (uint32_t i = 0; i < fi.n_seq; ++i) {
		const uint8_t l = (fi.flag & ref::I_NO_NAME) ? 0 : (uint8_t)fi.names[i].size();
		write_all(fp, &l, 1), write_all(fp, fi.names[i].data(), l), write_all(fp, &fi.seq_len[i], 4);
	}
	st.file_ms += wall_ms() - f0;
	// 3. the bucket section, in chunks of whole buckets: serialise + copy chunk c while chunk c - 1 is written
	const uint64_t chunk_words = std::max<uint64_t>(idx_io_chunk_bytes() / 4, 2);
	IdxIoBuffers B;
	B.alloc((size_t)std::min(total_words, std::max(chunk_words, max_rec)) * 4);
	struct Chunk { uint64_t bk0, bk1; };
	std::vector<Chunk> chunks;
	for (uint64_t bk = 0; bk < nb;) {
		uint64_t e = bk + 1;
		while (e < nb && rec_word(e + 1) - rec_word(bk) <= chunk_words) ++e;
		chunks.push_back(Chunk{bk, e});
		bk = e;
	}
	st.n_chunks = (double)chunks.size(), st.chunk_bytes = (double)chunk_words * 4, st.image_bytes = (double)total_words * 4;
	auto finish = [&](size_t c) { // chunk c has arrived in its pinned buffer: time it, write it
		const int s = (int)(c & 1);
		event_wait(B.done[s]);
		float a = 0, d = 0;
		HIP_CHECK(hipEventElapsedTime(&a, B.t0[s], B.t1[s])), HIP_CHECK(hipEventElapsedTime(&d, B.t1[s], B.t2[s]));
		st.kernel_ms += a, st.copy_ms += d;
		const double w0 = wall_ms();
		write_all(fp, B.pin[s], (size_t)(rec_word(chunks[c].bk1) - rec_word(chunks[c].bk0)) * 4);
		st.file_ms += wall_ms() - w0;
	};
	for (size_t c = 0; c < chunks.size(); ++c) {
		const int s = (int)(c & 1);
		const uint64_t w0 = rec_word(chunks[c].bk0), nw = rec_word(chunks[c].bk1) - w0;
		HIP_CHECK(hipEventRecord(B.t0[s], stream));
		hipLaunchKernelGGL(idx_serialise_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, stream, (const uint64_t *)d_hs.p, (const uint32_t *)d_cnt.p, (const uint32_t *)d_voff.p,
		                   (const uint32_t *)d_pcum.p, (const uint64_t *)T.pos.p, (const uint32_t *)d_bk_key.p, (const uint32_t *)d_bk_p.p, (uint32_t)chunks[c].bk0, (uint32_t)chunks[c].bk1, w0, nw, b, B.dev[s]);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipEventRecord(B.t1[s], stream));
		HIP_CHECK(hipMemcpyAsync(B.pin[s], B.dev[s], nw * 4, hipMemcpyDeviceToHost, stream));
		HIP_CHECK(hipEventRecord(B.t2[s], stream));
		HIP_CHECK(hipEventRecord(B.done[s], stream));
		if (c > 0) finish(c - 1);
	}
	if (!chunks.empty()) finish(chunks.size() - 1);
	// 4. the packed sequence
	const double s0 = wall_ms();
	if (!no_seq) write_all(fp, fi.S, (size_t)((fi.sum_len + 7) / 8) * 4);
	if (fflush(fp) != 0) throw IdxIoError(std::string("[mm2amd] index dump: write failed: ") + strerror(errno));
	st.seq_ms = wall_ms() - s0, st.file_ms += st.seq_ms;
	const long at = ftell(fp);
	st.file_bytes = at > 0 ? (double)at : 0;
	st.total_ms = wall_ms() - wall0;
}

// ---- load ----

struct MmiBucket { uint64_t p_word, pair_word, out_p, pair_base; uint32_t n, size, bucket, pad; }; // word offsets within the bucket section; out_p: n of the buckets before
struct MmiLong { uint64_t hash, src_word, dst; uint32_t cnt, n_seq; };                          // a position run too long for one thread
struct MmiCounters { unsigned long long n_single, sum_cnt; uint32_t err, n_long; };
enum { MMI_E_RANGE = 1, MMI_E_ZERO = 2, MMI_E_ORDER = 4, MMI_E_KEY = 8, MMI_E_POS = 16, MMI_E_GAP = 32 };
constexpr uint32_t kMmiShortRun = 32;

__device__ __forceinline__ uint64_t mmi_u64(const uint32_t *img, uint64_t word) { return (uint64_t)img[word] | (uint64_t)img[word + 1] << 32; }
__device__ __forceinline__ bool mmi_pos_ok(uint64_t p, const uint32_t *seq_len, uint32_t n_seq) { const uint32_t rid = (uint32_t)(p >> 32); return rid < n_seq && ((uint32_t)p >> 1) < seq_len[rid]; }

// One thread per (key, value) pair of the chunk's buckets desc[d0, d1).  A single occurrence goes to the end of the output (its rank among the singles
// comes from a counter bumped once per wavefront: any order will do, one position per key); a key of several owns p[start_p, start_p + cnt) of its
// bucket, which lands at out[out_p + start_p ...] -- file order, so ascending within the key.  Runs of more than kMmiShortRun are queued for
// idx_unpack_long_kernel.  Everything read from the file is checked before it is used as an index.
__global__ void __launch_bounds__(256) idx_unpack_pairs_kernel(const MmiBucket *desc, uint32_t d0, uint32_t d1, uint64_t n_pairs, uint64_t chunk_word0, const uint32_t *img, int b, int key_bits,
                                                               const uint32_t *seq_len, uint32_t n_seq, uint64_t single0, uint64_t *out_hash, uint64_t *out_pos, MmiCounters *ctr, MmiLong *longs, uint32_t long_cap)
{
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = t < n_pairs;
	const int lane = threadIdx.x & 63;
	bool single = false;
	uint64_t hash = 0, val = 0;
	uint32_t err = 0, cnt = 0;
	if (live) {
		const uint64_t tp = desc[d0].pair_base + t;
		uint32_t lo = d0, hi = d1 - 1; // the last bucket whose pairs start at or before tp (empty buckets have no descriptor)
		while (lo < hi) {
			const uint32_t mid = lo + (hi - lo + 1) / 2;
			if (desc[mid].pair_base <= tp) lo = mid; else hi = mid - 1;
		}
		const MmiBucket B = desc[lo];
		const uint64_t pw = B.pair_word - chunk_word0 + 4 * (tp - B.pair_base);
		const uint64_t key = mmi_u64(img, pw);
		val = mmi_u64(img, pw + 2);
		if (key_bits < 63 && (key >> 1 >> key_bits) != 0) err |= MMI_E_KEY;
		hash = key >> 1 << b | B.bucket;
		if (key & 1) {
			single = true;
			if (!mmi_pos_ok(val, seq_len, n_seq)) err |= MMI_E_POS, single = false;
		} else {
			const uint64_t start = val >> 32;
			cnt = (uint32_t)val;
			if (cnt == 0) err |= MMI_E_ZERO;
			else if (start + cnt > B.n) err |= MMI_E_RANGE, cnt = 0;
			else if (cnt > kMmiShortRun) {
				const uint32_t at = atomicAdd(&ctr->n_long, 1u);
				if (at < long_cap) { MmiLong L; L.hash = hash, L.src_word = B.p_word - chunk_word0 + 2 * start, L.dst = B.out_p + start, L.cnt = cnt, L.n_seq = n_seq; longs[at] = L; }
				else err |= MMI_E_RANGE; // (more long runs than the chunk's p entries allow: the runs overlap)
			} else {
				const uint64_t src = B.p_word - chunk_word0 + 2 * start, dst = B.out_p + start;
				uint64_t prev = 0;
				for (uint32_t j = 0; j < cnt; ++j) {
					const uint64_t p = mmi_u64(img, src + 2 * j);
					if (j && p <= prev) err |= MMI_E_ORDER;
					if (!mmi_pos_ok(p, seq_len, n_seq)) err |= MMI_E_POS;
					out_hash[dst + j] = hash, out_pos[dst + j] = p;
					prev = p;
				}
			}
		}
	}
	// the singles' places, and the sum of the counts (which must come to the sum of the buckets' n)
	const unsigned long long bal = __ballot(single);
	unsigned long long base = 0;
	const int leader = bal ? __ffsll((long long)bal) - 1 : 0;
	if (bal && lane == leader) base = atomicAdd(&ctr->n_single, (unsigned long long)__popcll(bal));
	base = __shfl(base, leader);
	if (single) {
		const uint64_t at = single0 + base + (uint64_t)__popcll(bal & ((1ull << lane) - 1));
		out_hash[at] = hash, out_pos[at] = val;
	}
	unsigned long long sum = cnt;
	for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
	if (lane == 0 && sum) atomicAdd(&ctr->sum_cnt, sum);
	if (err) atomicOr(&ctr->err, err);
}

// one block per queued run
__global__ void __launch_bounds__(256) idx_unpack_long_kernel(const MmiLong *longs, const MmiCounters *ctr, uint32_t long_cap, const uint32_t *img, const uint32_t *seq_len, uint64_t *out_hash, uint64_t *out_pos, uint32_t *err_out)
{
	const uint32_t n_long = ctr->n_long < long_cap ? ctr->n_long : long_cap;
	uint32_t err = 0;
	for (uint32_t it = blockIdx.x; it < n_long; it += gridDim.x) {
		const MmiLong L = longs[it];
		for (uint32_t j = threadIdx.x; j < L.cnt; j += blockDim.x) {
			const uint64_t p = mmi_u64(img, L.src_word + 2 * (uint64_t)j);
			if (j && p <= mmi_u64(img, L.src_word + 2 * (uint64_t)(j - 1))) err |= MMI_E_ORDER;
			if (!mmi_pos_ok(p, seq_len, L.n_seq)) err |= MMI_E_POS;
			out_hash[L.dst + j] = L.hash, out_pos[L.dst + j] = p;
		}
	}
	if (err) atomicOr(err_out, err);
}

// a p entry no key owns keeps the fill pattern
__global__ void __launch_bounds__(256) idx_unpack_gaps_kernel(const uint64_t *out_hash, uint64_t n, uint32_t *err_out)
{
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	bool gap = false;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) gap |= out_hash[i] == ~0ull;
	if (gap) atomicOr(err_out, (uint32_t)MMI_E_GAP);
}

namespace {
struct MmiLayout { // what the header, the name table and the bucket headers of one part say
	uint32_t w = 0, k = 0, b = 0, n_seq = 0, flag = 0;
	std::vector<std::string> names;
	std::vector<uint32_t> lens;
	uint64_t sum_len = 0, sec_off = 0, sec_bytes = 0, s_off = 0, end_off = 0, total_n = 0, total_size = 0;
	std::vector<uint32_t> bn, bsize;
};
[[noreturn]] void mmi_corrupt(const std::string &what) { throw std::invalid_argument("[mm2amd] index load: " + what); }
void pread_all(int fd, void *dst, size_t bytes, uint64_t off)
{
	char *p = (char *)dst;
	while (bytes) {
		const ssize_t r = pread(fd, p, bytes, (off_t)off);
		if (r < 0) { if (errno == EINTR) continue; throw IdxIoError(std::string("[mm2amd] index load: read failed: ") + strerror(errno)); }
		if (r == 0) mmi_corrupt("truncated file");
		p += r, off += (uint64_t)r, bytes -= (size_t)r;
	}
}
// every count is held against the bytes that remain before anything is sized by it
void mmi_layout(int fd, uint64_t file_size, uint64_t off, bool keep_names, MmiLayout &L)
{
	auto need = [&](uint64_t at, uint64_t bytes, const char *what) { if (at > file_size || bytes > file_size - at) mmi_corrupt(std::string("truncated file (") + what + ")"); };
	if (off >= file_size) mmi_corrupt("no such part");
	need(off, 24, "header");
	char magic[4];
	uint32_t x[5];
	pread_all(fd, magic, 4, off);
	if (memcmp(magic, "MMI\2", 4) != 0) mmi_corrupt("not a minimap2 index (bad magic)");
	pread_all(fd, x, 20, off + 4);
	L.w = x[0], L.k = x[1], L.b = x[2], L.n_seq = x[3], L.flag = x[4];
	if (L.w == 0 || L.w >= 256 || L.k == 0 || L.k > 28) mmi_corrupt("need 0<w<256 and 0<k<=28");
	if (L.b == 0 || L.b > 28 || L.b > 2 * L.k) mmi_corrupt("bucket bits outside [1, min(2k, 28)]");
	uint64_t at = off + 24;
	need(at, (uint64_t)L.n_seq * 5, "name table");
	L.lens.resize(L.n_seq);
	if (keep_names) L.names.resize(L.n_seq);
	{ // the name table through a sliding window
		std::vector<char> buf;
		uint64_t buf_off = at;
		auto fetch = [&](uint64_t pos, size_t bytes) -> const char * {
			if (pos < buf_off || pos + bytes > buf_off + buf.size()) {
				const uint64_t want = std::min<uint64_t>(file_size - pos, std::max<uint64_t>(bytes, 1 << 20));
				buf.resize((size_t)want);
				pread_all(fd, buf.data(), (size_t)want, pos);
				buf_off = pos;
			}
			return buf.data() + (pos - buf_off);
		};
		for (uint32_t i = 0; i < L.n_seq; ++i) {
			need(at, 1, "name table");
			const uint8_t l = (uint8_t)*fetch(at, 1);
			need(at + 1, (uint64_t)l + 4, "name table");
			const char *p = fetch(at + 1, (size_t)l + 4);
			if (keep_names) L.names[i].assign(p, l);
			memcpy(&L.lens[i], p + l, 4);
			if (L.lens[i] >= (1u << 31)) mmi_corrupt("a sequence of 2^31 bases or more");
			L.sum_len += L.lens[i];
			at += 1 + (uint64_t)l + 4;
		}
	}
	L.sec_off = at;
	const uint64_t nb = 1ull << L.b;
	need(at, nb * 8, "bucket section");
	L.bn.resize(nb), L.bsize.resize(nb);
	for (uint64_t bk = 0; bk < nb; ++bk) {
		uint32_t n, size;
		need(at, 4, "bucket header");
		pread_all(fd, &n, 4, at);
		if (n >= (1u << 31)) mmi_corrupt("negative position count in a bucket");
		need(at + 4, 8 * (uint64_t)n + 4, "position array");
		pread_all(fd, &size, 4, at + 4 + 8 * (uint64_t)n);
		need(at + 8 + 8 * (uint64_t)n, 16 * (uint64_t)size, "hash table");
		if (n && !size) mmi_corrupt("a bucket with positions and no keys");
		L.bn[bk] = n, L.bsize[bk] = size, L.total_n += n, L.total_size += size;
		at += 8 + 8 * (uint64_t)n + 16 * (uint64_t)size;
	}
	L.sec_bytes = at - L.sec_off, L.s_off = at;
	if (!(L.flag & ref::I_NO_SEQ)) { need(at, (L.sum_len + 7) / 8 * 4, "sequence"); at += (L.sum_len + 7) / 8 * 4; }
	L.end_off = at;
}
} // namespace

uint64_t DeviceIndexBuilder::skip_part(int fd, uint64_t file_size, uint64_t off)
{
	MmiLayout L;
	mmi_layout(fd, file_size, off, false, L);
	return L.end_off;
}

uint64_t DeviceIndexBuilder::load(FlatIndex &fi, DeviceIndexTables &T, int fd, uint64_t file_size, uint64_t off, hipStream_t stream)
{
	IdxIoStats &st = idx_io_stats();
	st = IdxIoStats();
	const double wall0 = wall_ms();
	MmiLayout L;
	mmi_layout(fd, file_size, off, true, L);
	st.file_ms += wall_ms() - wall0;
	fi.k = (int)L.k, fi.w = (int)L.w, fi.flag = (int)L.flag, fi.n_seq = L.n_seq, fi.n_alt = 0;
	fi.names.swap(L.names), fi.seq_len.swap(L.lens), fi.seq_off.resize(L.n_seq);
	if (fi.flag & ref::I_NO_NAME) for (std::string &nm : fi.names) nm.clear();
	uint64_t total = 0;
	for (uint32_t i = 0; i < L.n_seq; ++i) fi.seq_off[i] = total, total += fi.seq_len[i];
	fi.sum_len = total;
	const uint64_t nb = 1ull << L.b, cap = L.total_n + L.total_size; // every key adds its run, or one position
	if (L.total_n >= (1ull << 32)) mmi_corrupt("more than 2^32 - 1 positions in one part: split the reference");
	// descriptors of the buckets that hold keys
	std::vector<MmiBucket> desc;
	std::vector<uint64_t> rec_word(nb + 1); // where each bucket's record starts in the section (words)
	{
		uint64_t word = 0, out_p = 0, pair_base = 0;
		for (uint64_t bk = 0; bk < nb; ++bk) {
			rec_word[bk] = word;
			if (L.bsize[bk]) {
				MmiBucket d;
				d.p_word = word + 1, d.pair_word = word + 2 + 2 * (uint64_t)L.bn[bk], d.out_p = out_p, d.pair_base = pair_base;
				d.n = L.bn[bk], d.size = L.bsize[bk], d.bucket = (uint32_t)bk, d.pad = 0;
				desc.push_back(d);
			}
			word += 2 + 2 * (uint64_t)L.bn[bk] + 4 * (uint64_t)L.bsize[bk], out_p += L.bn[bk], pair_base += L.bsize[bk];
		}
		rec_word[nb] = word;
	}
	const uint64_t chunk_words = std::max<uint64_t>(idx_io_chunk_bytes() / 4, 2);
	struct Chunk { uint64_t bk0, bk1; uint32_t d0, d1; uint64_t n_long; }; // n_long: the most runs of more than kMmiShortRun positions its p arrays can hold
	std::vector<Chunk> chunks;
	uint64_t max_words = 0, max_long = 0;
	{
		uint32_t d = 0;
		for (uint64_t bk = 0; bk < nb;) {
			uint64_t e = bk + 1;
			while (e < nb && rec_word[e + 1] - rec_word[bk] <= chunk_words) ++e;
			Chunk c{bk, e, d, d, 0};
			uint64_t n_in = 0;
			while (c.d1 < desc.size() && desc[c.d1].bucket < e) n_in += desc[c.d1].n, ++c.d1;
			d = c.d1;
			c.n_long = n_in / (kMmiShortRun + 1);
			max_words = std::max(max_words, rec_word[e] - rec_word[bk]), max_long = std::max(max_long, c.n_long + 1);
			chunks.push_back(c);
			bk = e;
		}
	}
	if (max_long >= (1ull << 32)) mmi_corrupt("more than 2^32 - 1 positions in one part: split the reference");
	st.n_chunks = (double)chunks.size(), st.chunk_bytes = (double)chunk_words * 4, st.image_bytes = (double)L.sec_bytes, st.file_bytes = (double)(L.end_off - off);
	DevBuf<MmiBucket> d_desc;
	DevBuf<MmiLong> d_long;
	DevBuf<MmiCounters> d_ctr;
	DevBuf<uint32_t> d_seq_len;
	DevBuf<uint64_t> d_hash, d_pos, d_hash2, d_pos2;
	d_desc.ensure(desc.size() + 1, 1.0), d_long.ensure(max_long + 1, 1.0), d_ctr.ensure(1, 1.0), d_seq_len.ensure(L.n_seq + 1, 1.0);
	d_hash.ensure(cap + 1, 1.0), d_pos.ensure(cap + 1, 1.0);
	if (!desc.empty()) HIP_CHECK(hipMemcpyAsync(d_desc.p, desc.data(), desc.size() * sizeof(MmiBucket), hipMemcpyHostToDevice, stream));
	if (L.n_seq) HIP_CHECK(hipMemcpyAsync(d_seq_len.p, fi.seq_len.data(), (size_t)L.n_seq * 4, hipMemcpyHostToDevice, stream));
	HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, sizeof(MmiCounters), stream));
	if (L.total_n) HIP_CHECK(hipMemsetAsync(d_hash.p, 0xff, L.total_n * 8, stream));
	HIP_CHECK(hipStreamSynchronize(stream)); // (desc is pageable host memory)
	// the section through the two pinned buffers: read chunk c + 1 while chunk c is copied and unpacked
	IdxIoBuffers B;
	B.alloc((size_t)max_words * 4);
	const int key_bits = 2 * (int)L.k - (int)L.b;
	uint32_t *err_word = &d_ctr.p->err;
	for (size_t c = 0; c < chunks.size(); ++c) {
		const int s = (int)(c & 1);
		const Chunk &ch = chunks[c];
		const uint64_t w0 = rec_word[ch.bk0], nw = rec_word[ch.bk1] - w0;
		if (c >= 2) { // this buffer's last copy must have left it
			event_wait(B.done[s]);
			float a = 0, d = 0;
			HIP_CHECK(hipEventElapsedTime(&a, B.t0[s], B.t1[s])), HIP_CHECK(hipEventElapsedTime(&d, B.t1[s], B.t2[s]));
			st.copy_ms += a, st.kernel_ms += d;
		}
		const double r0 = wall_ms();
		pread_all(fd, B.pin[s], (size_t)nw * 4, L.sec_off + w0 * 4);
		st.file_ms += wall_ms() - r0;
		HIP_CHECK(hipEventRecord(B.t0[s], stream));
		HIP_CHECK(hipMemcpyAsync(B.dev[s], B.pin[s], nw * 4, hipMemcpyHostToDevice, stream));
		HIP_CHECK(hipEventRecord(B.t1[s], stream));
		if (ch.d1 > ch.d0) {
			const uint64_t n_pairs = desc[ch.d1 - 1].pair_base + desc[ch.d1 - 1].size - desc[ch.d0].pair_base;
			HIP_CHECK(hipMemsetAsync(&d_ctr.p->n_long, 0, 4, stream));
			hipLaunchKernelGGL(idx_unpack_pairs_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, stream, (const MmiBucket *)d_desc.p, ch.d0, ch.d1, n_pairs, w0, (const uint32_t *)B.dev[s],
			                   (int)L.b, key_bits, (const uint32_t *)d_seq_len.p, L.n_seq, L.total_n, d_hash.p, d_pos.p, d_ctr.p, d_long.p, (uint32_t)max_long);
			HIP_CHECK(hipGetLastError());
			if (ch.n_long) hipLaunchKernelGGL(idx_unpack_long_kernel, dim3((unsigned)std::min<uint64_t>(ch.n_long, 1024)), dim3(256), 0, stream, (const MmiLong *)d_long.p, (const MmiCounters *)d_ctr.p, (uint32_t)max_long, (const uint32_t *)B.dev[s],
			                   (const uint32_t *)d_seq_len.p, d_hash.p, d_pos.p, err_word);
			HIP_CHECK(hipGetLastError());
		}
		HIP_CHECK(hipEventRecord(B.t2[s], stream));
		HIP_CHECK(hipEventRecord(B.done[s], stream));
	}
	for (size_t c = chunks.size() >= 2 ? chunks.size() - 2 : 0; c < chunks.size(); ++c) {
		const int s = (int)(c & 1);
		event_wait(B.done[s]);
		float a = 0, d = 0;
		HIP_CHECK(hipEventElapsedTime(&a, B.t0[s], B.t1[s])), HIP_CHECK(hipEventElapsedTime(&d, B.t1[s], B.t2[s]));
		st.copy_ms += a, st.kernel_ms += d;
	}
	if (L.total_n) hipLaunchKernelGGL(idx_unpack_gaps_kernel, dim3((unsigned)std::min<uint64_t>((L.total_n + 255) / 256, 16384)), dim3(256), 0, stream, (const uint64_t *)d_hash.p, L.total_n, err_word);
	HIP_CHECK(hipGetLastError());
	MmiCounters ctr;
	HIP_CHECK(hipMemcpyAsync(&ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
	stream_wait(stream);
	if (ctr.err & MMI_E_KEY) mmi_corrupt("a key wider than 2k - b bits");
	if (ctr.err & MMI_E_ZERO) mmi_corrupt("a key with a position count of zero");
	if (ctr.err & MMI_E_RANGE) mmi_corrupt("a key whose positions lie beyond its bucket's array (start_p + n > bucket n)");
	if (ctr.err & MMI_E_ORDER) mmi_corrupt("a position list that is not ascending");
	if (ctr.err & MMI_E_POS) mmi_corrupt("a position outside the sequences the file names");
	if ((ctr.err & MMI_E_GAP) || ctr.sum_cnt != L.total_n) mmi_corrupt("the keys' position lists do not tile their bucket's array");
	const uint64_t n_pos = L.total_n + ctr.n_single;
	if (n_pos >= (1ull << 32)) mmi_corrupt("more than 2^32 - 1 positions in one part: split the reference");
	d_desc.release(), d_long.release();
	// one stable sort over the 2k hash bits, then step 4 of the build
	hipEvent_t e0, e1, e2;
	HIP_CHECK(hipEventCreate(&e0)), HIP_CHECK(hipEventCreate(&e1)), HIP_CHECK(hipEventCreate(&e2));
	struct EvGuard { hipEvent_t a, b, c; ~EvGuard() { (void)hipEventDestroy(a), (void)hipEventDestroy(b), (void)hipEventDestroy(c); } } evg{e0, e1, e2};
	HIP_CHECK(hipEventRecord(e0, stream));
	d_hash2.ensure(n_pos + 1, 1.0), d_pos2.ensure(n_pos + 1, 1.0);
	if (device_sort_pairs_u64(d_hash.p, d_pos.p, d_hash2.p, d_pos2.p, n_pos, 2 * (int)L.k, stream) == 1)
		std::swap(d_hash.p, d_hash2.p), std::swap(d_hash.cap, d_hash2.cap), std::swap(d_pos.p, d_pos2.p), std::swap(d_pos.cap, d_pos2.cap);
	d_hash2.release(), d_pos2.release();
	HIP_CHECK(hipEventRecord(e1, stream));
	const uint64_t n_keys = tables_from_sorted(fi, T, d_hash, d_pos, n_pos, (int)L.k, stream);
	HIP_CHECK(hipEventRecord(e2, stream));
	stream_wait(stream);
	float ms = 0;
	HIP_CHECK(hipEventElapsedTime(&ms, e0, e1)), st.sort_ms = ms;
	HIP_CHECK(hipEventElapsedTime(&ms, e1, e2)), st.tables_ms = ms;
	if (n_keys != L.total_size) mmi_corrupt("a key occurs twice in a bucket");
	// the packed sequence
	const double s0 = wall_ms();
	const uint64_t n_words = (total + 7) / 8;
	T.S.ensure(n_words + 1, 1.0);
	fi.S_own.clear(), fi.S = nullptr;
	if (!(L.flag & ref::I_NO_SEQ)) {
		fi.S_own.resize(n_words);
		pread_all(fd, fi.S_own.data(), (size_t)n_words * 4, L.s_off);
		fi.S = fi.S_own.data();
		if (n_words) HIP_CHECK(hipMemcpyAsync(T.S.p, fi.S, n_words * 4, hipMemcpyHostToDevice, stream));
	} else HIP_CHECK(hipMemsetAsync(T.S.p, 0, (n_words + 1) * 4, stream)); // (chain-level mapping only: mapper.cpp refuses base-level alignment without fi.S)
	HIP_CHECK(hipStreamSynchronize(stream));
	st.seq_ms = wall_ms() - s0, st.file_ms += st.seq_ms;
	st.total_ms = wall_ms() - wall0;
	return L.end_off;
}

} // namespace mm2amd
