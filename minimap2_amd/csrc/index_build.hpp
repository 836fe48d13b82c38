// Device-resident index tables and their construction on the GPU (index_build.hip).
#pragma once
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>
#include "hip_util.hpp"
#include "flat_index.hpp"

namespace mm2amd {

// The flat minimizer tables of flat_index.hpp living in HBM, plus the 4-bit packed reference.
// One probe record per distinct minimizer: the key, where its positions start and how many there are -- the key scan of a bucket and the count
// come out of ONE 64-byte sector (round 5; keys[] and val_off[] stay for the export and the occurrence statistics, the probes of seed_collect_kernel
// read this: bucket_start -> slot instead of bucket_start -> keys -> val_off, val_off + 1)
struct alignas(16) IdxSlot { uint64_t key; uint32_t off, cnt; };
// Round 6: one such record PER BUCKET as well -- the bucket's first key inline, its count's top bit set when the bucket holds more keys, an impossible key when it
// holds none.  A probe reads this one record first: an empty bucket, a bucket whose only key is another one, and a hit on a bucket's first key (three probes in four
// at the index' load factor of 0.65 keys per bucket) are answered by ONE sector read instead of two dependent ones (bucket_start, then the slots).
constexpr uint32_t kIdxMoreKeys = 1u << 31;
constexpr uint64_t kIdxNoKey = ~0ull; // (a minimizer key is hash << 8 | span: never all ones)

struct DeviceIndexTables {
	DevBuf<uint32_t> bucket_start, val_off, S;
	DevBuf<uint64_t> keys, pos;
	DevBuf<IdxSlot> slots, first;          // per distinct minimizer | per bucket (above)
	void make_slots(hipStream_t stream); // from keys / val_off (and bucket_start)
	uint64_t n_keys = 0, n_pos = 0;
	int bucket_bits = 0, key_shift = 0;
	std::vector<unsigned long long> occ_hist; // occ_hist[c] = number of distinct minimizers occurring c times (last bin: >=)
	int32_t cal_max_occ(float f) const;       // mm_idx_cal_max_occ (index.c:198-220) from the histogram
	void upload(const FlatIndex &fi, hipStream_t stream); // mirror host-side tables (index flattened from a reference mm_idx_t)
	void clone_from(const DeviceIndexTables &src, int src_device, int dst_device); // replica on another GPU: device-to-device copies (xGMI); the calling thread's current device must be dst_device
};

struct DeviceIndexBuilder {
	// In-memory index construction, the device counterpart of mm_idx_str (index.c:421-470) / mm_idx_gen (index.c:389-408).
	// Fills the host-side part of `fi` (names, lengths, packed S; no host hash tables) and the device tables `T`.
	static void build(FlatIndex &fi, DeviceIndexTables &T, int k, int w, int flag, int n_seq, const char *const *seqs, const uint64_t *lens,
	                  const char *const *names, hipStream_t stream);
	// Same tables from an index that already carries its packed sequence (fi.S and the sequence table set: FlatIndex::from_reference
	// without the host tables): the device part of mm_gpu_init.
	static void build_from_packed(FlatIndex &fi, DeviceIndexTables &T, hipStream_t stream);
	// One index part in the reference's MMI\2 format (mm_idx_dump, index.c:475-514), written to `fp`: the device regroups the flat
	// tables by the low b hash bits and serialises the bucket section; the host writes header, names, the section's chunks and S.
	// no_seq: an MM_I_NO_SEQ file (no S section).  Throws std::invalid_argument for what the format cannot hold, IdxIoError when a write fails.
	static void dump(const FlatIndex &fi, const DeviceIndexTables &T, FILE *fp, int b, bool no_seq, hipStream_t stream);
	// The reverse (mm_idx_load, index.c:516-569): the part that starts at file offset `off` of the file open as `fd` (`file_size`
	// bytes long).  The tables come from the file's bucket records; every count is checked against the bytes that remain before it is
	// believed.  Returns the offset the part ends at.  Throws std::invalid_argument for a corrupt file, IdxIoError when a read fails.
	static uint64_t load(FlatIndex &fi, DeviceIndexTables &T, int fd, uint64_t file_size, uint64_t off, hipStream_t stream);
	// Where the part at `off` ends, reading only its header, name table and bucket headers (the parts before the wanted one).
	static uint64_t skip_part(int fd, uint64_t file_size, uint64_t off);
private:
	static void tables_from_nt4(FlatIndex &fi, DeviceIndexTables &T, DevBuf<uint8_t> &d_nt4, hipStream_t stream);
	// step 4 of the build: distinct keys, value offsets, direct table, occurrence histogram and probe records from n_mz (hash, position)
	// pairs sorted by (hash, position); T.pos takes d_pos over.  Returns the number of distinct keys.
	static uint64_t tables_from_sorted(FlatIndex &fi, DeviceIndexTables &T, DevBuf<uint64_t> &d_hash, DevBuf<uint64_t> &d_pos, uint64_t n_mz, int k, hipStream_t stream);
};

struct IdxIoError : std::runtime_error { using std::runtime_error::runtime_error; }; // open / read / write failed (MM2AMD_EIO)
// Phase times of the last dump or load of this process (diagnostics: tools/mm2amd_index.py --json): milliseconds and bytes
struct IdxIoStats { double regroup_ms = 0, kernel_ms = 0, copy_ms = 0, file_ms = 0, sort_ms = 0, tables_ms = 0, total_ms = 0, image_bytes = 0, file_bytes = 0, n_chunks = 0, chunk_bytes = 0, seq_ms = 0; };
IdxIoStats &idx_io_stats();

} // namespace mm2amd
