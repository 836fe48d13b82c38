// fastx_lines_kernel / fastx_classify_kernel / fastx_copy_kernel: FASTA and 4-line FASTQ text into the records of kseq_read + kseq2bseq
// (kseq.h:192-232, bseq.c:65-78) on the device.  Compiled with index_build.hip; fastx.hpp has the parameters and the host's parser, DESIGN.md
// section 3h the grammar, the two buffer classes the device takes and why everything else goes to the host.
//
//   lines     workgroups take tiles of kFastxTile bytes counted from the 16-byte aligned address below the text: a lane reads one aligned 16-byte
//             vector (a partial first or last vector byte by byte, nothing outside the text) and finds its '\n' bytes.  The first pass leaves
//             the tile's count; after the exclusive sum over the tiles the second pass writes the start of the line behind every '\n'.
//   classify  one lane per line: the first byte, the payload after the CR rule, a header's name end; what the line contributes to the pool;
//             whether it violates the class (one atomicOr into state[0]); the long lines' work items.
//   copy      after the exclusive sum of the contributions.  Short class: kFastxShortLanes lanes per line write its bytes, the NULs and, for a
//             header, the record's table entry.  Long class: a workgroup per kFastxLongChunk bytes of a line of at least long_line bytes.
// No loop waits on another lane; every trip count is a line's or a chunk's length.
#pragma once
#include <hip/hip_runtime.h>
#include "hip_util.hpp"
#include "fastx.hpp"

namespace mm2amd {

__device__ __forceinline__ uint32_t fx_nl_mask(uint32_t w) // 0x80 in every byte of w that is '\n'
{
	const uint32_t x = w ^ 0x0a0a0a0au;
	return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}
__device__ __forceinline__ bool fx_isspace(uint32_t c) { return c == 32u || (c - 9u) < 5u; }

__global__ __launch_bounds__(256) void fastx_lines_kernel(FastxParams P, int write)
{
	__shared__ uint32_t s_wave[4];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t mis = (uint32_t)((uintptr_t)P.text & 15u);
	const uint64_t a0 = (uint64_t)blockIdx.x * kFastxTile + (uint64_t)tid * 16u; // this lane's vector, from the aligned address below the text
	const uint64_t lo = mis, hi = (uint64_t)mis + P.len;                           // the text within that numbering
	uint32_t m[4] = { 0u, 0u, 0u, 0u };
	if (a0 >= lo && a0 + 16u <= hi) {
		const uint4 v = *(const uint4 *)(P.text + (a0 - lo));
		m[0] = fx_nl_mask(v.x), m[1] = fx_nl_mask(v.y), m[2] = fx_nl_mask(v.z), m[3] = fx_nl_mask(v.w);
	} else if (a0 + 16u > lo && a0 < hi) { // a partial vector: only the bytes inside the text are read
		for (uint32_t k = 0; k < 16u; ++k) {
			const uint64_t a = a0 + k;
			if (a >= lo && a < hi && P.text[a - lo] == (uint8_t)'\n') m[k >> 2] |= 0x80u << ((k & 3u) * 8u);
		}
	}
	const uint32_t c = (uint32_t)(__popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]));
	uint32_t inc = c; // the inclusive sum over the wavefront
#pragma unroll
	for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
	if (lane == 63u) s_wave[wave] = inc;
	__syncthreads();
	uint32_t before = 0;
	for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
	if (!write) {
		if (tid == 255u) P.tile_cnt[blockIdx.x] = before + inc;
		return;
	}
	if (blockIdx.x == 0 && tid == 0) P.line_off[0] = 0;
	uint32_t at = 1u + P.tile_cnt[blockIdx.x] + before + inc - c;
	for (uint32_t k = 0; k < 16u && at <= P.n_nl; ++k)
		if (m[k >> 2] >> ((k & 3u) * 8u) & 0x80u) P.line_off[at++] = (uint32_t)(a0 + k - lo) + 1u;
}

// line i of the table: [b, e) without its '\n'
__device__ __forceinline__ void fx_line(const FastxParams &P, uint32_t i, uint32_t &b, uint32_t &e)
{
	b = P.line_off[i];
	e = i < P.n_nl ? P.line_off[i + 1] - 1u : P.len;
}
// what a sequence or quality line that stands alone contributes: a trailing CR goes when the line is longer than one byte
__device__ __forceinline__ uint32_t fx_payload(const FastxParams &P, uint32_t b, uint32_t e)
{
	const uint32_t n = e - b;
	return n > 1u && P.text[e - 1u] == (uint8_t)'\r' ? n - 1u : n;
}
// a header line [b, e): the name's length (from b + 1) and the comment [cb, cb + cn)
__device__ __forceinline__ uint32_t fx_comment(const FastxParams &P, uint32_t b, uint32_t e, uint32_t name_n, uint32_t &cb)
{
	const uint32_t q = b + 1u + name_n;
	cb = q + 1u;
	if (q >= e) return 0u;
	const uint32_t cn = e - cb;
	return cn > 1u && P.text[e - 1u] == (uint8_t)'\r' ? cn - 1u : cn;
}
__device__ __forceinline__ void fx_list_long(const FastxParams &P, uint32_t i, uint32_t n)
{
	if (n < P.long_line) return;
	const uint32_t n_chunk = (n + kFastxLongChunk - 1u) / kFastxLongChunk;
	const uint32_t at = atomicAdd(&P.state[1], n_chunk);
	for (uint32_t c = 0; c < n_chunk; ++c) if (at + c < P.work_cap) P.work[at + c] = make_uint2(i, c);
}

__global__ __launch_bounds__(256) void fastx_classify_kernel(FastxParams P)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= P.n_lines) return;
	uint32_t b, e;
	fx_line(P, i, b, e);
	const uint32_t n = e - b, first = n ? P.text[b] : (uint32_t)'\n';
	const bool fq = P.cls == MM2AMD_FASTX_PATH_FASTQ4;
	const uint32_t kind = fq ? (i & 3u) : (first == (uint32_t)'>' ? 0u : 1u);
	uint32_t contrib = 0, viol = 0, is_hdr = 0;
	if (kind == 0u) { // a header
		if (fq && first != (uint32_t)'@') viol = 1u;
		uint32_t q = b + 1u;
		while (q < e && !fx_isspace(P.text[q])) ++q;
		const uint32_t name_n = n ? q - (b + 1u) : 0u;
		uint32_t cb;
		const uint32_t cn = n ? fx_comment(P, b, e, name_n, cb) : 0u;
		P.name_len[i] = name_n;
		contrib = name_n + 1u + ((P.flags & MM2AMD_FASTX_WITH_COMMENT) && cn ? cn + 1u : 0u) + (!fq && i > 0u ? 1u : 0u); // (FASTA: the NUL of the sequence before)
		is_hdr = 1u;
		if (!fq) atomicMax(&P.state[2], i);
	} else if (fq) {
		const uint32_t pay = fx_payload(P, b, e);
		if (kind == 1u) {
			if (n == 0u || first == (uint32_t)'>' || first == (uint32_t)'+' || first == (uint32_t)'@' || first == (uint32_t)'\r') viol = 1u;
			contrib = pay + 1u;
			fx_list_long(P, i, pay);
		} else if (kind == 2u) {
			if (first != (uint32_t)'+') viol = 1u;
		} else {
			uint32_t sb, se;
			fx_line(P, i - 2u, sb, se);
			if (pay != fx_payload(P, sb, se)) viol = 1u;
			if (P.flags & MM2AMD_FASTX_WITH_QUAL) { contrib = pay + 1u; fx_list_long(P, i, pay); }
		}
	} else { // FASTA: a sequence line, or an empty one
		if (first == (uint32_t)'+' || first == (uint32_t)'@' || (n == 1u && first == (uint32_t)'\r')) viol = 1u; // (a lone CR counts only while the sequence is empty: the host's case)
		contrib = n ? fx_payload(P, b, e) : 0u;
		fx_list_long(P, i, contrib);
	}
	P.dst[i] = contrib;
	if (!fq) P.ridx[i] = is_hdr;
	if (viol) atomicOr(&P.state[0], 1u);
}

__device__ __forceinline__ uint8_t fx_u2t(uint8_t c) { return (uint8_t)(c - ((c | 0x20u) == (uint8_t)'u' ? 1u : 0u)); }

__global__ __launch_bounds__(256) void fastx_copy_kernel(FastxParams P, int long_class)
{
	const bool fq = P.cls == MM2AMD_FASTX_PATH_FASTQ4;
	if (long_class) { // a chunk of a long sequence / quality line
		const uint2 it = P.work[blockIdx.x];
		const uint32_t i = it.x;
		if (i >= P.n_lines) return;
		if (!fq && P.ridx[i] > P.n_rec) return; // (a line of the record the buffer does not complete)
		uint32_t b, e;
		fx_line(P, i, b, e);
		const uint32_t pay = fx_payload(P, b, e), from = it.y * kFastxLongChunk, to = from + kFastxLongChunk < pay ? from + kFastxLongChunk : pay;
		const bool is_seq = !fq || (i & 3u) == 1u;
		const uint8_t *const s = P.text + b;
		uint8_t *const d = P.pool + P.dst[i];
		if (is_seq) for (uint32_t k = from + threadIdx.x; k < to; k += 256u) d[k] = fx_u2t(s[k]);
		else for (uint32_t k = from + threadIdx.x; k < to; k += 256u) d[k] = s[k];
		return;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0 && P.pool_len) P.pool[P.pool_len - 1u] = 0; // (FASTA: the last record's sequence ends there)
	const uint32_t l = threadIdx.x % kFastxShortLanes, i = blockIdx.x * (256u / kFastxShortLanes) + threadIdx.x / kFastxShortLanes;
	if (i >= P.n_lines) return;
	uint32_t b, e;
	fx_line(P, i, b, e);
	const uint32_t n = e - b;
	const uint32_t kind = fq ? (i & 3u) : (n && P.text[b] == (uint8_t)'>' ? 0u : 1u);
	const uint32_t at = P.dst[i];
	if (kind == 0u) {
		const uint32_t r = fq ? i >> 2 : P.ridx[i];
		if (r > P.n_rec) return;
		uint32_t name_at = at;
		if (!fq && i > 0u) { if (l == 0u) P.pool[at] = 0; ++name_at; }
		if (r == P.n_rec) return; // (the header that completes the last record and opens one the buffer does not hold)
		const uint32_t name_n = P.name_len[i];
		uint32_t cb;
		uint32_t cn = fx_comment(P, b, e, name_n, cb);
		if (!(P.flags & MM2AMD_FASTX_WITH_COMMENT)) cn = 0u;
		for (uint32_t k = l; k < name_n; k += kFastxShortLanes) P.pool[name_at + k] = P.text[b + 1u + k];
		const uint32_t com_at = name_at + name_n + 1u;
		for (uint32_t k = l; k < cn; k += kFastxShortLanes) P.pool[com_at + k] = P.text[cb + k];
		if (l == 0u) {
			P.pool[name_at + name_n] = 0;
			if (cn) P.pool[com_at + cn] = 0;
			FastxDevRec R;
			R.name = name_at, R.name_len = name_n, R.comment_len = cn, R.seq = com_at + (cn ? cn + 1u : 0u);
			R.l_seq = 0u;
			if (fq) { uint32_t sb, se; fx_line(P, i + 1u, sb, se); R.l_seq = fx_payload(P, sb, se); }
			P.recs[r] = R;
		}
		return;
	}
	if (fq ? (kind == 2u || (kind == 3u && !(P.flags & MM2AMD_FASTX_WITH_QUAL))) : (n == 0u || P.ridx[i] > P.n_rec)) return;
	const uint32_t pay = fx_payload(P, b, e);
	if (fq && l == 0u) P.pool[at + pay] = 0;
	if (pay >= P.long_line) return; // the long class writes the bytes
	if (!fq || kind == 1u) for (uint32_t k = l; k < pay; k += kFastxShortLanes) P.pool[at + k] = fx_u2t(P.text[b + k]);
	else for (uint32_t k = l; k < pay; k += kFastxShortLanes) P.pool[at + k] = P.text[b + k];
}

void fastx_lines_launch(const FastxParams &P, bool write, void *stream)
{
	if (P.n_tiles == 0) return;
	hipLaunchKernelGGL(fastx_lines_kernel, dim3(P.n_tiles), dim3(256), 0, (hipStream_t)stream, P, write ? 1 : 0);
	HIP_CHECK(hipGetLastError());
}

void fastx_classify_launch(const FastxParams &P, void *stream)
{
	if (P.n_lines == 0) return;
	hipLaunchKernelGGL(fastx_classify_kernel, dim3((P.n_lines + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, P);
	HIP_CHECK(hipGetLastError());
}

void fastx_copy_launch(const FastxParams &P, bool long_class, uint32_t n_work, void *stream)
{
	const uint32_t per = 256u / kFastxShortLanes;
	const uint32_t grid = long_class ? n_work : (P.n_lines + per - 1u) / per;
	if (grid == 0) return;
	hipLaunchKernelGGL(fastx_copy_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, P, long_class ? 1 : 0);
	HIP_CHECK(hipGetLastError());
}

} // namespace mm2amd
