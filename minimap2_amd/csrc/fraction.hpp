// "%.4f" of a double in [0, 1] exactly as printf rounds it, shared by the host formatter (format.cpp) and rec_text_kernel (rec_text_dev.hpp).
// The double is M x 2^-k, so v x 10^4 = M x 10^4 / 2^k is an exact quotient and remainder: round to nearest, ties to even on the exact value
// (what glibc's printf does with its big-number arithmetic).  M x 10^4 needs 67 bits: two 64-bit words, no 128-bit type (there is none on the device).
#pragma once
#include <cstdint>
#include "exact_rsort.hpp" // MM2_HD

namespace mm2amd {

// v in [0, 1] (the caller checks): the four decimals and the digit before them as one number, 0 .. 10000
MM2_HD inline unsigned fraction_q4(double v)
{
	uint64_t bits;
	__builtin_memcpy(&bits, &v, 8);
	const int be = (int)(bits >> 52 & 0x7ff);
	uint64_t M = bits & ((1ull << 52) - 1);
	int k; // v = M x 2^-k
	if (be == 0) k = 1074; else M |= 1ull << 52, k = 1075 - be;
	if (k <= 0) return (unsigned)(M << -k) * 10000u; // (v <= 1 has k >= 52: never here; kept for completeness)
	if (k >= 68) return 0;                           // M x 10^4 < 2^67 <= half of 2^k: rounds to 0.0000
	// N = M x 10000 = hi x 2^64 + lo, from the two halves of M (a < 2^21, b < 2^32: no partial product overflows)
	const uint64_t a = (M >> 32) * 10000ull, b = (M & 0xffffffffull) * 10000ull;
	const uint64_t lo = (a << 32) + b, hi = (a >> 32) + (lo < b ? 1ull : 0ull);
	uint64_t quo, rem_hi, rem_lo, half_hi, half_lo;
	if (k < 64) {
		quo = (hi << (64 - k)) | (lo >> k);
		rem_hi = 0, rem_lo = lo & ((1ull << k) - 1), half_hi = 0, half_lo = 1ull << (k - 1);
	} else { // 64 .. 67
		const int s = k - 64;
		quo = hi >> s;
		rem_hi = hi & ((1ull << s) - 1), rem_lo = lo;
		half_hi = s > 0 ? 1ull << (s - 1) : 0, half_lo = s > 0 ? 0 : 1ull << 63;
	}
	unsigned q = (unsigned)quo;
	const bool above = rem_hi > half_hi || (rem_hi == half_hi && rem_lo > half_lo), tie = rem_hi == half_hi && rem_lo == half_lo;
	if (above || (tie && (q & 1u))) ++q;
	return q;
}

} // namespace mm2amd
