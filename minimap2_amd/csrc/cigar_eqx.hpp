// MM_F_EQX on the device: mm_update_cigar_eqx (align.c:183-252) for the regions region_finish_kernel has just finished.  Every match operation
// becomes its maximal stretches of equal (=, 7) and of unequal (X, 8) columns; a CIGAR none of whose matches splits is relabelled M -> = as it
// stands (the reference's in-place branch: also a match that is ONE stretch of mismatches becomes =).  The =/X CIGAR can be longer than the
// stitched one and longer than kFinMaxOps, so it does not fit the region's slot in the finish pool: a counting pass gives every region its
// length, an exclusive sum over the lengths places the regions in a pool of exactly that size, a writing pass stores the operations.
#pragma once
#include <cstdint>
#include "region_finish.hpp"

namespace mm2amd {

struct EqxParams {
	const FinRegion *regions; int n_regions;  // as region_finish_kernel saw them (q_pos, t_pos, out_off)
	const FinResult *results;                 // what it left: n_cigar (<= 0: nothing to do), qshift, tshift
	const uint32_t *fin_pool;                 // its output pool: region i's operations at regions[i].out_off
	const uint8_t *qpool;
	const uint32_t *S;
	uint32_t *n_ops;                          // counting pass, per region: operations of the =/X CIGAR; equal to n_cigar <=> relabelled in place
	const uint64_t *out_off;                  // writing pass, per region: where its =/X CIGAR starts in out_pool (the exclusive sum of n_ops)
	uint32_t *out_pool;
};

void cigar_eqx_launch(const EqxParams &P, bool write, void *stream);

// what the backend hands to the host beside the finish results (views it owns): region i's =/X CIGAR is cigars[off[i] .. off[i] + n_ops[i]).
// n_ops null: the pass did not run (no MM_F_EQX)
struct EqxOut { const uint32_t *n_ops = nullptr; const uint64_t *off = nullptr; const uint32_t *cigars = nullptr; };

// mm_extra_t::capacity after mm_update_cigar_eqx (align.c:199-207, :217): unchanged when the CIGAR was relabelled in place (the count stayed);
// otherwise the operation count plus the header's BYTE size, rounded up to a power of two, as the reference writes it
inline uint32_t eqx_capacity(uint32_t capacity, uint32_t n_before, uint32_t n_after, uint32_t header_bytes)
{
	if (n_after == n_before) return capacity;
	uint32_t x = n_after + header_bytes; // n_before + (n_EQX - n_M) is n_after
	--x, x |= x >> 1, x |= x >> 2, x |= x >> 4, x |= x >> 8, x |= x >> 16, ++x;
	return x;
}

} // namespace mm2amd
