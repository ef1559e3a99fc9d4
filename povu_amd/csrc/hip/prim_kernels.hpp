// prim_kernels.hpp -- the rows of povu_hip_call under POVU_HIP_PROFILE_DECOMPOSED (INTEGRATION.md "Decomposed calls";
// prim_kernels.hip, the aligner itself in prim_align.hpp): what call_kernels.hip hands over and what it gets back.
#pragma once
#include "call_common.hpp"

namespace povu_hip
{

// what lies on the device behind the spelling: the records in the order they are written, their spelled alleles, the
// reference paths.  Pair p = ac_off[j] + k - 1 is ALT k (1-based) of record j
struct PrimIn {
	uint32_t nrec;
	uint64_t n_pairs;
	const uint64_t *ac_off, *pos, *ref_spelled; // [nrec + 1], [nrec], [nrec]
	const uint32_t *path, *ref_allele, *block;
	const uint8_t *flags;
	const uint16_t *gt; // [nrec * slots.S]
	const uint64_t *block_off, *sp_off;
	const char *seq;
	PathsView paths;
	RefView ref;
	SlotsView slots;
	uint32_t cap;	    // the longest text that is aligned
	bool force_tier2;   // every aligned pair through the striped kernel
	uint64_t ref_bases; // bases of all reference paths (the width of the POS sort key)
};
// what the rows were made from, valid as long as they are: the rows before the sort (those of a pair consecutive, in alignment
// order, hence ascending by POS) and per pair where its rows lie there (n_pairs + 1 entries) and why it was kept whole
struct PrimPre {
	const uint64_t *row_off = nullptr, *pos = nullptr;
	const uint8_t *reason = nullptr, *lead = nullptr;
	const uint32_t *ref_len = nullptr;
};
// the rows, on the device (the context's arenas of the step, valid until the next call under the profile), in (reference path,
// row POS, record, ALT, alignment order), and the counters
struct PrimRows {
	uint64_t n_rows = 0;
	uint32_t *record = nullptr, *alt = nullptr, *index = nullptr, *ref_start = nullptr, *ref_len = nullptr, *alt_start = nullptr, *alt_len = nullptr,
		 *ac = nullptr, *an = nullptr, *ns = nullptr;
	uint8_t *kind = nullptr, *reason = nullptr, *lead = nullptr;
	uint64_t *pos = nullptr;
	uint64_t n_decomposed = 0, n_passthrough = 0, n_tier2 = 0, n_cells = 0;
	PrimPre pre; // (for merge_kernels.hip)
};
// Refused: 2^32 pairs or rows or more, a context base that is no nucleotide code (the message names the segment), slabs
// beyond device memory
PrimRows prim_rows(povu_hip_ctx *ctx, const PrimIn &in);

} // namespace povu_hip
