// merge_kernels.hpp -- the merged rows of povu_hip_call under POVU_HIP_PROFILE_DECOMPOSED with POVU_HIP_T_MERGE (INTEGRATION.md
// "Merged primitives"; merge_kernels.hip, the votes themselves in prim_merge.hpp): what call_kernels.hip gets back.
#pragma once
#include "prim_kernels.hpp"

namespace povu_hip
{

// the merged rows, on the device (the context's arena of the step, valid until the next call with the flag), in the order of
// their first members among the rows, and the counters
struct MergedRows {
	uint64_t n_mrows = 0;
	uint64_t *off = nullptr;    // [n_mrows + 1] members of merged row g: member[off[g] .. off[g + 1])
	uint32_t *member = nullptr; // [n_rows] row indices, those of a group in row order
	uint8_t *gt = nullptr;	    // [n_mrows * S] 0, 1, 0xFF
	uint32_t *ac = nullptr, *an = nullptr, *ns = nullptr;
	uint64_t n_groups = 0, n_members = 0, n_splits = 0, n_ref_consistent = 0, n_conflicts = 0;
};
// Groups the rows `rows` that prim_rows made of `in` and votes.  Refused: 2^32 (group, slot) entries or more
MergedRows merge_rows(povu_hip_ctx *ctx, const PrimIn &in, const PrimRows &rows);

} // namespace povu_hip
