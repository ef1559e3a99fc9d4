// untangle_kernels.hpp -- the untangled calls of povu_hip_call with POVU_HIP_T_UNTANGLE (untangle_kernels.hip; INTEGRATION.md
// "Untangled calls"): what the call hands the step and what it leaves on the device (the context's untangle arenas, valid
// until the next such call on the context).  Without the flag povu_hip_call runs none of this.
#pragma once
#include "call_common.hpp"

namespace povu_hip
{

// what the step reads of the call: the view, the slots, the sites' traversal ranges and kept numbers, the sorted flubble
// records (perm / dst as in call_kernels.hip: row dst[i], or i, holds record perm[i]) and the rows it rewrites
struct UntangleIn {
	CallView v;
	SlotsView slots;
	const uint32_t *qidx; // [n] number of a kept site among the kept
	uint32_t nQ;	      // kept sites
	uint32_t nfl, nrec;   // flubble records, all records
	const uint32_t *perm, *dst;
	InvRows rows;
	const uint32_t *smin, *smax; // the slot table of the old rule
	const uint64_t *ac_off;
	uint32_t *ac;
};
// the rows' own arrays and the counters
struct UntangleRows {
	uint8_t *rec_unt = nullptr;			// [nrec]
	uint32_t *lap = nullptr, *n_laps = nullptr;	// [nrec]
	uint16_t *lap_count = nullptr;			// [nrec * S]
	uint64_t n_tasks = 0, n_records = 0, n_missing = 0, n_extra = 0, n_fallback = 0;
};
UntangleRows untangle_rows(povu_hip_ctx *ctx, const UntangleIn &in);

} // namespace povu_hip
