// nest_kernels.hpp -- the nested calls of povu_hip_call with POVU_HIP_T_NESTED (nest_kernels.hip; INTEGRATION.md "Nested
// calls"): what the call hands the two steps and what they leave on the device (the context's nest arenas, valid until the
// next nested call on the context).
#pragma once
#include "call_common.hpp"
#include "span_rules.hpp"

namespace povu_hip
{

// the traversals of the called sites in path order: entry i is traversal it[i] of site iq[i] over the global path positions
// [ipos[i], iend[i]], ipos ascending (a global position names the path too: the paths are concatenated)
struct NestIndex {
	uint32_t ni = 0;
	uint64_t *ipos = nullptr, *iend = nullptr;
	uint32_t *iq = nullptr, *it = nullptr;
};
// (the first entry whose position is at least x: lower_bound(ipos, 0u, ni, x))
// The index of the traversals flagged in flag[0 .. R): ix's arrays (R + 1 entries each, the caller's) filled, ix.ni set.
// The scratch is the caller's: four lists of R + 1, one cleared word, prim_tmp_bytes(R + 1, true) bytes.  Waits for the stream
struct NestIndexWs {
	uint32_t *ilist, *pb, *key, *kout, *count;
	void *tmp;
	size_t tmp_bytes;
};
void nest_index(povu_hip_ctx *ctx, const TravDevice &d, const uint8_t *flag, NestIndex &ix, const NestIndexWs &w);

// the classes: of site q the classes [coff[q], coff[q + 1]), numbered in the order of their lowest exact allele; of class c its
// representative's global allele crep[c] and that allele's first traversal cfirst[c]; of traversal t its class within its
// site, oc[t]
struct NestClasses {
	NestIndex ix;
	uint32_t n_cl = 0, n_tier2 = 0;
	uint64_t n_splits = 0;
	uint32_t *coff = nullptr, *crep = nullptr, *cfirst = nullptr, *oc = nullptr;
};
// `called`: [n] the called sites; force_tier2: every candidate allele through the wave kernels
NestClasses nest_classes(povu_hip_ctx *ctx, const TravDevice &d, const uint8_t *called, uint32_t max_steps, bool force_tier2);

// the records' nesting, from the call's view: the flubble records before they are sorted (record j = traversal rlist[j], a
// reference traversal of a kept site), the sites' PVST heights, the written lengths of every record's REF and of its longest
// allele; `limits`: the profile and its limits.
// Out, per record j: level, the parent's site (NO_QUERY: none), rescued; `kept`: the n_kept records the profile keeps,
// ascending (raw-graph: all)
struct NestRecs {
	uint32_t *level = nullptr, *parent_q = nullptr, *kept = nullptr;
	uint8_t *rescued = nullptr;
	uint32_t n_kept = 0;
	uint64_t n_enclosed = 0, n_popped = 0, n_rescued = 0;
	// with NestSpan::on ("Spanning alleles"), per record j: star[j] = 1 when some entry of the record is spanned, and a word
	// per 64 slots, span_bits[j * span_words + sl / 64] bit sl % 64 = entry (j, sl) is spanned.  The counters are those of the
	// records the profile keeps and the regions pass.  Else: null, 0
	uint8_t *star = nullptr;
	unsigned long long *span_bits = nullptr;
	uint32_t span_words = 0;
	uint64_t n_star_records = 0, n_star_entries = 0;
};
// POVU_HIP_T_SPANNING: what k_ns_span reads beside the records -- the (kept site, slot) table of the call (the minimum allele,
// SPAN_SLOT_EMPTY where no path of the slot traverses the site), the kept sites' rows, the slots, and the sites the regions
// pass (null: no regions).  on == false: nothing is launched
struct NestSpan {
	bool on = false;
	const uint32_t *qidx = nullptr, *smin = nullptr, *slot_of_path = nullptr;
	uint32_t S = 0;
	const uint8_t *pass = nullptr;
};
NestRecs nest_records(povu_hip_ctx *ctx, const CallView &v, const NestIndex &ix, const povu_hip_call_profile_opts &limits, const NestSpan &span = NestSpan{});

} // namespace povu_hip
