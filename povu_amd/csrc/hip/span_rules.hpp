// span_rules.hpp -- the rules of the spanning alleles of a nested call (INTEGRATION.md "Spanning alleles"; restated in
// tests/span_ref.py) that are plain arithmetic: which (record, slot) entry is a candidate, when a candidate is spanned (a walk
// up the chain of enclosing records), the number the `*` ALT takes, and what a spanned entry adds to AC, AN and NS.  Free of
// HIP.  Two kinds of function live here:
//   run on the device, per lane   span_slot_empty, span_candidate (k_ns_span), span_n_alleles (k_cl_rec_fields), span_gt_code
//                                 (k_cl_records), and on the host span_refused (check_call_inputs, parse_call_args);
//   the definition, test-side     span_entry (the walk a lane would do alone: k_ns_span does it as a wave, 64 ancestors a
//                                 round), span_rounds, SpanCounts / span_count_sample (AC, AN and NS from the written codes:
//                                 k_cl_records keeps the plain call's loop, which counts whatever code it wrote).
// host/span_check.cpp runs both kinds on the CPU under the sanitizers and holds the first kind to the second: span_entry
// against a loop-over-the-lanes copy of the kernel's rounds, the counts on the codes span_gt_code gives.  It checks the rules,
// not the kernels' own loops; those are held to tests/span_ref.py on the GPU (tests/test_gpu_span.py).
#pragma once
#include "../../../include/povu_hip.h"

#include <cstdint>

#if defined(__HIPCC__)
#define SPAN_FN __host__ __device__ inline
#else
#define SPAN_FN inline
#endif

namespace povu_hip
{

static constexpr uint32_t SPAN_SLOT_EMPTY = 0xFFFFFFFFu; // the (site, slot) table's minimum where no path of the slot traverses the site
static constexpr uint32_t SPAN_NO_RECORD = 0xFFFFFFFFu;	 // "no parent" of the walk
static constexpr uint32_t SPAN_GT_MISSING = POVU_HIP_GT_MISSING;
static constexpr uint32_t SPAN_ROUND = 64;		 // ancestors a wave tests in one round

// no path of the slot traverses the site
SPAN_FN bool span_slot_empty(uint32_t slot_min) { return slot_min == SPAN_SLOT_EMPTY; }
// the entry may be spanned at all: the slot is empty at the record's site, the site's search was not cut short (any status
// bit means "unknown", which stays '.'), and the slot is not the record's own (that one is REF)
SPAN_FN bool span_candidate(bool slot_empty, uint8_t site_status, bool own_slot) { return slot_empty && site_status == 0 && !own_slot; }
// ... and it is: some ancestor's site is traversed by the slot.  parent(r): the enclosing record of r or SPAN_NO_RECORD;
// crossed(r): the slot is not empty at the site of record r.  A record without a parent has no ancestor
template <class Parent, class Crossed>
SPAN_FN bool span_entry(bool slot_empty, uint8_t site_status, bool own_slot, uint32_t rec, Parent &&parent, Crossed &&crossed)
{
	if (!span_candidate(slot_empty, site_status, own_slot))
		return false;
	for (uint32_t cur = parent(rec); cur != SPAN_NO_RECORD; cur = parent(cur))
		if (crossed(cur))
			return true;
	return false;
}
// rounds of SPAN_ROUND ancestors a chain of `depth` ancestors takes
SPAN_FN uint32_t span_rounds(uint32_t depth) { return (depth + SPAN_ROUND - 1) / SPAN_ROUND; }

// the record's numbering: its classes are 0 (REF) .. n_classes - 1, the `*` ALT comes last and takes the class count
SPAN_FN uint32_t span_star_code(uint32_t n_classes) { return n_classes; }
SPAN_FN uint32_t span_n_alleles(uint32_t n_classes, bool has_star) { return n_classes + (has_star ? 1u : 0u); }
// what is written for an entry: its code, or the `*` code where it is spanned (a spanned entry has no code of its own)
SPAN_FN uint32_t span_gt_code(uint32_t code, bool spanned, uint32_t n_classes) { return spanned && code == SPAN_GT_MISSING ? span_star_code(n_classes) : code; }

// AC, AN and NS of one record from its written codes: a spanned entry is called (AN, NS) and counts for the `*` ALT (AC)
struct SpanCounts {
	uint32_t an = 0, ns = 0;
};
// one sample's slots [s0, s1): ac[code - 1]++ for every ALT code, an per called slot, ns once when any slot is called
template <class Code> SPAN_FN void span_count_sample(uint32_t s0, uint32_t s1, Code &&code, uint32_t *ac, SpanCounts &c)
{
	bool any = false;
	for (uint32_t sl = s0; sl < s1; sl++) {
		const uint32_t g = code(sl);
		if (g == SPAN_GT_MISSING)
			continue;
		any = true;
		c.an++;
		if (g)
			ac[g - 1]++;
	}
	c.ns += any ? 1u : 0u;
}

// the option's own refusals (checked beside the limits of the profiles; profile: POVU_HIP_PROFILE_*): null, or the text of
// the library's message / of the command line's
inline const char *span_refused(bool command_line, bool nested_or_implied, uint32_t profile)
{
	if (profile == POVU_HIP_PROFILE_LEFT_NORMALIZED)
		return command_line ? "Flag '--spanning-alleles' cannot be combined with --profile left-normalized: a '*' allele is neither shifted nor trimmed"
				    : "POVU_HIP_T_SPANNING (spanning alleles) is refused with profile left-normalized: a '*' allele is neither shifted nor trimmed";
	if (profile == POVU_HIP_PROFILE_DECOMPOSED)
		return command_line ? "Flag '--spanning-alleles' cannot be combined with --profile decomposed: a '*' allele is not aligned"
				    : "POVU_HIP_T_SPANNING (spanning alleles) is refused with profile decomposed: a '*' allele is not aligned";
	if (!nested_or_implied)
		return command_line ? "Flag '--spanning-alleles' is an option of a nested call: it needs --nested, --profile top-level-only or --profile popped"
				    : "POVU_HIP_T_SPANNING (spanning alleles) is an option of a nested call: refused without POVU_HIP_T_NESTED and without a "
				      "profile that implies it";
	return nullptr;
}

} // namespace povu_hip
