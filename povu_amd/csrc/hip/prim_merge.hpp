// prim_merge.hpp -- the joint genotypes of merged primitives (INTEGRATION.md "Merged primitives"; restated in tests/merge_ref.py),
// everything of them that needs neither a cross-lane move nor a memory space: the span of a row, whether the rows of a
// (record, ALT) leave a span alone, what one member of a group says about one slot, and what the votes of a slot make.
// Plain C++17: merge_kernels.hip runs it on the device, a lane per sample; host/merge_check.cpp runs it under the sanitizers.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MERGE_HD __host__ __device__ inline
#else
#define MERGE_HD inline
#endif

namespace prim_merge
{

constexpr uint32_t GT_MISSING = 0xFFFFu; // POVU_HIP_GT_MISSING
constexpr uint8_t SLOT_MISSING = 0xFFu;	 // '.' in mrow_gt
// what a member says about a slot; _REF_ELSEWHERE: reference here because the slot's own ALT lies elsewhere
constexpr uint32_t VOTE_NONE = 0, VOTE_REF = 1, VOTE_ALT = 2, VOTE_REF_ELSEWHERE = 3;

// the rows as prim_rows made them, before the sort: those of a (record, ALT) are consecutive and ascend by POS and by span end
struct Rows {
	const uint64_t *pos;
	const uint32_t *ref_len;
	const uint8_t *lead;
};
// last base of the span of a row: POS + len(written REF) - 1, the written REF being the lead and the REF stretch
MERGE_HD uint64_t span_end(uint64_t pos, uint32_t ref_len, uint8_t lead) { return pos + ref_len + (lead ? 1u : 0u) - 1; }

// Does a row of [lo, hi) have a span that intersects [a, b]?  The first row whose span ends at a or behind it is found by
// bisection (its trip count fixed before the loop from hi - lo); it intersects when it begins at b or before, and no other
// row can: those before it end in front of a, those behind it begin no earlier than it does.
MERGE_HD bool rows_touch(const Rows &r, uint64_t lo, uint64_t hi, uint64_t a, uint64_t b)
{
	uint32_t trips = 0;
	for (uint64_t n = hi > lo ? hi - lo : 0; n; n >>= 1)
		trips++;
	uint64_t l = lo, h = hi > lo ? hi : lo;
	for (uint32_t t = 0; t < trips; t++) {
		if (l >= h)
			continue;
		const uint64_t mid = l + (h - l) / 2;
		if (span_end(r.pos[mid], r.ref_len[mid], r.lead[mid]) < a)
			l = mid + 1;
		else
			h = mid;
	}
	return l < hi && r.pos[l] <= b;
}

// the rows of another ALT of the member's record: primitive rows [lo, hi), or the ALT kept whole
struct OtherAlt {
	bool primitive;
	uint64_t lo, hi;
};
// The vote of member (j, k) of a group with span [a, b] on a slot that carries allele g of record j.  other(g) is asked only
// for 1 <= g <= n_alts, g != k.  A member of the group among the other ALT's rows overlaps the span and so needs no look of
// its own: it casts its own vote.  `rule`: false for a group that keeps the plain projection (a row kept whole)
template <class Other>
MERGE_HD uint32_t vote(uint32_t g, uint32_t k, uint32_t n_alts, bool rule, const Rows &rows, uint64_t a, uint64_t b, Other &&other)
{
	if (g == GT_MISSING)
		return VOTE_NONE;
	if (g == k)
		return VOTE_ALT;
	if (g == 0)
		return VOTE_REF;
	if (!rule || g > n_alts)
		return VOTE_NONE;
	const OtherAlt o = other(g);
	if (!o.primitive || rows_touch(rows, o.lo, o.hi, a, b))
		return VOTE_NONE;
	return VOTE_REF_ELSEWHERE;
}

// the votes of a slot, one bit per kind of vote, and what they make
struct Tally {
	uint32_t seen = 0;
};
MERGE_HD void cast(Tally &t, uint32_t v) { t.seen |= 1u << v; }
MERGE_HD bool any_alt(const Tally &t) { return t.seen & (1u << VOTE_ALT); }
MERGE_HD bool any_ref(const Tally &t) { return t.seen & ((1u << VOTE_REF) | (1u << VOTE_REF_ELSEWHERE)); }
MERGE_HD uint8_t slot_value(const Tally &t) { return any_alt(t) ? (uint8_t)1 : any_ref(t) ? (uint8_t)0 : SLOT_MISSING; }
MERGE_HD bool conflict(const Tally &t) { return any_alt(t) && any_ref(t); }
// 0 through the non-overlap rule alone
MERGE_HD bool ref_consistent(const Tally &t) { return !any_alt(t) && (t.seen & (1u << VOTE_REF_ELSEWHERE)) && !(t.seen & (1u << VOTE_REF)); }

} // namespace prim_merge
