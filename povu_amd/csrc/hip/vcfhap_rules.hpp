// vcfhap_rules.hpp -- the rules of the haplotype comparison (INTEGRATION.md "Haplotype comparison"; restated in
// tests/vcfhap_ref.py) that are plain arithmetic: the full trim that makes an edit, one step of a reach, when a sorted span
// opens a window, when an edit of a sorted list conflicts with those in front of it, where byte h of a haplotype comes from,
// and the order of the statuses.  Free of HIP: vcfhap_kernels.hip runs them per lane and, chunk by chunk, per wave (the
// trims through the wave loops of vcfcmp_rules.hpp); host/vcfhap_check.cpp runs them on the CPU under the sanitizers.
// Coordinates are kept with one added (POS for the base POS names), so that a record at POS 0 has no negative start.
#pragma once
#include "search_rules.hpp"
#include "vcfcmp_rules.hpp"

namespace povu_hip
{

// ---- the full trim: the whole common suffix of REF and ALT, then the whole common prefix of what is left; either text may
// become empty.  The predicates byte by byte are the VCF comparison's (vm_suffix_differs, vm_prefix_differs)
VCFCMP_FN uint64_t vh_trim_limit(uint64_t nr, uint64_t na) { return nr < na ? nr : na; }
VCFCMP_FN uint64_t vh_suffix(const char *ref, uint64_t nr, const char *alt, uint64_t na)
{
	return vm_suffix_upto(ref, nr, alt, na, vh_trim_limit(nr, na));
}
VCFCMP_FN uint64_t vh_prefix(const char *ref, uint64_t nr, const char *alt, uint64_t na, uint64_t s)
{
	return vm_prefix_upto(ref, alt, vh_trim_limit(nr - s, na - s));
}
// the edit of (POS, REF, ALT) from the two trims: [bs, be) with one added, T = ALT[p, na - s)
struct VhEdit {
	uint64_t bs, be, t_at, t_len;
};
VCFCMP_FN VhEdit vh_edit(uint64_t pos, uint64_t nr, uint64_t na, uint64_t s, uint64_t p) { return {pos + p, pos + nr - s, p, na - s - p}; }
// an edit has a reach when exactly one of [bs, be) and T is empty
VCFCMP_FN bool vh_has_reach(uint64_t bs, uint64_t be, uint64_t t_len) { return (bs == be) != (t_len == 0); }
// the hash of an edit, a function of (s, e, T) alone (the text hash of T is vm_text_hash's)
VCFCMP_FN uint64_t vh_edit_hash(uint64_t bs, uint64_t be, uint64_t t_len, uint64_t t_hash) { return vm_key_hash(bs, be - bs, t_len, 0, t_hash); }

// ---- one step of a reach: step i to the right reads the base at e + i, to the left the base at s - 1 - i; the unit U of m
// bytes repeats
VCFCMP_FN bool vh_reach_right_ok(const char *unit, uint64_t m, uint64_t i, uint8_t base) { return vm_fold((char)base) == vm_fold(unit[i % m]); }
VCFCMP_FN bool vh_reach_left_ok(const char *unit, uint64_t m, uint64_t i, uint8_t base) { return vm_fold((char)base) == vm_fold(unit[m - 1 - (i % m)]); }

// ---- windows: sorted span k, whose predecessors reach the sorted spans below `reached` (the exclusive running maximum of
// 1 + the last span that starts at or before a span's end; 0 in front of the first), opens a window when none reaches it
VCFCMP_FN bool vh_window_head(uint32_t reached, uint32_t k) { return reached <= k; }

// ---- conflicts: an edit of a side's list, sorted by (s, e), against those in front of it: it starts before the largest end
// among them, or it is an insertion and so is its predecessor, at the same point
VCFCMP_FN bool vh_conflict(uint64_t bs, uint64_t be, bool has_prev, uint64_t max_end_before, uint64_t prev_bs, uint64_t prev_be)
{
	if (!has_prev)
		return false;
	return bs < max_end_before || (bs == be && prev_bs == prev_be && prev_bs == bs);
}

// ---- the byte locator.  A side's n edits, free of conflicts and in order, begin at the haplotype offsets start(u), ascending
// (start(u) = s_u - lo + the length changes of the edits in front).  vh_locate gives the last edit that begins at or before
// h, n when there is none; vh_source then says where byte h comes from: byte `at` of that edit's T, or byte `at` of the
// window's text
template <class Start>
VCFCMP_FN uint32_t vh_locate(uint64_t h, uint32_t n, Start &&start)
{
	const uint32_t lo = first_not(0u, n, [&](uint32_t u) { return start(u) <= h; }); // the first edit that begins behind h
	return lo ? lo - 1 : n;
}
struct VhSource {
	bool from_edit;
	uint64_t at;
};
// (none: no edit begins at or before h; else the found edit begins at `start`, carries t_len bytes and ends at window offset e_off)
VCFCMP_FN VhSource vh_source(uint64_t h, bool none, uint64_t start, uint64_t t_len, uint64_t e_off)
{
	if (none)
		return {false, h};
	const uint64_t in = h - start;
	return in < t_len ? VhSource{true, in} : VhSource{false, e_off + (in - t_len)};
}

// ---- the status of a cell: the first that applies (POVU_HIP_H_* of include/povu_hip.h); VH_COMPARE: the bytes decide
enum { VH_COMPARE = 0xFF };
VCFCMP_FN uint8_t vh_status(bool inconsistent, bool called_a, bool called_b, bool unspelled_a, bool unspelled_b, bool conflict_a, bool conflict_b)
{
	return inconsistent ? 0 : !called_a ? 1 : !called_b ? 2 : unspelled_a ? 3 : unspelled_b ? 4 : conflict_a ? 5 : conflict_b ? 6 : (uint8_t)VH_COMPARE;
}
VCFCMP_FN uint8_t vh_compared(bool equal, uint32_t edits_a, uint32_t edits_b) { return !equal ? 9 : (edits_a || edits_b) ? 8 : 7; }

} // namespace povu_hip
