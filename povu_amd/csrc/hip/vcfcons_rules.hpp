// vcfcons_rules.hpp -- the rules of the consensus haplotypes (INTEGRATION.md "Consensus haplotypes"; restated in
// tests/vcfcons_ref.py) that are plain arithmetic: the order of a haplotype's applied edits, what the three drop rules make of
// an edit given the edits in front of it, by how much a kept edit changes the length, and the walk of a lane of the
// materialiser through a haplotype's kept edits.  Free of HIP: vcfcons_kernels.hip runs them per lane and, chunk by chunk,
// per wave; host/vcfcons_check.cpp runs them on the CPU under the sanitizers.  The edit, the conflict predicate and the byte
// locator are those of the haplotype comparison (vcfhap_rules.hpp).  Coordinates are kept with one added, as there.
#pragma once
#include "vcfhap_rules.hpp"

namespace povu_hip
{

// ---- the order: s ascending, insertions (s == e) first, e descending, then the edit group.  The device sorts by the parts,
// least significant first; s and e are below 2^VC_COORD_BITS (a POS below 2^40 and a text below 2^32)
constexpr unsigned VC_COORD_BITS = 42;
VCFCMP_FN uint64_t vc_key_e(uint64_t be) { return ((1ull << VC_COORD_BITS) - 1) - be; } // (e descending)
VCFCMP_FN uint32_t vc_key_kind(uint64_t bs, uint64_t be) { return bs == be ? 0u : 1u; }	 // (insertions first)
// the parts of the order as the device's stable sort takes them, one pass each, least significant first: 0 the group, 1 / 2 the
// low and high word of the e key, 3 the kind, 4 / 5 the low and high word of s; a pass sorts the low vc_sort_bits bits of its part
constexpr int VC_SORT_PASSES = 6;
VCFCMP_FN uint32_t vc_sort_key(int which, uint64_t bs, uint64_t be, uint32_t group)
{
	switch (which) {
	case 0:
		return group;
	case 1:
		return (uint32_t)vc_key_e(be);
	case 2:
		return (uint32_t)(vc_key_e(be) >> 32);
	case 3:
		return vc_key_kind(bs, be);
	case 4:
		return (uint32_t)bs;
	default:
		return (uint32_t)(bs >> 32);
	}
}
VCFCMP_FN unsigned vc_sort_bits(int which, unsigned group_bits)
{
	return which == 0 ? group_bits : which == 3 ? 1u : (which == 1 || which == 4) ? 32u : VC_COORD_BITS - 32;
}
struct VcOrdered {
	uint64_t bs, be;
	uint32_t group;
};
VCFCMP_FN bool vc_before(const VcOrdered &a, const VcOrdered &b)
{
	if (a.bs != b.bs)
		return a.bs < b.bs;
	if (vc_key_kind(a.bs, a.be) != vc_key_kind(b.bs, b.be))
		return vc_key_kind(a.bs, a.be) < vc_key_kind(b.bs, b.be);
	if (a.be != b.be)
		return vc_key_e(a.be) < vc_key_e(b.be);
	return a.group < b.group;
}

// ---- the drops.  An edit of the ordered list against those in front of it: `max_end_before` is the exclusive running
// maximum of their ends, kept or not (0 in front of the first: an end is 1 at least), prev_* the edit right in front.
//   VC_DUPLICATE  the same (s, e, T) as its predecessor (the same group, s and e);
//   VC_ENCLOSED   it starts below that maximum and ends at or below it;
//   VC_OVERLAP    it starts below that maximum and ends behind it, or it is a second insertion at its predecessor's point
enum { VC_KEEP = 0, VC_DUPLICATE = 1, VC_ENCLOSED = 2, VC_OVERLAP = 3 };
VCFCMP_FN uint32_t vc_decide(uint64_t bs, uint64_t be, uint32_t group, bool has_prev, uint64_t max_end_before, uint64_t prev_bs, uint64_t prev_be,
			     uint32_t prev_group)
{
	if (!has_prev)
		return VC_KEEP;
	if (prev_bs == bs && prev_be == be && prev_group == group)
		return VC_DUPLICATE;
	if (!vh_conflict(bs, be, true, max_end_before, prev_bs, prev_be))
		return VC_KEEP;
	return bs < max_end_before && be <= max_end_before ? VC_ENCLOSED : VC_OVERLAP;
}
// the length change of a kept edit (modulo 2^64; a haplotype's sum is never negative)
VCFCMP_FN uint64_t vc_delta(uint64_t bs, uint64_t be, uint64_t t_len) { return t_len - (be - bs); }

// ---- the walk.  A haplotype's n kept edits, in order and free of overlaps, begin at the haplotype offsets start(u),
// ascending; edit(u) gives VcKept.  vc_seek finds the edit byte h lies in or behind (vh_locate, once per lane); vc_source
// moves on from there through the edits that begin at or before h -- h ascending from call to call -- and says where byte h
// comes from (vh_source): byte `at` of that edit's T, or base `at` of the path
struct VcKept {
	uint64_t start, t_len, e_off; // where it begins in the haplotype, |T|, its e (0-based: the base behind the replaced ones)
};
struct VcWalk {
	uint32_t k;  // the last edit that begins at or before the byte; n: none
	uint32_t nx; // the edit after it (0 when none)
	VcKept cur;
	uint64_t next_start; // start(nx), ~0 when there is none
};
template <class Edit>
VCFCMP_FN void vc_load(VcWalk &w, uint32_t n, Edit &&edit)
{
	if (w.k != n)
		w.cur = edit(w.k);
	w.next_start = w.nx < n ? edit(w.nx).start : ~0ull;
}
template <class Edit>
VCFCMP_FN VcWalk vc_seek(uint64_t h, uint32_t n, Edit &&edit)
{
	VcWalk w{};
	w.k = vh_locate(h, n, [&](uint32_t u) { return edit(u).start; });
	w.nx = w.k == n ? 0u : w.k + 1;
	vc_load(w, n, edit);
	return w;
}
// ... when the edit is known to lie between two others: `first` is the last edit that begins at or before some offset at or
// below h, `last` the last that begins at or before some offset at or above h (n each: none) -- the materialiser finds the pair
// once per tile, for the tile's first and last byte, and a lane bisects only the edits that begin inside the tile
template <class Edit>
VCFCMP_FN VcWalk vc_seek_between(uint64_t h, uint32_t first, uint32_t last, uint32_t n, Edit &&edit)
{
	VcWalk w{};
	const uint32_t lo = first == n ? 0u : first, hi = last == n ? 0u : last + 1;
	const uint32_t at = first_not(lo, hi, [&](uint32_t u) { return edit(u).start <= h; }); // the first edit that begins behind h
	w.k = at ? at - 1 : n;
	w.nx = w.k == n ? 0u : w.k + 1;
	vc_load(w, n, edit);
	return w;
}
template <class Edit>
VCFCMP_FN VhSource vc_source(VcWalk &w, uint64_t h, uint32_t n, Edit &&edit)
{
	while (w.next_start <= h) { // (of several edits that begin at one offset the last counts, as with vh_locate)
		w.k = w.nx, w.nx = w.nx + 1;
		vc_load(w, n, edit);
	}
	return vh_source(h, w.k == n, w.cur.start, w.cur.t_len, w.cur.e_off);
}
// the bytes from h on that come from consecutive bases of the path, when byte h does (else 0): up to the next edit
VCFCMP_FN uint64_t vc_ref_run(const VcWalk &w, uint64_t h, uint32_t n)
{
	if (w.k != n && h - w.cur.start < w.cur.t_len)
		return 0;
	return w.next_start - h; // (next_start > h after vc_source; ~0: to the haplotype's end and beyond)
}

} // namespace povu_hip
