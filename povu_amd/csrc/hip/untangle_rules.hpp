// untangle_rules.hpp -- the rules of the untangled calls (INTEGRATION.md "Untangled calls (decided here, modelled on
// `ita::untangle`)"; restated in tests/untangle_ref.py), everything of them that needs neither a cross-lane move nor a memory
// space: which (record, slot) entries are aligned, how the haplotype's lap sequence is oriented, a lane's step of the sweep
// over 16-bit symbols (the allele numbers of the laps), the step of the traceback to partner[], and the genotype code of a
// partner.  Plain C++17: untangle_kernels.hip runs it on the device, a lane of a wave each; host/untangle_check.cpp runs it
// under the sanitizers, 64 lane states stepped in lockstep.
//
// The table is that of prim_align.hpp (cell, code_of, two words of codes a lane): rows are the laps of the reference path R
// (n of them), columns the laps of the haplotype p (m of them), both at most 64, so the table is one stripe (tier 1).
#pragma once
#include "prim_align.hpp"

namespace untangle
{

constexpr uint32_t MAX_LAPS = prim_align::TIER1_MAX; // laps of either side an alignment takes: 64 rows at two bits each
constexpr uint8_t NO_PARTNER = 0xFF;		      // partner[i]: row i was deleted (the haplotype has no lap for it)
constexpr uint32_t CN_MAX = 65535;		      // lap_count saturates here
// state of a (reference run, slot) entry
constexpr uint8_t ENTRY_OLD = 0, ENTRY_TRIVIAL = 1, ENTRY_TASK = 2; // the old rule / aligned, one lap each / aligned by a task

// what is known of a slot at a site: the paths of the slot that traverse the site, the laps of the one path when it is one
// (m), whether that path is mixed; of the reference run: its laps n, mixed, its slot
PRIM_HD uint8_t entry_state(uint32_t n, bool ref_mixed, uint32_t ref_slot, uint32_t slot, uint32_t slot_paths, uint32_t m, bool mixed)
{
	if (ref_mixed || n < 1 || n > MAX_LAPS || slot == ref_slot || slot_paths != 1 || mixed || m < 1 || m > MAX_LAPS)
		return ENTRY_OLD;
	return (n >= 2 || m >= 2) ? ENTRY_TASK : ENTRY_TRIVIAL;
}
// lap of the haplotype's run (m laps in path order) that is symbol k of b: read backwards when the directions differ
PRIM_HD uint32_t oriented_lap(uint32_t k, uint32_t m, bool flipped) { return flipped ? m - 1 - k : k; }

// what a lane hands to its right neighbour: the value of its cell (at most 128) and the row's symbol
PRIM_HD uint32_t pack(uint32_t value, uint32_t a) { return (value & 0xFFFFu) | (a << 16); }
PRIM_HD uint32_t packed_value(uint32_t msg) { return msg & 0xFFFFu; }
PRIM_HD uint32_t packed_symbol(uint32_t msg) { return msg >> 16; }

// a lane of the sweep: prim_align::Lane with both words of codes kept
struct Lane {
	uint32_t up = 0, diag = 0, out = 0;
	uint64_t w0 = 0, w1 = 0; // the codes of rows 1 .. 32 and 33 .. 64 of the lane's column
};
// Step t of lane l, which owns column l + 1 (its symbol of b: `b`; live: l < m).  `in` is what the left neighbour handed on
// at step t - 1, or for lane 0 pack(t, a[t - 1]) (the border column).  A lane without a cell at this step changes nothing.
PRIM_HD void lane_step(Lane &s, uint32_t t, uint32_t l, uint32_t n, bool live, uint32_t b, uint32_t in)
{
	if (!live || t < l || t - l > n)
		return;
	const uint32_t i = t - l, left = packed_value(in);
	if (i == 0) { // the border row
		s.up = l + 1;
		s.diag = left;
		s.out = pack(l + 1, 0);
		return;
	}
	const uint32_t a = packed_symbol(in);
	const prim_align::Cell c = prim_align::cell(s.diag, s.up, left, a != b);
	s.diag = left;
	s.up = c.value;
	s.out = pack(c.value, a);
	const uint64_t bits = (uint64_t)c.code << (2 * ((i - 1) % prim_align::WORD_ROWS));
	if (i - 1 < prim_align::WORD_ROWS)
		s.w0 |= bits;
	else
		s.w1 |= bits;
}
// the word of a lane's column that holds row i (1-based)
PRIM_HD uint64_t word_of(const Lane &s, uint32_t i) { return i - 1 < prim_align::WORD_ROWS ? s.w0 : s.w1; }

// one step of the traceback from (i, j), not both 0.  `word`: the word of column j that holds row i (read only inside the
// table).  A diagonal step pairs row i with column j, a deletion leaves row i without a partner, an insertion is an extra lap
struct Trace {
	uint32_t i, j;
	bool row_done;	 // partner[row] is decided by this step ...
	uint32_t row;	 // ... for this row (0-based)
	uint8_t partner; // ... as this column (0-based) or NO_PARTNER
	bool extra;
};
PRIM_HD Trace trace_step(uint64_t word, uint32_t i, uint32_t j)
{
	const uint32_t code = (i && j) ? prim_align::code_of(word, i) : 0;
	const prim_align::TraceStep ts = prim_align::trace_step(code, i, j, false);
	if (ts.col == prim_align::COL_I)
		return {ts.i, ts.j, false, 0, NO_PARTNER, true};
	if (ts.col == prim_align::COL_D)
		return {ts.i, ts.j, true, i - 1, NO_PARTNER, false};
	return {ts.i, ts.j, true, i - 1, (uint8_t)(j - 1), false};
}

// the genotype code of allele x in a record whose REF is allele ra
PRIM_HD uint32_t code_of_allele(uint32_t x, uint32_t ra) { return x == ra ? 0 : x < ra ? x + 1 : x; }

} // namespace untangle
