// prim_align.hpp -- the aligner of the `decomposed` profile (INTEGRATION.md "Decomposed calls"; restated in tests/prim_ref.py),
// everything of it that needs neither a cross-lane move nor a memory space: upper-casing, the cell of the unit-cost table, a
// lane's state in the anti-diagonal sweep of a stripe of 64 columns, the step of the traceback, the primitives of the columns a
// traceback yields, and the rules that make rows of them.  Plain C++17: prim_kernels.hip runs it on the device, a lane of a
// wave each; host/prim_check.cpp runs it under the sanitizers, 64 lane states stepped in lockstep.
//
// The table D of REF a (n bytes) and ALT b (m bytes) has rows 0 .. n and columns 0 .. m, D[i][0] = i, D[0][j] = j.  A stripe
// holds the columns c0 + 1 .. c0 + 64; lane l owns column c0 + l + 1 and computes cell i = t - l at step t, so that the cell
// to its left was made one step before by lane l - 1 (the one cross-lane move of a step), the cell above by itself one step
// before and the diagonal one is the left cell of the step before.  Lane 0's left cell is column c0: the border (c0 = 0) or
// what the stripe before left of its last column.  With the value travels the byte of a for the row: lane 0 reads it, the
// others are handed it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PRIM_HD __host__ __device__ inline
#else
#define PRIM_HD inline
#endif

namespace prim_align
{

constexpr uint32_t MAX_LENGTH = 512; // POVU_HIP_PRIM_MAX_LENGTH
constexpr uint32_t LANES = 64;
constexpr uint32_t TIER1_MAX = 64; // both texts at most this long: the table is one stripe and its codes stay in two words a lane
// POVU_HIP_ROW_* and POVU_HIP_REASON_*
constexpr uint32_t ROW_RAW = 0, ROW_SNP = 1, ROW_INS = 2, ROW_DEL = 3, ROW_PASS = 4;
constexpr uint32_t REASON_NONE = 0, REASON_MAX_ALLELE_LENGTH = 1, REASON_CONTIG_START = 2, REASON_EMPTY_ALLELE = 3, REASON_EQUALS_REF = 4,
		   REASON_SUBR = 5;
// where a cell's value came from (two bits a cell), in the order the traceback prefers them
constexpr uint32_t CODE_DIAG = 0, CODE_DEL = 1, CODE_INS = 2;
// a column of the alignment
constexpr uint32_t COL_M = 0, COL_X = 1, COL_D = 2, COL_I = 3;

PRIM_HD uint8_t upper(uint8_t c) { return c >= 'a' && c <= 'z' ? (uint8_t)(c - 32) : c; }

struct Cell {
	uint32_t value, code;
};
// D[i][j] from D[i-1][j-1], D[i-1][j], D[i][j-1] and a[i-1] != b[j-1]; the code names the first of diagonal, deletion, insertion
// that gives the value
PRIM_HD Cell cell(uint32_t diag, uint32_t up, uint32_t left, bool differ)
{
	const uint32_t d = diag + (differ ? 1u : 0u), del = up + 1, ins = left + 1;
	const uint32_t v = d < del ? (d < ins ? d : ins) : (del < ins ? del : ins);
	return {v, d == v ? CODE_DIAG : del == v ? CODE_DEL : CODE_INS};
}

// what a lane hands to its right neighbour: the value of its cell (at most 1024) and the row's byte of a
PRIM_HD uint32_t pack(uint32_t value, uint8_t a) { return value | ((uint32_t)a << 16); }
PRIM_HD uint32_t packed_value(uint32_t msg) { return msg & 0xFFFFu; }
PRIM_HD uint8_t packed_base(uint32_t msg) { return (uint8_t)(msg >> 16); }

// rows of codes in one 64-bit word, and the words of a column of n rows
constexpr uint32_t WORD_ROWS = 32;
PRIM_HD uint32_t code_words(uint32_t n) { return (n + WORD_ROWS - 1) / WORD_ROWS; }
PRIM_HD uint32_t stripes(uint32_t m) { return (m + LANES - 1) / LANES; }
// 64-bit words of the codes of a whole table, [stripe][word of rows][lane]
PRIM_HD uint64_t slab_words(uint32_t n, uint32_t m) { return (uint64_t)stripes(m) * code_words(n) * LANES; }
PRIM_HD uint64_t slab_index(uint32_t stripe, uint32_t n, uint32_t word, uint32_t lane)
{
	return ((uint64_t)stripe * code_words(n) + word) * LANES + lane;
}

// a lane of the sweep: the cell above, the cell to the upper left, what it hands on, the codes of the rows of the open word
struct Lane {
	uint32_t up = 0, diag = 0, out = 0;
	uint64_t word = 0;
};
// a word of codes that is complete: rows [32 index, 32 index + 32) of the lane's column
struct Flush {
	bool full;
	uint32_t index;
	uint64_t word;
};
// Step t of lane l, which owns column jj (its byte of b: `b`; live: the column exists).  `in` is what the left neighbour
// handed on at step t - 1, or for lane 0 pack(D[t][c0], a[t - 1]).  A lane without a cell at this step changes nothing.
PRIM_HD Flush lane_step(Lane &s, uint32_t t, uint32_t l, uint32_t n, bool live, uint32_t jj, uint8_t b, uint32_t in)
{
	Flush f{false, 0, 0};
	if (!live || t < l || t - l > n)
		return f;
	const uint32_t i = t - l, left = packed_value(in);
	if (i == 0) { // the border row
		s.up = jj;
		s.diag = left;
		s.word = 0;
		s.out = pack(jj, 0);
		return f;
	}
	const uint8_t a = packed_base(in);
	const Cell c = cell(s.diag, s.up, left, upper(a) != upper(b));
	s.diag = left;
	s.up = c.value;
	s.out = pack(c.value, a);
	s.word |= (uint64_t)c.code << (2 * ((i - 1) % WORD_ROWS));
	if ((i - 1) % WORD_ROWS == WORD_ROWS - 1 || i == n) {
		f = Flush{true, (i - 1) / WORD_ROWS, s.word};
		s.word = 0;
	}
	return f;
}
// the code of cell (i, j), i and j at least 1, in the word of its column that holds row i
PRIM_HD uint32_t code_of(uint64_t word, uint32_t i) { return (uint32_t)(word >> (2 * ((i - 1) % WORD_ROWS))) & 3u; }

// one step of the traceback from (i, j), not both 0: the column and where it leads.  `code` is read only inside the table
// (the borders: i == 0 insertion, j == 0 deletion); differ: a[i-1] != b[j-1] upper-cased, read only on a diagonal step
struct TraceStep {
	uint32_t i, j, col;
};
PRIM_HD TraceStep trace_step(uint32_t code, uint32_t i, uint32_t j, bool differ)
{
	const uint32_t c = i == 0 ? CODE_INS : j == 0 ? CODE_DEL : code;
	if (c == CODE_DIAG)
		return {i - 1, j - 1, differ ? COL_X : COL_M};
	if (c == CODE_DEL)
		return {i - 1, j, COL_D};
	return {i, j - 1, COL_I};
}

// The primitives of an alignment whose columns arrive right to left: an SNP per X, a DEL per maximal run of D, an INS per
// maximal run of I.  sink.row(kind, ref_start, ref_len, alt_start, alt_len) takes them, the rightmost first.
struct Run {
	uint32_t kind = 0, len = 0, i = 0, j = 0; // kind 0: no run is open; (i, j): where its leftmost column begins
};
template <class Sink>
PRIM_HD void close_run(Run &r, Sink &sink)
{
	if (r.kind == ROW_DEL)
		sink.row(ROW_DEL, r.i, r.len, r.j, 0);
	else if (r.kind == ROW_INS)
		sink.row(ROW_INS, r.i, 0, r.j, r.len);
	r.kind = 0, r.len = 0;
}
// a column, and (i, j) behind it: the offsets in a and b where it begins
template <class Sink>
PRIM_HD void feed(Run &r, uint32_t col, uint32_t i, uint32_t j, Sink &sink)
{
	const uint32_t kind = col == COL_D ? ROW_DEL : col == COL_I ? ROW_INS : 0;
	if (kind != r.kind || !kind)
		close_run(r, sink);
	if (kind) {
		r.kind = kind, r.len++, r.i = i, r.j = j;
	} else if (col == COL_X) {
		sink.row(ROW_SNP, i, 1, j, 1);
	}
}

// ---- rows
struct Row {
	uint32_t kind, reason, index, ref_start, ref_len, alt_start, alt_len;
	uint64_t pos;
	uint8_t lead;	  // the anchor base of an indel, 0 for an SNP and a whole ALT ...
	bool context;	  // ... still to be read: the reference path's base in front of POS (an indel at offset 0)
};
// the ALT kept whole
PRIM_HD Row whole_row(uint32_t reason, uint64_t pos, uint32_t n, uint32_t m) { return Row{ROW_PASS, reason, 0, 0, n, 0, m, pos, 0, false}; }
// a primitive of a record at `pos` whose REF text is `ref`
PRIM_HD Row primitive_row(uint32_t kind, uint32_t index, uint64_t pos, uint32_t ref_start, uint32_t ref_len, uint32_t alt_start, uint32_t alt_len,
			  const char *ref)
{
	if (kind == ROW_SNP)
		return Row{kind, REASON_NONE, index, ref_start, ref_len, alt_start, alt_len, pos + ref_start, 0, false};
	return Row{kind, REASON_NONE, index, ref_start, ref_len, alt_start, alt_len, pos + ref_start - 1, ref_start ? (uint8_t)ref[ref_start - 1] : (uint8_t)0,
		   ref_start == 0};
}
// why a pair is not aligned, in the spec's order, or REASON_NONE
PRIM_HD uint32_t unaligned_reason(bool subr, uint64_t n, uint64_t m, uint32_t cap)
{
	return subr ? REASON_SUBR : (!n || !m) ? REASON_EMPTY_ALLELE : (n > cap || m > cap) ? REASON_MAX_ALLELE_LENGTH : REASON_NONE;
}
PRIM_HD uint32_t tier_of(uint32_t n, uint32_t m, bool force_tier2) { return (force_tier2 || n > TIER1_MAX || m > TIER1_MAX) ? 2 : 1; }

// the count pass: the rows of every kind and the last one fed, which is the leftmost
// (the rows of the three kinds in one word, 16 bits each: counters of their own behind a kind that is no constant become an
// indexed array, which leaves the registers)
PRIM_HD uint32_t kind_shift(uint32_t kind) { return 16 * (kind - ROW_SNP); }
PRIM_HD uint32_t kind_count(uint64_t packed, uint32_t kind) { return (uint32_t)(packed >> kind_shift(kind)) & 0xFFFFu; }
struct CountSink {
	uint64_t n = 0;
	uint32_t kind = 0, ref_start = 0, ref_len = 0, alt_start = 0, alt_len = 0;
	PRIM_HD void row(uint32_t k, uint32_t rs, uint32_t rl, uint32_t as, uint32_t al)
	{
		n += 1ull << kind_shift(k);
		kind = k, ref_start = rs, ref_len = rl, alt_start = as, alt_len = al;
	}
};
// what the count pass leaves of a pair
struct Counted {
	uint32_t n_snp, n_ins, n_del;
	uint32_t reason; // REASON_EQUALS_REF, REASON_CONTIG_START or REASON_NONE
	uint32_t n_rows;
	bool raw; // its one row is the record as the raw call writes it (_ROW_RAW)
};
// one_alt: the record has no other ALT.  The one row of such a record is _ROW_RAW when it spells the record's POS, REF and
// ALT: the lead and the row's stretch are all of REF, the lead and its stretch of b all of ALT, byte for byte
PRIM_HD Counted counted(const CountSink &c, uint64_t pos, bool one_alt, const char *ref, uint32_t n, const char *alt, uint32_t m)
{
	Counted o{kind_count(c.n, ROW_SNP), kind_count(c.n, ROW_INS), kind_count(c.n, ROW_DEL), REASON_NONE, 0, false};
	const uint32_t total = o.n_snp + o.n_ins + o.n_del;
	if (!total)
		o.reason = REASON_EQUALS_REF;
	else if (c.kind != ROW_SNP && c.ref_start == 0 && pos == 1)
		o.reason = REASON_CONTIG_START;
	o.n_rows = o.reason ? 1 : total;
	if (one_alt && !o.reason && total == 1) {
		const Row r = primitive_row(c.kind, 1, pos, c.ref_start, c.ref_len, c.alt_start, c.alt_len, ref);
		const uint32_t nl = (r.lead || r.context) ? 1 : 0;
		o.raw = r.pos == pos && !r.context && r.ref_start == nl && nl + r.ref_len == n && r.alt_start == nl && nl + r.alt_len == m &&
			(!nl || (uint8_t)alt[0] == r.lead);
	}
	return o;
}

// the emit pass: the same traceback again; row r from the right is row n_rows - 1 - r of the pair, its number within its
// kind what the count pass found less what has been seen from the right.  put(slot, row) is the writer's
template <class Writer>
struct EmitSink {
	Writer &w;
	uint64_t n; // the rows of every kind still to come (kind_count)
	uint32_t n_rows, seen = 0;
	uint64_t pos;
	const char *ref;
	bool raw;
	PRIM_HD EmitSink(Writer &writer, const Counted &c, uint64_t p, const char *r)
		: w(writer), n((uint64_t)c.n_snp << kind_shift(ROW_SNP) | (uint64_t)c.n_ins << kind_shift(ROW_INS) | (uint64_t)c.n_del << kind_shift(ROW_DEL)),
		  n_rows(c.n_rows), pos(p), ref(r), raw(c.raw)
	{
	}
	PRIM_HD void row(uint32_t k, uint32_t rs, uint32_t rl, uint32_t as, uint32_t al)
	{
		Row x = primitive_row(k, kind_count(n, k), pos, rs, rl, as, al, ref);
		n -= 1ull << kind_shift(k);
		if (raw)
			x.kind = ROW_RAW, x.index = 0;
		w.put(n_rows - 1 - seen, x);
		seen++;
	}
};

} // namespace prim_align
