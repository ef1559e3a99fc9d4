// prim_kernels.hip -- the rows of a call under POVU_HIP_PROFILE_DECOMPOSED: every (REF, ALT) of a record aligned and written as
// its primitives.
//
// The definition is this project's own (INTEGRATION.md "Decomposed calls"; restated in tests/prim_ref.py); the aligner's logic
// is prim_align.hpp, which host/prim_check.cpp runs on the CPU.  The step reads the records as they are written (sorted, the
// inversion records merged in) and their spelled alleles:
//   pairs   a lane per (record, ALT): its texts, why it is not aligned (SUBR, an empty text, a text over the cap) or its tier;
//           two compacted lists of the aligned pairs;
//   align   one wave per pair, twice: a count pass that leaves the rows of every kind and the reasons that need the alignment
//           (equals_ref, contig_start), and after a scan of the row counts an emit pass that runs the same sweep and traceback
//           again and writes row r from the right at the pair's offset + rows - 1 - r.  Tier 1 (both texts of at most 64
//           bytes): the table is one stripe, the codes stay in two 64-bit words a lane.  Tier 2: stripes of 64 columns, the
//           last column of a stripe goes to the next through LDS, the codes to the pair's slab in the arena (sized by a scan
//           over the tier-2 pairs; DESIGN.md says what that costs);
//   rows    the projected genotype counts of every pair (one wave, a lane per sample), the stable sort of the rows by
//           (reference, row POS) and the gather of the 14 row arrays through it.
// Rules every kernel here keeps: the trip count of every loop is computed before the loop from the two lengths, from a count
// the host passed or from the grid (no loop ends on a value read from memory); no kernel waits for another wave or block and
// none has a block barrier; every shuffle runs with all 64 lanes (a lane without work is clamped, not left out); every store
// is checked against the range the host carved.
#include "prim_kernels.hpp"

#include "prim_align.hpp"

#include <type_traits>

namespace povu_hip
{

namespace
{

namespace pa = prim_align;

constexpr int WAVES = Q_TPB / 64;
// words[]: what the kernels tell the host
enum { W_CELLS = 0, W_MAX_LEN, W_DECOMPOSED, W_PASSTHROUGH, W_BROKEN, W_WORDS = 8 };

// per pair (n_pairs + 1 entries each)
struct PrPairs {
	uint32_t *rec, *nref, *nalt; // its record, the lengths of both texts
	uint64_t *ref_at, *alt_at;   // where the texts begin in the spelled bytes
	uint8_t *reason, *raw;	     // POVU_HIP_REASON_* when it is kept whole; its one row is _ROW_RAW
	uint32_t *n_snp, *n_ins, *n_del;
	uint64_t *nrows, *row_off;
	uint32_t *ac, *an, *ns; // of the genotypes projected on this ALT
};
// per row before the sort (n_rows + 1 entries each)
struct PrRows {
	uint64_t n;
	uint32_t *pair, *index, *ref_start, *ref_len, *alt_start, *alt_len;
	uint64_t *pos;
	uint8_t *kind, *reason, *lead;
};

__device__ __forceinline__ uint32_t alt_of_pair(const PrimIn &I, uint32_t j, uint64_t p) { return (uint32_t)(p - I.ac_off[j]) + 1; }

// a lane per pair
__global__ __launch_bounds__(Q_TPB) void k_pr_pairs(PrimIn I, PrPairs P, uint8_t *__restrict__ tier1, uint8_t *__restrict__ tier2,
						    unsigned long long *__restrict__ words)
{
	const uint64_t np = I.n_pairs, stride = (uint64_t)gridDim.x * Q_TPB;
	const uint32_t lane = threadIdx.x & 63u;
	// (a whole block per trip: the wave sums below run with every lane)
	for (uint64_t base = (uint64_t)blockIdx.x * Q_TPB; base < np; base += stride) {
		const uint64_t p = base + threadIdx.x;
		unsigned long long cells = 0, longest = 0;
		if (p < np) {
			const uint32_t j = span_of(I.ac_off, I.nrec, p), k = alt_of_pair(I, j, p), ra = I.ref_allele[j];
			const uint64_t sr = I.ref_spelled[j], sa = I.block_off[I.block[j]] + (k - 1 < ra ? k - 1 : k);
			const uint64_t r0 = I.sp_off[sr], n = I.sp_off[sr + 1] - r0, a0 = I.sp_off[sa], m = I.sp_off[sa + 1] - a0;
			const uint32_t reason = pa::unaligned_reason((I.flags[j] & POVU_HIP_CALL_SUBR) != 0, n, m, I.cap);
			const uint32_t tier = reason ? 0 : pa::tier_of((uint32_t)n, (uint32_t)m, I.force_tier2);
			P.rec[p] = j;
			P.nref[p] = (uint32_t)n;
			P.nalt[p] = (uint32_t)m;
			P.ref_at[p] = r0;
			P.alt_at[p] = a0;
			P.reason[p] = (uint8_t)reason;
			P.raw[p] = 0;
			P.n_snp[p] = P.n_ins[p] = P.n_del[p] = 0;
			tier1[p] = tier == 1;
			tier2[p] = tier == 2;
			cells = reason ? 0 : (n + 1) * (m + 1);
			longest = n > m ? n : m;
		}
		cells = wave_sum(cells);
		longest = wave_all_reduce(longest, ScanOp<1>{});
		if (lane == 0 && cells)
			atomicAdd(words + W_CELLS, cells);
		if (lane == 0 && longest >= (1ull << 32))
			atomicMax(words + W_MAX_LEN, longest);
	}
}

// words of the slab of every tier-2 pair
__global__ void k_pr_slab_words(uint32_t n2, const uint32_t *__restrict__ list, PrPairs P, uint64_t *__restrict__ cnt)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x <= n2; x += (uint64_t)gridDim.x * Q_TPB)
		cnt[x] = x < n2 ? pa::slab_words(P.nref[list[x]], P.nalt[list[x]]) : 0;
}

// ---- the sweep and the traceback of one pair by one wave; every lane calls, every lane feeds the sink the same rows
// ordering of LDS between the lanes of a wave (no instruction of its own: a wave's LDS accesses execute in order)
__device__ __forceinline__ void wave_order()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// tier 1: 1 <= n, m <= 64
template <class Sink>
__device__ __forceinline__ void pr_wave_tier1(const char *__restrict__ ref, uint32_t n, const char *__restrict__ alt, uint32_t m, uint32_t lane, Sink &sink)
{
	const uint32_t areg = lane < n ? pa::upper((uint8_t)ref[lane]) : 0, breg = lane < m ? pa::upper((uint8_t)alt[lane]) : 0;
	pa::Lane s;
	uint64_t w0 = 0, w1 = 0;
	const uint32_t steps = n + m + 1;
	for (uint32_t t = 0; t < steps; t++) {
		uint32_t in = __shfl_up(s.out, 1, 64);
		const uint32_t row = t < n ? t : n; // (lane 0 has no cell behind row n)
		const uint32_t a_row = __shfl(areg, (int)(row ? row - 1 : 0), 64);
		if (lane == 0)
			in = pa::pack(row, row ? (uint8_t)a_row : (uint8_t)0);
		const pa::Flush f = pa::lane_step(s, t, lane, n, lane < m, lane + 1, (uint8_t)breg, in);
		if (f.full) {
			if (f.index == 0)
				w0 = f.word;
			else
				w1 = f.word;
		}
	}
	uint32_t i = n, j = m;
	pa::Run run;
	const uint32_t trace = n + m;
	for (uint32_t k = 0; k < trace; k++) {
		if (i == 0 && j == 0)
			break;
		const uint32_t ii = (i ? i - 1 : 0) & 63u, jj = (j ? j - 1 : 0) & 63u;
		const unsigned long long mine = ii < pa::WORD_ROWS ? w0 : w1;
		const uint64_t word = __shfl(mine, (int)jj, 64);
		const uint32_t a = __shfl(areg, (int)ii, 64), b = __shfl(breg, (int)jj, 64);
		const pa::TraceStep ts = pa::trace_step(pa::code_of(word, ii + 1), i, j, a != b);
		i = ts.i, j = ts.j;
		pa::feed(run, ts.col, i, j, sink);
	}
	pa::close_run(run, sink);
}

// tier 2: 1 <= n, m <= 512.  sa, sb: MAX_LENGTH bytes, col: MAX_LENGTH + 1 values, the wave's own; slab: `words` words
template <class Sink>
__device__ __forceinline__ void pr_wave_tier2(const char *__restrict__ ref, uint32_t n, const char *__restrict__ alt, uint32_t m, uint32_t lane, uint8_t *sa,
					      uint8_t *sb, uint16_t *col, uint64_t *__restrict__ slab, uint64_t words, Sink &sink)
{
	for (uint32_t x = lane; x < n; x += 64)
		if (x < pa::MAX_LENGTH)
			sa[x] = pa::upper((uint8_t)ref[x]);
	for (uint32_t x = lane; x < m; x += 64)
		if (x < pa::MAX_LENGTH)
			sb[x] = pa::upper((uint8_t)alt[x]);
	wave_order();
	const uint32_t n_stripes = pa::stripes(m);
	for (uint32_t st = 0; st < n_stripes; st++) {
		const uint32_t c0 = st * pa::LANES, width = m - c0 < pa::LANES ? m - c0 : pa::LANES;
		const bool live = lane < width;
		const uint8_t b = live ? sb[c0 + lane] : (uint8_t)0;
		pa::Lane s;
		const uint32_t steps = n + width + 1;
		for (uint32_t t = 0; t < steps; t++) {
			uint32_t in = __shfl_up(s.out, 1, 64);
			const uint32_t row = t < n ? t : n;
			if (lane == 0)
				in = pa::pack(st ? col[row] : row, row ? sa[row - 1] : (uint8_t)0);
			const pa::Flush f = pa::lane_step(s, t, lane, n, live, c0 + lane + 1, b, in);
			if (f.full) {
				const uint64_t at = pa::slab_index(st, n, f.index, lane);
				if (at < words)
					slab[at] = f.word;
			}
			// The stripe's last column, for the next stripe, in place.  Invariant: col[r] is written at step r + 63 (here)
			// and the read of col[r] that is used is lane 0's at step r (row == t <= n), 63 steps before; the reads at
			// t > n are clamped to row n and their value is not used (lane 0 has no cell there).  Both accesses of a step
			// are the wave's own LDS operations in program order, the read first.  `steps`, the clamp of `row` and
			// this store keep that only together
			if (lane == pa::LANES - 1 && live && t >= lane && t - lane <= n && t - lane <= pa::MAX_LENGTH)
				col[t - lane] = (uint16_t)s.up;
		}
		wave_order();
	}
	__threadfence_block(); // (the slab is read back by other lanes of this wave)
	uint32_t i = n, j = m;
	pa::Run run;
	uint64_t key = ~0ull, mine = 0;
	const uint32_t trace = n + m, per_stripe = pa::code_words(n);
	for (uint32_t k = 0; k < trace; k++) {
		if (i == 0 && j == 0)
			break;
		const uint32_t ii = i ? i - 1 : 0, jj = j ? j - 1 : 0;
		// the 64 words of (stripe, rows) are loaded once, a lane each, and kept while the traceback stays in them
		const uint64_t want = (uint64_t)(jj / pa::LANES) * per_stripe + ii / pa::WORD_ROWS;
		if (want != key) {
			key = want;
			const uint64_t at = want * pa::LANES + lane;
			mine = at < words ? slab[at] : 0;
		}
		const uint64_t word = __shfl((unsigned long long)mine, (int)(jj % pa::LANES), 64);
		const bool differ = sa[ii < pa::MAX_LENGTH ? ii : 0] != sb[jj < pa::MAX_LENGTH ? jj : 0];
		const pa::TraceStep ts = pa::trace_step(pa::code_of(word, ii + 1), i, j, differ);
		i = ts.i, j = ts.j;
		pa::feed(run, ts.col, i, j, sink);
	}
	pa::close_run(run, sink);
}

// what an align kernel reads and writes beside the texts
struct PrAlign {
	PrimIn in;
	PrPairs pairs;
	PrRows rows; // (emit pass)
	unsigned long long *words, *bad;
};
// the emit pass's writer: lane 0 stores the row, behind the checks of its slot and of the row arrays
struct PrWriter {
	const PrAlign &A;
	uint64_t p;
	uint32_t lane, n_rows;
	__device__ __forceinline__ void put(uint32_t slot, pa::Row r)
	{
		if (lane != 0)
			return;
		const uint64_t x = A.pairs.row_off[p] + slot;
		if (slot >= n_rows || x >= A.rows.n) { // (the passes disagree: the call is refused)
			atomicOr(A.words + W_BROKEN, 1ull);
			return;
		}
		if (r.context && r.pos >= 1) { // the reference path's base in front of POS (r.pos is POS - 1)
			const PrimIn &I = A.in;
			const RefPathSlice R = ref_path_slice(I.ref, I.paths, I.ref.ref_of_path[I.path[A.pairs.rec[p]]]);
			if (R.n && r.pos - 1 < I.ref.roff[R.b + R.n] - I.ref.roff[R.b]) {
				uint32_t seg;
				r.lead = ref_path_base(I.paths, I.ref.roff, R, r.pos - 1, &seg);
				if (!comp(r.lead))
					atomicMin(A.bad, (unsigned long long)seg);
			}
		}
		const PrRows &o = A.rows;
		o.pair[x] = (uint32_t)p;
		o.kind[x] = (uint8_t)r.kind;
		o.reason[x] = (uint8_t)r.reason;
		o.index[x] = r.index;
		o.pos[x] = r.pos;
		o.ref_start[x] = r.ref_start;
		o.ref_len[x] = r.ref_len;
		o.alt_start[x] = r.alt_start;
		o.alt_len[x] = r.alt_len;
		o.lead[x] = r.lead;
	}
};
using PrEmitSink = pa::EmitSink<PrWriter>;

// One pair by one wave, for either pass.  align(sink) is the tier's sweep and traceback.  Count: lane 0 leaves what
// prim_align::counted makes of the rows.  Emit: a pair the count pass kept whole is left to k_pr_whole (the whole wave leaves
// before any shuffle)
template <class Sink, class Align>
__device__ __forceinline__ void pr_pair(const PrAlign &A, uint64_t p, uint32_t lane, const char *ref, uint32_t n, const char *alt, uint32_t m, Align &&align)
{
	const PrPairs &P = A.pairs;
	const uint32_t j = P.rec[p];
	const uint64_t pos = A.in.pos[j];
	if constexpr (std::is_same_v<Sink, pa::CountSink>) {
		pa::CountSink sink;
		align(sink);
		if (lane == 0) {
			const pa::Counted c = pa::counted(sink, pos, A.in.ac_off[j + 1] - A.in.ac_off[j] == 1, ref, n, alt, m);
			P.n_snp[p] = c.n_snp, P.n_ins[p] = c.n_ins, P.n_del[p] = c.n_del;
			P.reason[p] = (uint8_t)c.reason;
			P.raw[p] = c.raw;
		}
	} else {
		if (P.reason[p])
			return;
		pa::Counted c{P.n_snp[p], P.n_ins[p], P.n_del[p], pa::REASON_NONE, (uint32_t)P.nrows[p], P.raw[p] != 0};
		PrWriter w{A, p, lane, c.n_rows};
		PrEmitSink sink(w, c, pos, ref);
		align(sink);
		if (lane == 0 && sink.seen != c.n_rows)
			atomicOr(A.words + W_BROKEN, 1ull);
	}
}

// one wave per tier-1 pair
template <class Sink>
__global__ __launch_bounds__(Q_TPB) void k_pr_align(uint32_t n1, const uint32_t *__restrict__ list, PrAlign A)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t waves = (uint64_t)gridDim.x * WAVES;
	for (uint64_t x = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); x < n1; x += waves) {
		// a pair that is not what the host listed cannot be: the whole wave leaves it before any shuffle and the call is refused
		const uint64_t p = list[x];
		const bool listed = p < A.in.n_pairs;
		const uint32_t n = listed ? A.pairs.nref[p] : 0, m = listed ? A.pairs.nalt[p] : 0;
		if (!n || !m || n > pa::TIER1_MAX || m > pa::TIER1_MAX) {
			if (lane == 0)
				atomicOr(A.words + W_BROKEN, 1ull);
			continue;
		}
		const char *ref = A.in.seq + A.pairs.ref_at[p], *alt = A.in.seq + A.pairs.alt_at[p];
		pr_pair<Sink>(A, p, lane, ref, n, alt, m, [&](auto &sink) { pr_wave_tier1(ref, n, alt, m, lane, sink); });
	}
}

// one wave per tier-2 pair: its texts and the column between stripes in the wave's own LDS, its codes in slab[off[x] .. off[x + 1])
template <class Sink>
__global__ __launch_bounds__(Q_TPB) void k_pr_align_striped(uint32_t n2, const uint32_t *__restrict__ list, PrAlign A, uint64_t *__restrict__ slab,
							    const uint64_t *__restrict__ slab_off, uint64_t slab_total)
{
	__shared__ uint8_t s_a[WAVES][pa::MAX_LENGTH], s_b[WAVES][pa::MAX_LENGTH];
	__shared__ uint16_t s_col[WAVES][pa::MAX_LENGTH + 4];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint64_t waves = (uint64_t)gridDim.x * WAVES;
	for (uint64_t x = (uint64_t)blockIdx.x * WAVES + wave; x < n2; x += waves) {
		// a pair that is not what the host listed and carved cannot be: the whole wave leaves it before any shuffle and the
		// call is refused
		const uint64_t p = list[x];
		const bool listed = p < A.in.n_pairs;
		const uint32_t n = listed ? A.pairs.nref[p] : 0, m = listed ? A.pairs.nalt[p] : 0;
		const uint64_t s0 = slab_off[x], s1 = slab_off[x + 1];
		if (!n || !m || n > pa::MAX_LENGTH || m > pa::MAX_LENGTH || s1 > slab_total || s0 > s1 || s1 - s0 < pa::slab_words(n, m)) {
			if (lane == 0)
				atomicOr(A.words + W_BROKEN, 1ull);
			continue;
		}
		const char *ref = A.in.seq + A.pairs.ref_at[p], *alt = A.in.seq + A.pairs.alt_at[p];
		pr_pair<Sink>(A, p, lane, ref, n, alt, m,
			      [&](auto &sink) { pr_wave_tier2(ref, n, alt, m, lane, s_a[wave], s_b[wave], s_col[wave], slab + s0, s1 - s0, sink); });
	}
}

// rows of every pair, and the counters of the (record, ALT) that were split / kept whole (a _ROW_RAW row is neither)
__global__ __launch_bounds__(Q_TPB) void k_pr_row_count(uint64_t np, PrPairs P, unsigned long long *__restrict__ words)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t stride = (uint64_t)gridDim.x * Q_TPB;
	for (uint64_t base = (uint64_t)blockIdx.x * Q_TPB; base < np; base += stride) {
		const uint64_t p = base + threadIdx.x;
		unsigned long long dec = 0, pass = 0;
		if (p < np) {
			const bool whole = P.reason[p] != 0;
			P.nrows[p] = whole ? 1 : (uint64_t)P.n_snp[p] + P.n_ins[p] + P.n_del[p];
			pass = whole;
			dec = !whole && !P.raw[p];
		}
		dec = wave_sum(dec), pass = wave_sum(pass);
		if (lane == 0 && dec)
			atomicAdd(words + W_DECOMPOSED, dec);
		if (lane == 0 && pass)
			atomicAdd(words + W_PASSTHROUGH, pass);
	}
}

// the one row of a pair kept whole
__global__ void k_pr_whole(PrimIn I, PrPairs P, PrRows o)
{
	for (uint64_t p = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; p < I.n_pairs; p += (uint64_t)gridDim.x * Q_TPB) {
		const uint64_t x = P.row_off[p];
		if (!P.reason[p] || x >= o.n)
			continue;
		const pa::Row r = pa::whole_row(P.reason[p], I.pos[P.rec[p]], P.nref[p], P.nalt[p]);
		o.pair[x] = (uint32_t)p;
		o.kind[x] = (uint8_t)r.kind;
		o.reason[x] = (uint8_t)r.reason;
		o.index[x] = 0;
		o.pos[x] = r.pos;
		o.ref_start[x] = 0;
		o.ref_len[x] = r.ref_len;
		o.alt_start[x] = 0;
		o.alt_len[x] = r.alt_len;
		o.lead[x] = 0;
	}
}

// AC, AN and NS of a pair, counted on its record's GT row projected on the ALT (0 stays, the ALT is 1, anything else is
// missing): one wave per pair, a lane per sample (its slots are consecutive), as k_cl_records counts
__global__ __launch_bounds__(Q_TPB) void k_pr_genotypes(PrimIn I, PrPairs P)
{
	const uint32_t lane = threadIdx.x & 63u, S = I.slots.S, n_samples = I.slots.NS;
	const uint32_t *__restrict__ slot_first = I.slots.slot_first;
	const uint64_t waves = (uint64_t)gridDim.x * WAVES;
	for (uint64_t p = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); p < I.n_pairs; p += waves) {
		const uint32_t j = P.rec[p], k = alt_of_pair(I, j, p);
		const uint16_t *__restrict__ gt = I.gt + (uint64_t)j * S;
		uint32_t ac = 0, an = 0, ns = 0;
		for (uint32_t sm = lane; sm < n_samples; sm += 64) {
			bool any = false;
			const uint32_t s0 = slot_first[sm], s1 = min(slot_first[sm + 1], S);
			for (uint32_t sl = s0; sl < s1; sl++) {
				const uint32_t g = gt[sl];
				if (g == 0 || g == k) {
					any = true;
					an++;
					ac += g == k;
				}
			}
			ns += any;
		}
		ac = wave_sum(ac), an = wave_sum(an), ns = wave_sum(ns);
		if (lane == 0)
			P.ac[p] = ac, P.an[p] = an, P.ns[p] = ns;
	}
}

// sort key of row perm[x]: 0 = POS low word, 1 = POS high word, 2 = reference
__global__ void k_pr_key(uint32_t n, int which, const uint32_t *__restrict__ perm, PrRows o, const uint32_t *__restrict__ rec, PrimIn I,
			 uint32_t *__restrict__ key)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x < n; x += (uint64_t)gridDim.x * Q_TPB) {
		const uint32_t y = perm[x];
		key[x] = which == 0 ? (uint32_t)o.pos[y] : which == 1 ? (uint32_t)(o.pos[y] >> 32) : I.ref.ref_of_path[I.path[rec[o.pair[y]]]];
	}
}

__global__ void k_pr_gather(uint32_t n, const uint32_t *__restrict__ perm, PrRows u, PrPairs P, PrimIn I, PrimRows o)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x < n; x += (uint64_t)gridDim.x * Q_TPB) {
		const uint32_t y = perm[x], p = u.pair[y], j = P.rec[p];
		o.record[x] = j;
		o.alt[x] = alt_of_pair(I, j, p);
		o.kind[x] = u.kind[y];
		o.reason[x] = u.reason[y];
		o.index[x] = u.index[y];
		o.pos[x] = u.pos[y];
		o.ref_start[x] = u.ref_start[y];
		o.ref_len[x] = u.ref_len[y];
		o.alt_start[x] = u.alt_start[y];
		o.alt_len[x] = u.alt_len[y];
		o.lead[x] = u.lead[y];
		o.ac[x] = P.ac[p];
		o.an[x] = P.an[p];
		o.ns[x] = P.ns[p];
	}
}

} // namespace

PrimRows prim_rows(povu_hip_ctx *ctx, const PrimIn &in)
{
	hipStream_t s = ctx->stream;
	const uint64_t np = in.n_pairs;
	refuse_2_32(np, "the decomposed call needs ", "(record, ALT) pairs");
	PrimRows out;
	// ---- pairs
	const size_t p1 = (size_t)np + 1;
	PrPairs P;
	uint8_t *tier1, *tier2;
	uint32_t *list1, *list2, *counts;
	uint64_t *slab_cnt, *slab_off, *s64;
	unsigned long long *words, *bad;
	void *tmp;
	const size_t tmp_bytes = prim_tmp_bytes(p1, false) + 256;
	carve(ctx->pr_ws, [&](Spans &take) {
		take(p1, P.rec, P.nref, P.nalt, P.n_snp, P.n_ins, P.n_del, P.ac, P.an, P.ns, list1, list2);
		take(p1, P.ref_at, P.alt_at, P.nrows, P.row_off, slab_cnt, slab_off);
		take(p1, P.reason, P.raw, tier1, tier2);
		take(W_WORDS, words);
		take(1, bad);
		take(4, counts);
		take(scan_exclusive_u64_tmp(p1), s64);
		take(tmp_bytes, tmp);
	});
	HIP_CHECK(hipMemsetAsync(words, 0, W_WORDS * 8, s));
	HIP_CHECK(hipMemsetAsync(bad, 0xFF, 8, s));
	HIP_CHECK(hipMemsetAsync(counts, 0, 16, s));
	HIP_CHECK(hipMemsetAsync(P.nrows + np, 0, 8, s));
	if (np)
		KLAUNCH(k_pr_pairs, dim3(stride_blocks(np)), dim3(Q_TPB), 0, s, in, P, tier1, tier2, words);
	compact_flagged_u8(tier1, np, list1, counts, tmp, tmp_bytes, s);
	compact_flagged_u8(tier2, np, list2, counts + 1, tmp, tmp_bytes, s);
	uint32_t h_counts[2] = {0, 0};
	unsigned long long h_words[W_WORDS] = {};
	HIP_CHECK(copy_async(h_counts, counts, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(copy_async(h_words, words, W_WORDS * 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	const uint32_t n1 = h_counts[0], n2 = h_counts[1];
	refuse_2_32(h_words[W_MAX_LEN], "an allele of the decomposed call has ", "bases");
	out.n_cells = h_words[W_CELLS];
	out.n_tier2 = n2;
	// ---- the slabs of the tier-2 pairs, then the count pass
	uint64_t *slab = nullptr, slab_total = 0;
	if (n2) {
		KLAUNCH(k_pr_slab_words, dim3(stride_blocks((size_t)n2 + 1)), dim3(Q_TPB), 0, s, n2, list2, P, slab_cnt);
		scan_exclusive_u64(slab_cnt, slab_off, (size_t)n2 + 1, s64, s);
		slab_total = read_back(slab_off + n2, s);
		carve(ctx->pr_slab, [&](Spans &take) { take(slab_total + 1, slab); });
	}
	PrAlign A{in, P, PrRows{}, words, bad};
	if (n1)
		KLAUNCH(k_pr_align<pa::CountSink>, dim3(wave_blocks(n1)), dim3(Q_TPB), 0, s, n1, list1, A);
	if (n2)
		KLAUNCH(k_pr_align_striped<pa::CountSink>, dim3(wave_blocks(n2)), dim3(Q_TPB), 0, s, n2, list2, A, slab, slab_off, slab_total);
	if (np)
		KLAUNCH(k_pr_row_count, dim3(stride_blocks(np)), dim3(Q_TPB), 0, s, np, P, words);
	scan_exclusive_u64(P.nrows, P.row_off, p1, s64, s);
	const uint64_t n_rows = read_back(P.row_off + np, s);
	refuse_2_32(n_rows, "the decomposed call needs ", "rows");
	// ---- rows
	const uint32_t nr = (uint32_t)n_rows;
	const size_t r1 = (size_t)nr + 1;
	PrRows u;
	u.n = n_rows;
	uint32_t *perm, *perm2, *key, *key2;
	void *sort_tmp;
	const size_t sort_bytes = prim_tmp_bytes(r1, true) + 256;
	carve(ctx->pr_rows, [&](Spans &take) {
		take(r1, u.pair, u.index, u.ref_start, u.ref_len, u.alt_start, u.alt_len, perm, perm2, key, key2);
		take(r1, out.record, out.alt, out.index, out.ref_start, out.ref_len, out.alt_start, out.alt_len, out.ac, out.an, out.ns);
		take(r1, u.pos, out.pos);
		take(r1, u.kind, u.reason, u.lead, out.kind, out.reason, out.lead);
		take(sort_bytes, sort_tmp);
	});
	A.rows = u;
	if (np) {
		KLAUNCH(k_pr_whole, dim3(stride_blocks(np)), dim3(Q_TPB), 0, s, in, P, u);
		KLAUNCH(k_pr_genotypes, dim3(wave_blocks(np)), dim3(Q_TPB), 0, s, in, P);
	}
	if (n1)
		KLAUNCH(k_pr_align<PrEmitSink>, dim3(wave_blocks(n1)), dim3(Q_TPB), 0, s, n1, list1, A);
	if (n2)
		KLAUNCH(k_pr_align_striped<PrEmitSink>, dim3(wave_blocks(n2)), dim3(Q_TPB), 0, s, n2, list2, A, slab, slab_off, slab_total);
	uint64_t h_bad = 0;
	HIP_CHECK(copy_async(h_words, words, W_WORDS * 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(copy_async(&h_bad, bad, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	if (h_words[W_BROKEN])
		throw HipError("decomposed call: an aligner wave met a pair it was not listed for, or its passes disagree (internal error)");
	if (h_bad != ~0ull)
		throw HipError("segment " + std::to_string(read_back(ctx->g.vid + h_bad, s)) + " holds a byte that is no nucleotide code (ACGTN, lower case, IUPAC)");
	out.n_decomposed = h_words[W_DECOMPOSED], out.n_passthrough = h_words[W_PASSTHROUGH];
	out.n_rows = n_rows;
	out.pre = PrimPre{P.row_off, u.pos, P.reason, u.lead, u.ref_len}; // (no later step of this call writes them or carves their arenas)
	if (!nr)
		return out;
	// ---- order: stable by (reference, row POS); record, ALT and alignment order follow from the order the rows were made in
	launch_iota(nr, perm, s);
	LsdSort sort{perm, perm2, key, key2, nr, sort_tmp, sort_bytes, s};
	auto write_key = [&](int which, const uint32_t *cur, uint32_t *k) {
		KLAUNCH(k_pr_key, dim3(stride_blocks(nr)), dim3(Q_TPB), 0, s, nr, which, cur, u, P.rec, in, k);
	};
	sort.pass(0, 32, write_key);
	if (in.ref_bases + 1 >= (1ull << 32))
		sort.pass(1, 32, write_key);
	if (in.ref.nR > 1)
		sort.pass(2, bits_for(in.ref.nR), write_key);
	KLAUNCH(k_pr_gather, dim3(stride_blocks(nr)), dim3(Q_TPB), 0, s, nr, sort.cur, u, P, in, out);
	return out;
}

} // namespace povu_hip
