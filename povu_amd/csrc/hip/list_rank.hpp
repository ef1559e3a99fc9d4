// list_rank.hpp -- splitter-based list ranking (list_rank.hip): inclusive suffix sums along linked lists of up to 2^30 - 1
// elements.  The tree stage ranks two sets of lists with it, the Euler tour of the spanning forest (rank_tour) and the
// events of the pre-order (rank_events).  The contract, in one place:
//
// The writer fills RankBufs::pk and RankBufs::heads before it starts a ranking.
//   pk[x]     one level-0 word per element x < n (rank_pack): the successor, the element's 0/1 weight, and P0_HEAD on
//             every element that heads a list.  An element in no list gets P0_END; no walk reaches it, its rank is undefined.
//   heads[h]  for h < nh, the element that heads list h, or NIL for none.  A head is nobody's successor.
// The ranking walks the list once and leaves a RECORD per element in the caller's record array (n 8-byte slots, used as
// two planes) and the sums of the level above in the pools of RankBufs; the L0Ranks it returns names both.  An element's
// rank = R[owner] - partial, worked out where it is read (rank_l0*).  L0Ranks stays valid until the pools are used
// again -- by the next ranking or by whoever shares their memory -- and the records until the caller overwrites them.
//
// The reader batches its look-ups.
// The gathers are unconditional (gather_if, common.hpp), so that a reader's look-ups leave together as one batch: it gathers
// R.ra (and R.rb) at l0_at() of every record, puts landed() behind the batch and hands each word to rank_l0* with its record.
// An owner outside R, a record that holds a final rank (fin) and a record the caller does not want read R[0] in its place --
// safe: a ranking that ran has M >= 1 elements on level 1, and the callers only get here with records of a ranking that ran
// (a graph without links has no slot, and its R stays null: root_forest).
#pragma once
#include "common.hpp"
#include "pass_hooks.hpp"

namespace povu_hip
{

// words of the list itself (level 0): bits 0..29 successor (P0_END = none), bit 30 = the element's 0/1 weight, bit 31 = the
// element heads a list.  Whether the walk stops behind an element -- its successor is a splitter, or there is none -- is
// worked out from the successor (three integer operations), not stored: the bit it would take is the difference between
// 1.8 * 10^8 and 3.6 * 10^8 segments a graph may have.
static constexpr uint32_t P0_END = 0x3FFFFFFFu, P0_W = 0x40000000u, P0_HEAD = 0x80000000u;
// the word of an element with successor nx (NIL: none) and weight w; the writer that knows the heads ors P0_HEAD into theirs
__host__ __device__ __forceinline__ uint32_t rank_pack(uint32_t nx, uint32_t w) { return (nx == POVU_NIL ? P0_END : nx) | ((w & 1u) ? P0_W : 0u); }

// Level 0 leaves a RECORD per element on the walk up, and no walk goes down it again: the lane's id (= the
// element one level up whose rank the walks above hand out) and the sums from the splitter up to, not including, the
// element.  Its rank is then R[owner] - partial (rank_l0 / rank_l0_pair), resolved by the kernels that read it -- one
// store per element, where the way back stored the rank itself.  A record is {owner, partial}; with TWO the second word
// holds partial(a) | (partial(a) - partial(b)) << 16 (both never negative, at most two per element), and a segment
// whose sums outgrow 16 bits raises *ovf: k_rank_l0_fallback then walks the list once more and stores final ranks.
//
// The record array (n 8-byte slots) is used as two PLANES of n words, and nearly every record is one word of plane 0:
// the owner of x is a lane near bucket x >> b wherever the ids run along the lists, and a partial is bounded by the
// length of a splitter segment (geometric, mean 2^b).
//   narrow   plane0[x] = signed(owner - (x >> b)) << 15 | partial(s)         (bit 31 clear; ONE store)
//   escaped  plane0[x] = REC_ESC | owner,  plane1[x] = the second word        (delta or partial out of its field)
//   final    plane0[x] = a,  plane1[x] = b                                    (k_rank_l0_fallback; R.fin says so)
// The delta takes the 16 bits below REC_ESC in both rankings.  The tour: 15 bits of partial.  The events: 7 bits of
// partial(a), then 7 of partial(a) - partial(b); bit 14 stays clear.  Widths from the distributions in
// profiles/rank_records_summary.md: on graphs whose ids run along the lists no delta needs more than 16 bits but those of
// the head-led segments of later components, and no partial more than 8; a wider delta would buy nothing there, and at 16
// bits both edges of the field can be reached by lists of 2^18 elements (tests/test_gpu_rank_records.py).
static constexpr uint32_t REC_MAX = 0xFFFFu;
static constexpr uint32_t REC_ESC = 0x80000000u;
static constexpr unsigned REC_T_PBITS = 15, REC_T_DBITS = 16;
static constexpr unsigned REC_E_PBITS = 7, REC_E_DBITS = 16;
// {owner, second word} from the words of the planes (w1 is looked at only where w0 carries REC_ESC, or fin); rec_store of
// list_rank.hip is the way in.  TWO, here and below: a record of rank_events (two sums), else one of rank_tour
template <bool TWO>
__device__ __forceinline__ uint2 rec_decode(uint32_t x, unsigned b, uint32_t w0, uint32_t w1, bool fin = false)
{
	constexpr unsigned PB = TWO ? REC_E_PBITS : REC_T_PBITS, DB = TWO ? REC_E_DBITS : REC_T_DBITS;
	constexpr uint32_t PMAX = (1u << PB) - 1u;
	if (fin)
		return make_uint2(w0, w1);
	if (w0 & REC_ESC)
		return make_uint2(w0 & ~REC_ESC, w1);
	const uint32_t d = (uint32_t)((int32_t)(w0 << 1) >> (32 - DB));
	return make_uint2((x >> b) + d, TWO ? ((w0 & PMAX) | (((w0 >> PB) & PMAX) << 16)) : (w0 & PMAX));
}

// Where a level-0 rank is read (k_t0_parents, k_tree_emit): R = the inclusive suffix sums of the level-1
// elements (rb.wa, and rb.wb when TWO), M of them; with TWO, fin = the overflow word (set: the records hold final
// ranks).  (An owner outside R -- only a slot no tour reaches, which k_t0_parents reports as an error -- reads 0
// instead of memory past the pool.)
struct L0Ranks {
	const uint32_t *ra, *rb, *fin;
	uint32_t M;
	const uint32_t *w0, *w1; // the two planes of the level-0 records (plane 1 begins at a multiple of four words behind plane 0)
	unsigned b;		  // bucket bits of the ranking (rec_decode)
};
__device__ __forceinline__ uint32_t l0_at(const L0Ranks &R, uint2 rec, bool want = true) { return want && rec.x < R.M ? rec.x : 0u; }
// rank of an element (the 0/1 weights) from its record {owner, partial} and ra = R.ra[l0_at(R, rec)] ...
__device__ __forceinline__ uint32_t rank_l0(const L0Ranks &R, uint2 rec, uint32_t ra) { return (rec.x < R.M ? ra : 0u) - rec.y; }
// ... and with TWO (fin read once per lane by the caller; the words gathered at l0_at(R, rec, !fin)) the first sum or both
__device__ __forceinline__ uint32_t rank_l0_a(const L0Ranks &R, uint2 rec, bool fin, uint32_t ra)
{
	return fin ? rec.x : (rec.x < R.M ? ra : 0u) - (rec.y & REC_MAX);
}
__device__ __forceinline__ uint2 rank_l0_pair(const L0Ranks &R, uint2 rec, bool fin, uint32_t ra, uint32_t rb)
{
	const bool in = rec.x < R.M;
	const uint32_t pa = rec.y & REC_MAX;
	return fin ? rec : make_uint2((in ? ra : 0u) - pa, (in ? rb : 0u) - pa + (rec.y >> 16));
}
// one element on its own, from the planes (plane 1 only where the record escaped)
__device__ __forceinline__ uint32_t rank_l0_of(const L0Ranks &R, uint32_t x)
{
	const uint32_t w0 = R.w0[x];
	const uint2 rec = rec_decode<false>(x, R.b, w0, (w0 & REC_ESC) ? R.w1[x] : 0u);
	return rank_l0(R, rec, R.ra[l0_at(R, rec)]);
}
__device__ __forceinline__ uint2 rank_l0_pair_of(const L0Ranks &R, uint32_t x, bool fin)
{
	const uint32_t w0 = R.w0[x];
	const uint2 rec = rec_decode<true>(x, R.b, w0, (fin || (w0 & REC_ESC)) ? R.w1[x] : 0u, fin);
	const uint32_t i = l0_at(R, rec, !fin);
	return rank_l0_pair(R, rec, fin, R.ra[i], R.rb[i]);
}

struct RankBufs {
	uint32_t *pk;			 // [n+1] packed list words of level 0 (rank_pack)
	uint32_t *heads;		 // [max heads] level-0 element that heads list h, NIL for none
	uint32_t *nx, *wa, *wb;		 // pools for the levels above 0 (next words, sums), rank_pool_words() each
	uint32_t *tA, *tB, *tC;		 // three more pools: ping-pong of the global-memory fallback of the top level
};
// words every pool needs for lists of n elements in total with nh heads
size_t rank_pool_words(size_t n, size_t nh);
// bucket bits of a ranking: 3 (one element in 8 is a splitter), or what the hooks of the pass say (PassHooks::rank_bits)
unsigned rank_bucket_bits(const PassHooks &hooks);

// What a level-0 walk of a list ranking left in its records (debug hook povu_hip_debug_rank_escapes; k_rank_rec_stats).
// hist[33 * d + p]: live elements whose owner delta needs d bits (zigzag) and whose partial sums need p bits (the events: the
// larger of the two) -- worked out by walking the lists again, so the same for any split of the record word.
struct RankRecStats {
	bool valid = false;
	uint32_t fin = 0;	   // the walk overflowed its 16-bit partials: the records hold final ranks (all count as escaped)
	uint32_t bits = 0;	   // bucket bits of the ranking
	uint32_t delta_bits = 0;   // width of the signed owner delta of a narrow record
	uint32_t part_bits[2] = {}; // widths of its partial(s): the tour's one, the events' two
	uint64_t live = 0, esc = 0; // elements a walk reaches, and those of them whose record carries the escape bit
	uint64_t hist[33 * 33] = {};
};

// suffix sums (inclusive) along the lists packed in rb.pk, left as level-0 records rec[x] to be resolved by rank_l0:
// the sums of the 0/1 weights in the words (the Euler tour) ...
L0Ranks rank_tour(uint32_t n, unsigned b, uint2 *rec, uint32_t nh, RankBufs &rb, hipStream_t s, RankRecStats *st = nullptr);
// ... or, by rank_l0_pair, the two sums of the pre-order events: three elements per segment, whose weights follow from
// the index (rank_l0_weights).  `ovf` = a device word for the overflow flag (L0Ranks::fin)
L0Ranks rank_events(uint32_t n, unsigned b, uint2 *rec, uint32_t *ovf, uint32_t nh, RankBufs &rb, hipStream_t s,
		    RankRecStats *st = nullptr);

// unit-test hook: the level-0 ranks of the lists next[] (NIL = end) with heads[nh], as the readers resolve them -- mode 0:
// rank_tour, ra = suffix sums of the 0/1 weights w; mode 1: rank_events, ra, rb = the two sums of the events' weights (w =
// the weight bit of the words).  bits = bucket bits (0: the default).  Elements that are in no list get no defined value.
// st, plane0 (optional): what the walk left in its records, and the first word of every element's record
void debug_list_rank(uint32_t n, const uint32_t *next, const uint8_t *w, const uint32_t *heads, uint32_t nh, int mode,
		     unsigned bits, uint32_t *ra, uint32_t *rb, hipStream_t s, RankRecStats *st = nullptr,
		     std::vector<uint32_t> *plane0 = nullptr);

} // namespace povu_hip
