// par_kernels.hpp -- data-parallel formulations of rows D-G (see par_kernels.hip)
#pragma once
#include "common.hpp"
#include "graph_kernels.hpp"
#include "pass_hooks.hpp"
#include "seq_kernels.hpp"

#include <functional>

namespace povu_hip
{

// Min segment tree over n values, kept COARSE: its leaves are the minima of blocks of SEG_BLK consecutive values, the
// values themselves stay where they are (val must outlive the queries).  A query reads the one or two blocks at its ends
// as whole cache lines and walks the tree only over the blocks in between: 1/16 of the writes of a full tree, and the
// short ranges most queries have never touch it (segtree.hpp).
struct SegTree {
	uint32_t *tree = nullptr;     // [2P], node 1 = root, block minima at [P, 2P)
	const uint32_t *val = nullptr; // [n] the values (16-byte aligned, readable up to the next multiple of SEG_BLK)
	uint32_t P = 1;		      // blocks, padded to a power of two with +inf
	static constexpr uint32_t BLK = 16;
	static uint32_t pow2(size_t n)
	{
		uint32_t p = 1;
		while (p < n)
			p <<= 1;
		return p;
	}
	static size_t tree_words(size_t n) { return 2 * (size_t)pow2((n + BLK - 1) / BLK + 1); }
};

// The words of ParWs::err: the counters and internal error flags of one pass, cleared together ahead of the tree stage
// (zero_component_counters).  Each line: who writes the word -> who reads it.  The numbers are part of no interface, but the
// two crossing words stay adjacent (povu_hip_last_crossings copies them as a pair).
enum PassWord : uint32_t {
	PW_NO_BRACKET = 0,   // k_top_bracket: a tree vertex has no live bracket -> k_summary
	PW_FOREST_SIZE = 2,  // k_t0_parents: the spanning forest of the links has the wrong size -> k_summary
	PW_N_OVER = 4,	     // k_class_dfs_small: classes handed to the wave walk -> the host (class_walks)
	PW_LITERAL_RULE = 5, // k_capping: the literal hi_2 rule capped below the second-highest reach -> the host (place_brackets)
	PW_NB0 = 6,	     // k_back_edges: back edges of the tree stage -> k_bracket_extra, the host (place_brackets)
	PW_POOL_TOP = 7,     // k_class_walk_wave: entries taken from the walks' stack pool (no other reader)
	PW_WALK_POOL = 8,    // k_class_walk_wave: the stack pool ran out -> the host (class_walks), k_summary
	PW_N_ENTRY = 9,	     // k_entry_list: entries of the 2-edge-connected classes -> k_class_dfs_small, the host (F_BIG_CLASS_DFS)
	PW_N_BRIDGE = 10,    // k_hi_simp: bridge vertices listed -> k_capping
	PW_N_X = 11,	     // compact_flagged_u8: stack entries with a crossed interval -> k_resolve_crossings, povu_hip_last_crossings
	PW_N_CROSSED = 12,   // k_resolve_crossings: crossings resolved in place -> povu_hip_last_crossings
	PW_RANK_OVF = 13,    // rank_events (list_rank.hip, the pre-order ranking): records whose partial sum left its 16 bits (its fallback kernel)
	PW_INCNT_OVF = 14,   // k_bracket_extra: a byte of incnt8 would have passed 255 -> the host (place_brackets: the pass is repeated with words)
	PW_LSZ_SAT = 15,     // k_count_saturated (on demand, behind the pass): stack entries whose list size did not fit the payload's field (LszField) -> povu_hip_last_lsz_field
	PASS_WORDS = 16	     // words carved and cleared (1, 3: unused)
};

// The payload of the black-only class sort: the stack index of an entry in the low `abits` bits and, above them, the size of
// its bracket list in `w` bits, saturating at lmax.  A size below lmax is all a reader needs; a saturated one (>= lmax) is
// looked up in ParWs::lsz, which k_top_bracket<true> writes for those entries only.  The sort looks at key bits and is
// stable, so the payload is opaque to it.  w = the bits a stack index below S leaves free, at most `cap`; w = 0 (lmax = 0):
// every entry is saturated and the payload is the bare index -- the form every pass had before, so no graph is refused.
struct LszField {
	unsigned w, abits; // abits = 32 - w >= 24
	uint32_t lmax;	   // 2^w - 1
	__host__ __device__ constexpr uint32_t mask() const { return 0xFFFFFFFFu >> w; }
	// (two shifts: abits = 32 must give 0, and a shift by the full width is undefined)
	__host__ __device__ constexpr uint32_t pack(uint32_t at, uint32_t live) const { return at | (((live < lmax ? live : lmax) << 1) << (abits - 1)); }
	__host__ __device__ constexpr uint32_t index(uint32_t u) const { return u & mask(); }
	__host__ __device__ constexpr uint32_t size(uint32_t u) const { return (u >> 1) >> (abits - 1); }
};
constexpr LszField lsz_field(uint64_t S, unsigned cap = LSZ_FIELD_CAP)
{
	unsigned b = 1; // bits_for(S), common.hpp
	while (b < 32 && (uint64_t(1) << b) <= S)
		b++;
	const unsigned w = 32 - b < cap ? 32 - b : cap;
	return LszField{w, 32 - w, (uint32_t(1) << w) - 1};
}
static_assert(lsz_field(1).w == 8 && lsz_field(1).abits == 24 && lsz_field(1).lmax == 255, "the cap");
static_assert(lsz_field((1u << 24) - 1).w == 8 && lsz_field(1u << 24).w == 7 && lsz_field(1u << 24).abits == 25, "S = 2^24");
static_assert(lsz_field((1u << 27) - 1).w == 5 && lsz_field(1u << 27).w == 4 && lsz_field(1u << 27).lmax == 15, "S = 2^27 - 1, 2^27");
static_assert(lsz_field(1u << 29).w == 2 && lsz_field(1u << 29).mask() == 0x3FFFFFFFu, "S = 2^29");
static_assert(lsz_field(0xFFFFFFFFull).w == 0 && lsz_field(0xFFFFFFFFull).lmax == 0 && lsz_field(0xFFFFFFFFull).mask() == 0xFFFFFFFFu, "S = 2^32 - 1: no field");
static_assert(lsz_field(0xFFFFFFFFull).pack(0xFFFFFFFEu, 7) == 0xFFFFFFFEu && lsz_field(0xFFFFFFFFull).size(0xFFFFFFFEu) == 0, "no field: the bare index");
static_assert(lsz_field(1u << 24, 3).w == 3 && lsz_field(1u << 29, 3).w == 2 && lsz_field(5, 0).w == 0, "a lower cap");
static_assert(lsz_field(1u << 27).pack((1u << 27) - 1, 99) == 0xF7FFFFFFu && lsz_field(1u << 27).index(0xF7FFFFFFu) == (1u << 27) - 1 && lsz_field(1u << 27).size(0xF7FFFFFFu) == 15, "the largest index under a saturated size");

// One more bracket ends at tree vertex t; returns the count in front of it.  A byte is incremented by a 32-bit atomic add of
// 1 << 8 (t & 3) on its aligned word (ParWs::incnt8 is 16-byte aligned): no carry leaves a byte that stays below 256.
__device__ __forceinline__ uint32_t incnt_add(uint32_t *incnt, uint32_t t) { return atomicAdd(&incnt[t], 1u); }
__device__ __forceinline__ uint32_t incnt_add(uint8_t *incnt, uint32_t t)
{
	const unsigned sh = 8u * (t & 3u);
	return (atomicAdd(reinterpret_cast<uint32_t *>(incnt + (t & ~3u)), 1u << sh) >> sh) & 0xFFu;
}
// ... and taken back (the add found the byte at 255)
__device__ __forceinline__ void incnt_take_back(uint8_t *incnt, uint32_t t)
{
	atomicSub(reinterpret_cast<uint32_t *>(incnt + (t & ~3u)), 1u << (8u * (t & 3u)));
}

// The outcome of a pass as k_summary writes it into page-locked host memory, one view for the kernel and every reader:
// ERR_WORDS error words, then bad[C], status[C], npvst[C], nbry[C], doff[C+1].
struct PassSummary {
	enum Err : uint32_t { NO_BRACKET = 0, WALK_POOL = 1, FOREST_SIZE = 2, SPARE = 3, ERR_WORDS = 4 }; // (SPARE: always 0, keeps bad[] 16-byte aligned)
	uint32_t C;
	uint32_t *w;
	__host__ __device__ PassSummary(uint32_t C_, const uint32_t *w_) : C(C_), w(const_cast<uint32_t *>(w_)) {}
	__host__ __device__ static size_t words(uint32_t C) { return ERR_WORDS + 5 * (size_t)C + 1 + 3; } // (three words of slack)
	__host__ __device__ uint32_t &err(uint32_t k) const { return w[k]; }
	__host__ __device__ uint32_t &bad(uint32_t c) const { return w[ERR_WORDS + c]; } // the component must be redone sequentially
	__host__ __device__ uint32_t &status(uint32_t c) const { return w[ERR_WORDS + (size_t)C + c]; }
	__host__ __device__ uint32_t &npvst(uint32_t c) const { return w[ERR_WORDS + 2 * (size_t)C + c]; }
	__host__ __device__ uint32_t &nbry(uint32_t c) const { return w[ERR_WORDS + 3 * (size_t)C + c]; }
	__host__ __device__ uint32_t &doff(uint32_t c) const { return w[ERR_WORDS + 4 * (size_t)C + c]; } // c <= C: first dense PVST slot
	__host__ __device__ uint32_t total() const { return doff(C); } // PVST vertices of all processed components
};

// (arrays that a pass also uses under another type or meaning: see ClassViews in par_kernels.hip, the one place that names them)
struct ParWs {
	HostScratch *host; // pinned read-back scratch of the owning context
	uint32_t V, E, C, T;
	bool all_vertex_classes = false; // in: number the classes of all tree edges even when the black ones would do (A/B tests)
	bool check_laminar = false;	 // in: run the laminarity check of the candidate stack even when the class stage was exact
	bool laminar_checked = false;	 // out: the last pass ran it
	bool black_only_used = false;	 // out: the last pass numbered the classes of the black tree edges only
	int prefix_records = 0;		 // out: it read count records (common.hpp) for: bit 0 psin, bit 1 the bracket range starts
	LszField lsz_field{0, 32, 0};	 // out: the payload format of the last black-only class sort (w = 0 also behind an all-vertices pass)
	bool s_cls_valid = false;	 // s_cls holds class ids (a black-only pass numbers its classes only when a debug hook asks)
	bool gcls_valid = false;	 // gcls holds the classes in T-space (a black-only pass keeps them in stack order only)
	// T-space (global tree vertex idx)
	uint32_t *t_comp, *t_root, *gpar, *gsize;
	uint32_t *hi0, *cov, *psA, *psB, *flagC, *psC; // exclusive scans of the byte flags below [T+1]; flagC: run marks
	uint8_t *f8a, *f8b, *f8c, *f8d; // [T+1] one-byte flags (bridge / simplifying / capping / branching vertex, class and stack flags)
	uint32_t *cap_tgt, *mpre, *dlt, *dlt_ps, *incnt, *psin, *topi, *lsz, *gcls;
	// The two bracket counts per tree vertex between the tree stage's emit kernel and the placing of the brackets, as BYTES
	// [T+2]: ordcnt8 (ordinary back edges leaving a vertex: k_tree_emit / k_back_edges -> the difference scan, k_bracket_extra)
	// lies in the first quarter of lsz, srccnt8 (brackets per mirror pre-order position: k_tree_emit / k_bracket_extra ->
	// the scan of the range starts) in the first quarter of dlt.  Those are the two word arrays that hold the same counts
	// in the wide form, so neither has another user in that stretch: lsz is next written by k_top_bracket, dlt by row E.
	// A pass uses them when no count can reach 256 (narrow_*: set by the caller ahead of the tree stage from the most
	// links any side has; srccnt <= ordcnt + 2); otherwise the word kernels run.
	uint8_t *ordcnt8, *srccnt8;
	bool narrow_ordcnt = false, narrow_srccnt = false; // in (srccnt only together with ordcnt)
	// The third count, incnt (brackets that END at a tree vertex), as bytes [T+2] in the first quarter of incnt itself: cleared by
	// k_tree_emit, counted into by k_back_edges / k_bracket_extra (incnt_add), last read by the scan of place_brackets; the
	// next writer of those words is k_tree_emit of the next pass.  The byte form leaves out every bracket that ends at a ROOT
	// -- the tips' back edges and the simplifying brackets, millions on one word -- because nothing reads a root's count: the
	// two scans of it are only ever read as differences over the subtree of a vertex WITH a parent (pscov in k_bridge_flags,
	// psin in k_top_bracket), and a root is in no such subtree.  Away from the roots the ordinary back edges that end at a
	// vertex are at most the links of its side, which the gate of narrow_ordcnt bounds; the capping brackets that share a
	// target are not bounded by anything, so k_bracket_extra looks at the byte its add returns, takes the add back at 255 and
	// raises PW_INCNT_OVF: place_brackets then gives up and the caller repeats the pass with words.
	uint8_t *incnt8;
	bool narrow_incnt = false; // in (only together with the other two)
	uint32_t *sdl;		 // [V+2] row E's difference array (k_shift_delta) when the tree stage's emit kernel already filled it
	bool sdl_filled = false; // ... which it says here
	uint32_t *vals_t, *vals_t2;
	uint32_t *keys_t, *keys_t2; // [T]
	// dense back edges / brackets
	uint32_t *dbo;			 // [C+1]
	uint32_t *b_src, *b_tgt, *b_val, *b_val2, *tgtR, *b_ord; // [NBmax]; b_ord = rank among the source's ordinary edges, bottom first
	uint32_t *b_key, *b_key2;	 // [NBmax] (only behind a sequential tree stage)
	size_t nb_cap = 0;		 // entries the bracket arrays were carved for
	// candidate stack space
	uint32_t *s_vtx, *s_cls, *ns, *prev; // [V+1] (prev: only written when the laminarity check runs or all vertices get a class)
	uint32_t *soff;				     // [C+1] first stack entry of a component (host-built table, set by the caller)
	uint32_t *walk, *walk_ps, *wrun; // [V+2] steps of the stack machine (one per entry), their prefix sums, running minimum (complemented)
	uint32_t *lev, *e_i;		 // [V+1]
	// two bit-rank directories over the stack positions (common.hpp), (n_stack / 64 + 2) records each: erec counts the entries
	// that open a flubble in front of a position, crec has a bit where a non-empty component starts; clist [C] names those
	// components in order (StackComp), rk_cnt is the scratch of bitrank_build
	uint4 *erec, *crec;
	uint32_t *clist, *rk_cnt;
	StackComp stack_comp() const { return StackComp{crec, clist}; }
	uint32_t *comp_bad;		 // [C+1] components that must be redone sequentially
	// dense PVST output (all processed components back to back): what goes over PCIe
	uint32_t *cproc_ps, *doff;	 // [C+1] processed components before c; first dense PVST slot of c
	size_t d_total;			 // PVST vertices of all processed components (dense output)
	uint32_t n_stack;		 // candidate-stack entries of the last pass
	uint32_t nb0 = 0, ncap = 0, nsimp = 0; // out: ordinary / capping / simplifying back edges of the last pass (b_src / b_tgt hold them in that order)
	uint32_t n_emitted = 0;		 // out: flubbles the last pass emitted (e_i / lev hold one entry each)
	uint32_t *d_a, *d_z, *d_parent;	 // [d_total] device views into the forest's page-locked result block
	uint8_t *d_aor, *d_zor;		 // [d_total] 0 forward, 1 reverse
	void *stage;			 // device block with the layout of the result block (large results are copied out by the DMA engine)
	uint32_t *err;			 // [PASS_WORDS] counters and internal error words of the pass (PassWord)
	SegTree segA, segB, segP, segL;
	// --hairpins on the parallel path
	uint8_t *hpf;			 // [T] bit0 simplifying vertex, bit1 top bracket is a simplifying edge
	uint32_t *hp1, *hp2, *hp3;	 // [T+1] segment-tree inputs / push flags
	unsigned long long *hp_b12;	 // [2T] boundary pairs before they are compacted
	SegTree segH1, segH2, segH3;
	void *scan_tmp, *sort_tmp;
	size_t scan_tmp_bytes, sort_tmp_bytes;
};

// second stream of a context + the two events that fork it from / join it to the main stream
struct SideStream {
	hipStream_t stream = nullptr;
	hipEvent_t fork = nullptr, join = nullptr;
	hipEvent_t fork2 = nullptr; // main -> side a second time: the PVST parents are ready for their copy
};

// The end of a pass (run_parallel_dg).  The pass reads everything the host needs to build the forest's tree table
// back TOGETHER with the PVST count (one synchronisation), so nothing but the PVST arrays themselves is still in
// flight when run_parallel_dg returns: the emit kernels and the copies of the finished arrays to the host, ALL of the
// copies on the side stream.  `done` is recorded behind the last of them.  With want_overlap the main stream does not
// wait for the side stream: the caller may start the next pass on it while the copy engine still moves this one's
// result over PCIe (povu_hip_decompose: POVU_HIP_F_ASYNC).
struct PassTail {
	bool want_overlap = false;		 // in
	hipEvent_t done = nullptr;		 // in: recorded when all work of the pass (kernels and copies) is complete
	hipEvent_t done2 = nullptr;		 // in: a second event recorded at the same point (the context's own)
	const uint32_t *early_summary = nullptr; // out: pass_summary's words (PassSummary) in page-locked host memory, as of the PVST count
	bool summary_final = false;		 // out: nothing after the count changes them (no laminarity check ran)
	bool overlapped = false;		 // out: the main stream was left free (want_overlap and summary_final)
};

// What a pass will NOT need is not carved (the arrays' pointers are then null): the default is everything.
struct StageWsOpts {
	size_t nb_cap = 0;	     // brackets the pass can have at most (0: the loose bound E + V + T)
	bool full_t = true;	     // per-vertex component / root / parent / size tables: a sequential tree stage or the hairpin report
	bool sorted_brackets = true; // keys of the bracket sort: only behind a sequential tree stage
	bool hairpins = true;	     // the hairpin report's arrays
	bool walk_inline = true;     // the wave walk's records / stack pool / parents inside the tree stage's block (else taken from
				     // TreeWs::walk_arena when a pass has large classes)
};
// groups: bit 0 = the arrays the tree stage already writes, bit 1 = those first written by the class stage (see for_each_span)
size_t par_workspace_bytes(size_t V, size_t E, size_t Cmax, int groups = 3, const StageWsOpts &o = StageWsOpts{});
void par_carve(Arena &ar, ParWs &pw, size_t V, size_t E, size_t Cmax, int groups = 3, const StageWsOpts &o = StageWsOpts{});

// Runs rows D-G for every processed component from the spanning trees / back edges the tree stage
// left in `sw`.  Components whose candidate stack is not laminar are flagged in pw.comp_bad (see pass_summary).
// dense_nb0 < 0: densify the back edges the sequential tree stage wrote; otherwise b_src/b_tgt hold them -- NB0_ON_DEVICE:
// their number still sits in pw.err[PW_NB0] (the parallel tree stage does not wait for it: the class stage reads it with the
// capping / simplifying counts, one host synchronisation instead of two).
// alloc_result_block(total) returns the device view of a page-locked host block laid out a | z | parent | a_or |
// z_or (each padded to 64 B) for `total` PVST vertices; the emit kernels write into it.
// Returns false when the pass kept incnt as bytes (ParWs::narrow_incnt) and one of them would have passed 255: nothing
// behind the placing of the brackets has run, and the caller runs the tree stage and this again with narrow_incnt off.
static constexpr int64_t NB0_ON_DEVICE = int64_t(1) << 40;
bool run_parallel_dg(const CompState &cs, SeqWs &sw, ParWs &pw, uint32_t C, uint32_t n_processed, uint32_t n_stack,
		     int64_t dense_nb0, const PassHooks &hooks, const std::function<void *(size_t)> &alloc_result_block, StageTimer &tm,
		     hipStream_t s, const SideStream &side, PassTail &tail);

// Hairpin boundaries (`--hairpins`, flubbles.cpp:531-535, 621-656, 712-717) from the parallel class stage's
// per-vertex flags; writes sw.hairpins / sw.c_nbry like the sequential kernels do.
void run_parallel_hairpins(const CompState &cs, SeqWs &sw, ParWs &pw, uint32_t C, StageTimer &tm, hipStream_t s);

// Copies the candidate stack / classes / next_seen of the last parallel pass into the per-component layout the
// debug hooks (and the sequential kernels) use; not needed by the pass itself.
// debug hook after a black-only pass: the classes of the black tree vertices into pw.gcls (NIL elsewhere)
void classes_to_tree_space(ParWs &pw, hipStream_t s);
// debug hook after a black-only pass: the stack entries whose list size filled the payload's field (LszField), counted from the
// sorted order the pass left behind into pw.err[PW_LSZ_SAT]; 0 behind any other pass
uint32_t count_saturated(ParWs &pw, hipStream_t s);
void export_parallel_stack(const CompState &cs, SeqWs &sw, ParWs &pw, hipStream_t s);

// One launch that writes the outcome of a pass into page-locked host memory (PassSummary::words(C) words, read through
// PassSummary).  pw == nullptr (sequential-only pass): error words, bad and doff read as 0.  The caller synchronises.
void pass_summary(const SeqWs &sw, const ParWs *pw, uint32_t C, uint32_t *host_out, hipStream_t s);

} // namespace povu_hip
