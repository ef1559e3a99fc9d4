// tree_kernels.hpp -- parallel spanning tree (row C), see tree_kernels.hip
#pragma once
#include "common.hpp"
#include "graph_kernels.hpp"
#include "list_rank.hpp"
#include "par_kernels.hpp"
#include "seq_kernels.hpp"

namespace povu_hip
{

// (arrays that a pass also uses under another type or meaning: see TreeViews in tree_kernels.hip, the one place that names them)
struct TreeWs {
	HostScratch *host; // pinned read-back scratch of the owning context
	// unrooted spanning forest of the biedged graph H, as arcs
	uint2 *dist;					  // [2E] level-0 records of the adjacency slots in the Euler-tour ranking, as two planes of 2E words (slots of hooked links = arcs; a slot's rank, the arcs behind it: rank_l0 of rec_decode, see list_rank.hpp)
	ulonglong2 *xval, *xps;				  // [max(V, E) + 16] xor values (two 64-bit hashes) of the segments that have any, in tour order, and their running xor (inside the shared block, see tree_spans)
	uint4 *xrec;					  // [(4V+8)/64 + 4] per 64 tour positions {which of them carry a value (64 bits), set bits in front of the word, -}: a bit-rank directory (common.hpp)
	uint32_t *xrank;				  // [(4V+8)/64 + 4] scan buffer of bitrank_build (the entry behind the last word: the number of values)
	uint4 *t0seg;					  // [V] rooted forest, per segment: {parent of the entered side, link to it | r bit, tour position in, out}
	uint2 *dps;					  // [2V] {DFS parent side, scan slot of the parent it was found through}
	uint8_t *dvis;					  // [2V]
	// the wave-cooperative walk of large 2-edge-connected classes
	uint32_t *wadj;					  // [2V + 2E] class-filtered scan lists (sides), deg + 1 slots per side
	uint4 *wrec;					  // [2 x 2V] 32-byte record per side: {count, list begin, first six candidates}
	uint2 *wstk;					  // [3 x 2V] pool of the walks' stacks {side, next candidate}
	uint32_t *wpar;					  // [2V] DFS parent of a side the walk reached, W_UNVIS before
	uint8_t *dvis_slots;				  // [2E] slot repeats an earlier link of its side (hub graphs)
	uint32_t *entry_ps, *entry_list;		  // [2V+1]
	uint32_t *side_tidx;				  // [2V] tree vertex (T-space) of a side
	uint32_t *be_cnt;				  // [2V+1] first arc of a side (tour); free afterwards
	RankBufs rk;					  // list ranking (list_rank.hpp): packed list words pk [4V+8] (between the first ranking and k_events: the far sides' stretches, [V] 8-byte records), list heads [C], the six pools of the levels above the list itself
	uint2 *evt;					  // [4V+2] level-0 records of the pre-order ranking's events, as two planes of 3V words (ranks {enter count, depth}: rank_l0_pair of rec_decode)
	uint32_t *cproc;				  // [C+1] 1 = component is decomposed by this shard
	const uint8_t *last_dupflag;			  // dvis_slots when the last pass filled it, else null
	bool tour_words_done = false;			  // tree_tour_words ran for this pass already (started ahead of the host's wait for the component sizes)
	hipStream_t walk_stream = nullptr; // second stream of the wave walks (the context's; null: both forms on the pass's stream)
	hipEvent_t walk_fork = nullptr, walk_join = nullptr;
	Arena *walk_arena = nullptr;			  // where the wave walk's arrays are taken from when the pass needs them and they are not inside the stage block
	bool walk_inline = true;
	RankRecStats rec_stats[2];			  // the tour's and the events' records of the last pass (collected only when PassHooks::rank_stats asks)
};

// groups: bit 0 = the arrays that outlive the tree stage, bit 1 = those that are dead when the class stage starts (tree_spans)
size_t tree_workspace_bytes(size_t V, size_t E, size_t Cmax, int groups = 3, const StageWsOpts &o = StageWsOpts{});
void tree_carve(Arena &ar, TreeWs &tw, size_t V, size_t E, size_t Cmax, int groups = 3, const StageWsOpts &o = StageWsOpts{});
// both parallel stages in one arena, the class stage's own arrays over the tree stage's dead ones
size_t stage_workspace_bytes(size_t V, size_t E, size_t Cmax, const StageWsOpts &o = StageWsOpts{});
void stage_workspace_carve(Arena &ar, ParWs &pw, TreeWs &tw, size_t V, size_t E, size_t Cmax, const StageWsOpts &o = StageWsOpts{});
// the wave walk's arrays (records of all sides, stack pool, parents): only a pass with large 2-edge-connected classes needs them
size_t walk_workspace_bytes(size_t V);

// the tree stage's first kernel (Euler-tour words of the spanning forest): it reads the re-indexed adjacency only, so
// povu_hip_decompose may start it before the host has the component sizes; run_parallel_tree then skips it
void tree_tour_words(const CompState &cs, uint32_t V, uint32_t E, TreeWs &tw, hipStream_t s);

// Builds the reference's spanning tree of every processed component (tree arrays in sw, T-space
// layout) and the dense list of from_bd back edges (pw.b_src / pw.b_tgt).  Returns their count.
int64_t run_parallel_tree(const CompState &cs, SeqWs &sw, ParWs &pw, TreeWs &tw, uint32_t C, uint32_t max_side_links,
			   bool force_big_class_dfs, bool force_sparse_splitters, const PassHooks &hooks, StageTimer &tm, hipStream_t s);

// back edges from_bd creates just before each tree vertex (w, T-space) and after the last child of each (tail, T-space); both
// arrays must be zeroed by the caller.  Reads the state of the last run_parallel_tree.  Callers: the leaf passes and the
// inserting passes of -s, and the conformance export (debug_hooks.hip).
void edge_id_weights(const CompState &cs, const SeqWs &sw, const TreeWs &tw, uint32_t *w, uint32_t *tail, hipStream_t s);

} // namespace povu_hip
