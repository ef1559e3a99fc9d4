// context.hpp -- the objects behind the opaque handles of include/povu_hip.h (shared by the .hip files that
// implement the C ABI).
#pragma once
#include "../../../include/povu_hip.h"

#include "forest_wire.hpp"
#include "graph_kernels.hpp"
#include "leaf_kernels.hpp"
#include "par_kernels.hpp"
#include "seq_kernels.hpp"
#include "sub_kernels.hpp"
#include "tree_kernels.hpp"

#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>

using namespace povu_hip;

// Pinned host blocks for the PVST arrays: D2H into page-locked memory runs at PCIe speed, and a
// block returns to its context's pool when the forest is freed (steady state: no allocation).
// In SHARED mode (povu_hip_share_results) a block is a POSIX shared-memory segment "/povu.<tag>.<k>", page-locked and
// mapped for the device with hipHostRegister: another process of the node maps it by name and reads the PVST arrays where
// this GPU's copy engine put them -- a multi-process gather without a second trip over PCIe (shard.hip).
struct PinnedPool {
	struct Block {
		void *p;
		size_t cap;
		int seg; // shared mode: k of the segment name, else -1
	};
	std::mutex m;
	std::vector<Block> free_blocks;
	std::vector<Block> segments; // every segment this pool created (shared mode): unmapped and unlinked with the pool
	std::string shared_tag;	     // empty: plain hipHostMalloc blocks
	int next_seg = 0;
	~PinnedPool();
	void *get(size_t bytes, size_t &cap, int *seg = nullptr);
	void put(void *p, size_t cap, int seg = -1)
	{
		std::lock_guard<std::mutex> g(m);
		if (seg >= 0 || free_blocks.size() < 24) // (a gather on 8+ ranks cycles through one block per rank)
			free_blocks.push_back(Block{p, cap, seg}); // (a segment stays mapped until the pool goes)
		else
			(void)hipHostFree(p);
	}
	static std::string segment_name(const std::string &tag, int k) { return "/povu." + tag + "." + std::to_string(k); }
};

// A host array whose memory comes out of the context's pool of page-locked blocks when it is given one (the label arrays of
// -s: 9 bytes per PVST vertex -- as pageable std::vectors their copy off the device took 10 - 30 ms on the whole-genome
// workload, depending on what the allocator made of 220 fresh megabytes), else from malloc.  Just enough of std::vector's
// surface for the code that uses it; resize() does not initialise (every caller overwrites).
template <typename T>
struct PinnedVec {
	T *p = nullptr;
	size_t n = 0, cap_bytes = 0;
	int seg = -1;
	std::shared_ptr<PinnedPool> pool; // null: malloc
	PinnedVec() = default;
	PinnedVec(const PinnedVec &) = delete;
	PinnedVec &operator=(const PinnedVec &) = delete;
	PinnedVec(PinnedVec &&o) noexcept { *this = std::move(o); }
	PinnedVec &operator=(PinnedVec &&o) noexcept
	{
		if (this != &o) {
			release();
			p = o.p, n = o.n, cap_bytes = o.cap_bytes, seg = o.seg, pool = std::move(o.pool);
			o.p = nullptr, o.n = 0, o.cap_bytes = 0, o.seg = -1;
		}
		return *this;
	}
	~PinnedVec() { release(); }
	void release()
	{
		if (p) {
			if (pool)
				pool->put(p, cap_bytes, seg);
			else
				free(p);
		}
		p = nullptr, n = 0, cap_bytes = 0, seg = -1;
		pool.reset();
	}
	void resize(size_t m, const std::shared_ptr<PinnedPool> &from = nullptr)
	{
		release();
		if (!m)
			return;
		if (from && from->shared_tag.empty()) { // (a pool of named shared-memory segments keeps them for the PVST blocks)
			pool = from;
			p = static_cast<T *>(pool->get(m * sizeof(T), cap_bytes, &seg));
		} else {
			p = static_cast<T *>(malloc(m * sizeof(T)));
			if (!p)
				throw std::bad_alloc();
		}
		n = m;
	}
	void assign(size_t m, T v)
	{
		resize(m);
		std::fill(p, p + m, v);
	}
	void assign(const T *a, const T *b)
	{
		resize((size_t)(b - a));
		if (n)
			memcpy(p, a, n * sizeof(T));
	}
	T *data() { return p; }
	const T *data() const { return p; }
	T *begin() { return p; }
	const T *begin() const { return p; }
	size_t size() const { return n; }
	bool empty() const { return n == 0; }
	T &operator[](size_t i) { return p[i]; }
	const T &operator[](size_t i) const { return p[i]; }
};

struct povu_hip_forest {
	uint32_t total_components = 0;
	// the pass that fills this forest: ev0 at its first kernel, ev1 behind its last copy.  `pending` while the arrays may
	// still be on their way (POVU_HIP_F_ASYNC); every accessor calls ready() first
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	bool pending = false;
	double pass_ms = -1.0;
	// a merged forest took over blocks whose arrays were still on their way: the events behind those passes (owned here)
	std::vector<hipEvent_t> more_events;
	// (may be reached from several threads at once -- the writer threads of `povu decompose` read one forest: the waits and
	// the pass time are taken exactly once, and the destructor goes through the same flag)
	std::once_flag ready_once;
	void wait_arrays()
	{
		if (pending) {
			if (ev1)
				(void)hipEventSynchronize(ev1);
			for (hipEvent_t e : more_events)
				(void)hipEventSynchronize(e);
			pending = false;
		}
	}
	void ready()
	{
		std::call_once(ready_once, [this] {
			wait_arrays();
			float ms = 0;
			if (ev0 && ev1 && pass_ms < 0 && hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess)
				pass_ms = ms;
		});
	}
	std::shared_ptr<PinnedPool> pool;
	size_t meta_reserve = 0; // trees a block leaves room for behind the arrays (povu_hip_forest_share writes their table there)
	static size_t meta_bytes(size_t n_trees) { return 64 + 32 * n_trees; }
	using Arrays = forest_wire::PvstArrays; // the five arrays of a block: a | z | parent | a_or | z_or
	static size_t block_bytes_for(size_t total) { return Arrays::layout(nullptr, total) + 64; } // (what a block takes on the wire)
	// The PVST arrays live in page-locked blocks: blocks[0] is the one the pass fills (a mixed pass: blocks[1] holds its redone
	// components); a merged forest holds the blocks it took over from other forests, received from other ranks or mapped
	// from their segments, so that merging never copies a PVST array.  With a block go the labels of
	// POVU_HIP_F_LEAF_SUBFLUBBLES (ai / zi, flubbles.cpp:264-290, and the line letter of every PVST vertex, indexed like the
	// arrays) and the trees after all five passes of -s.
	struct Block : Arrays {
		void *p = nullptr;
		size_t cap = 0, bytes = 0, total = 0; // of the memory / of the five arrays / PVST vertices
		int seg = -1;			  // shared-memory segment (PinnedPool shared mode), else -1
		std::shared_ptr<PinnedPool> pool; // null: the memory is not ours (a segment of another rank, mapped by the context)
		PinnedVec<uint32_t> sub_ai, sub_zi;
		PinnedVec<uint8_t> sub_fam;
		std::shared_ptr<SubForest> subx;
	};
	std::vector<Block> blocks;
	bool labels = false; // the blocks carry sub_ai / sub_zi / sub_fam
	// `q` (of `cap` bytes; null: out of the forest's pool, with room for the tree table) as a new block of `total` PVST vertices
	Block &alloc(size_t total, void *q = nullptr, size_t cap = 0)
	{
		Block b;
		b.total = total, b.p = q, b.cap = cap;
		if (!q) {
			b.pool = pool;
			b.p = pool->get(block_bytes_for(total) + meta_bytes(meta_reserve), b.cap, &b.seg);
		}
		b.bytes = Arrays::layout(b.p, total, &b);
		blocks.push_back(std::move(b));
		return blocks.back();
	}
	void release_blocks()
	{
		for (auto &b : blocks)
			if (b.p && b.pool)
				b.pool->put(b.p, b.cap, b.seg);
		blocks.clear();
	}
	~povu_hip_forest()
	{
		std::call_once(ready_once, [this] { wait_arrays(); }); // (the copy engine may still be writing the blocks)
		if (ev0)
			(void)hipEventDestroy(ev0);
		if (ev1)
			(void)hipEventDestroy(ev1);
		for (hipEvent_t e : more_events)
			(void)hipEventDestroy(e);
		release_blocks();
		if (xblk && pool)
			pool->put(xblk, xblk_cap, xblk_seg);
	}
	struct Tree : forest_wire::TreeRecord { // (off into the arrays of its block, hp_off into `hairpins` in pairs)
		int blk = 0; // its block
	};
	std::vector<Tree> trees;
	std::vector<uint64_t> hairpins;
	// povu_hip_forest_share: a second shared-memory segment with what the five arrays do not hold (labels, hairpin
	// boundaries, the extended trees of -s), kept alive as long as the forest
	void *xblk = nullptr;
	size_t xblk_cap = 0;
	int xblk_seg = -1;
	// povu_hip_forest_walks: the context and upload generation whose graph a povu_hip_decompose of the whole resident graph
	// (no shard) decomposed; merged, attached and sharded forests keep null / 0 and are refused
	const void *walk_ctx = nullptr;
	uint64_t walk_gen = 0;
};

// What a pass does, decided once from its options and the environment hooks (plan_pass in povu_hip.hip).
// all_seq: every stage on the one-lane kernels; seq_tree / par_tree: the tree stage on the one-lane / parallel kernels;
// leaf_sub: the leaf subflubble passes (find_tiny, find_parallel); all_sub: all five passes of -s; timed: stage times;
// overlap_tail: POVU_HIP_F_ASYNC on the one pass that has that form (the tail may overlap the next pass); heaviest_first:
// components in LPT order (shard assignment, launch order of the one-lane kernels); hooks: the A/B and tuning hooks of the
// environment as this pass read them (pass_hooks.hpp).
struct PassPlan {
	uint32_t rank = 0, world = 1;
	bool hairpins = false, all_seq = false, seq_tree = false, par_tree = true, leaf_sub = false, all_sub = false;
	bool sorted_adj = false, force_redo = false, redo_odd = false;
	bool big_class_dfs = false, sparse_splitters = false, all_vertex_classes = false, check_laminar = false;
	bool timed = true, overlap_tail = false, heaviest_first = false;
	PassHooks hooks;
};

// What the last decompose of a context left in its stage workspace (debug / parity hooks): with plan.par_tree the
// parallel tree stage's per-side state, unless plan.all_seq the classes in the parallel stage's own array (pw.gcls).
struct LastPass {
	bool valid = false; // false: no state, or a pass failed or something else has used the workspace since
	PassPlan plan;
	uint32_t C = 0, seq_redo = 0; // components, and those through the sequential redo
	// mixed: SOME components redone (the stage state is half parallel layout, half sequential); redo_pvst_only: the redo
	// only re-ran add_flubbles (tree, classes and stack are the parallel stages'); stack_export_pending: the parallel
	// stages' candidate stack is still in its dense layout
	bool mixed = false, redo_pvst_only = false, stack_export_pending = false;
	// the parallel stages kept the bracket counts per tree vertex (ordcnt / srccnt, see ParWs) as bytes
	bool narrow_counts = false;
	int narrow_forms = 0; // which of them: bit 0 ordcnt, bit 1 srccnt, bit 2 incnt
	int prefix_records = 0; // the class stage read count records for: bit 0 psin, bit 1 the bracket range starts
};

// Every device arena of a context besides the six of SubArenas, declared once: X(name, kind).  The list makes the members
// of povu_hip_ctx and its for_each_arena, so povu_hip_release_workspace, povu_hip_destroy and povu_hip_arena_report reach
// an arena because it exists.  ARENA_RESIDENT survives povu_hip_release_workspace, ARENA_WORKSPACE does not.
enum ArenaKind { ARENA_WORKSPACE = 0, ARENA_RESIDENT = 1 };
#define POVU_CTX_ARENAS(X)                                                                                                       \
	/* povu_hip_decompose: the stage workspaces (ws_b: what the re-index needs beyond the labelling's arrays; ws_leaf: the   \
	 * leaf passes of -s, kept from one -s pass to the next; ws_walk: the wave walk's arrays, taken by the first pass that   \
	 * meets large classes) */                                                                                               \
	X(ws, ARENA_WORKSPACE)                                                                                                   \
	X(ws_b, ARENA_WORKSPACE)                                                                                                 \
	X(ws2, ARENA_WORKSPACE)                                                                                                  \
	X(ws_seq, ARENA_WORKSPACE)                                                                                               \
	X(ws_leaf, ARENA_WORKSPACE)                                                                                              \
	X(ws_walk, ARENA_WORKSPACE)                                                                                              \
	X(upload_tmp, ARENA_WORKSPACE)                                                                                           \
	X(shard_buf, ARENA_RESIDENT)   /* a shard received from another rank */                                                  \
	X(graph_arena, ARENA_RESIDENT) /* backs the resident graph */                                                            \
	/* povu_hip_forest_walks (walk_kernels.hip): queries, counts and tier-2 stacks / the walks themselves */                 \
	X(wk_ws, ARENA_WORKSPACE)                                                                                                \
	X(wk_out, ARENA_WORKSPACE)                                                                                               \
	X(paths_buf, ARENA_RESIDENT) /* povu_hip_paths_upload: the paths of the resident graph */                                \
	/* povu_hip_forest_traversals (trav_kernels.hip): queries and the boundary table / scan tasks / traversals and dedup /   \
	 * allele steps */                                                                                                       \
	X(tr_ws, ARENA_WORKSPACE)                                                                                                \
	X(tr_task, ARENA_WORKSPACE)                                                                                              \
	X(tr_trav, ARENA_WORKSPACE)                                                                                              \
	X(tr_steps, ARENA_WORKSPACE)                                                                                             \
	X(seq_buf, ARENA_RESIDENT) /* povu_hip_segments_upload: the sequences of the resident graph */                           \
	/* povu_hip_call's workspace and outputs (call_kernels.hip) */                                                           \
	X(cl_ws, ARENA_WORKSPACE)                                                                                                \
	X(cl_slot, ARENA_WORKSPACE)                                                                                              \
	X(cl_rec, ARENA_WORKSPACE)                                                                                               \
	X(cl_spell, ARENA_WORKSPACE)                                                                                             \
	X(cl_bytes, ARENA_WORKSPACE)                                                                                             \
	/* povu_hip_call with POVU_HIP_T_INVERSIONS (inv_kernels.hip): the step index and head counts / the run heads, runs and  \
	 * records / the rows of the flubble records in the merged list */                                                       \
	X(iv_ws, ARENA_WORKSPACE)                                                                                                \
	X(iv_heads, ARENA_WORKSPACE)                                                                                             \
	X(iv_rows, ARENA_WORKSPACE)                                                                                              \
	X(nm_ws, ARENA_WORKSPACE) /* left-normalisation (norm_kernels.hip) */                                                    \
	/* the `decomposed` profile (prim_kernels.hip): the (record, ALT) pairs / the codes of the striped alignments / the      \
	 * rows */                                                                                                               \
	X(pr_ws, ARENA_WORKSPACE)                                                                                                \
	X(pr_slab, ARENA_WORKSPACE)                                                                                              \
	X(pr_rows, ARENA_WORKSPACE)                                                                                              \
	/* ... with POVU_HIP_T_MERGE (merge_kernels.hip): the grouping's scratch / the merged rows */                            \
	X(mg_ws, ARENA_WORKSPACE)                                                                                                \
	X(mg_rows, ARENA_WORKSPACE)                                                                                              \
	/* povu_hip_call with POVU_HIP_T_NESTED (nest_kernels.hip): the index of the called sites' traversals / the classes /    \
	 * the scratch of both / the records' parents, levels and the profile's choice */                                        \
	X(ns_idx, ARENA_WORKSPACE)                                                                                               \
	X(ns_cls, ARENA_WORKSPACE)                                                                                               \
	X(ns_ws, ARENA_WORKSPACE)                                                                                                \
	X(ns_rec, ARENA_WORKSPACE)                                                                                               \
	/* povu_hip_call with POVU_HIP_T_OFFREF (offref_kernels.hip): the sites' surrogates and the calling paths / the view of  \
	 * the calling paths / the inversion records' numbers among them / the host index and offers / the rows' arrays */       \
	X(or_ws, ARENA_WORKSPACE)                                                                                                \
	X(or_view, ARENA_WORKSPACE)                                                                                              \
	X(or_inv, ARENA_WORKSPACE)                                                                                               \
	X(or_host, ARENA_WORKSPACE)                                                                                              \
	X(or_rows, ARENA_WORKSPACE)                                                                                              \
	/* povu_hip_call with POVU_HIP_T_UNTANGLE (untangle_kernels.hip): the lap runs and the slots' cells / the entries and    \
	 * the task list / the tasks' row counts and offsets / the partner table / the rows' arrays */                           \
	X(un_ws, ARENA_WORKSPACE)                                                                                                \
	X(un_task, ARENA_WORKSPACE)                                                                                              \
	X(un_part, ARENA_WORKSPACE)                                                                                              \
	X(un_pair, ARENA_WORKSPACE)                                                                                              \
	X(un_rows, ARENA_WORKSPACE)                                                                                              \
	/* povu_hip_vcf_check (vcfcheck_kernels.hip): the step index, the uploaded walks, texts and tasks and the results / the  \
	 * table of (allele, slot) hits */                                                                                       \
	X(vc_ws, ARENA_WORKSPACE)                                                                                                \
	X(vc_hit, ARENA_WORKSPACE)                                                                                               \
	/* the packed shards of the last povu_hip_shard_partition (kept warm: a step of a sharded job re-partitions) */          \
	X(part_arena, ARENA_RESIDENT)

struct povu_hip_ctx {
	int device = 0;
	hipStream_t stream = nullptr;
	SideStream side; // PCIe-bound result writes run beside the main stream's kernels
	ResidentGraph g;
	SubArenas ws_sub; // tables of the inserting passes of -s, one arena per phase (sub_kernels.hpp); kept from one -s pass to the next
#define POVU_ARENA_MEMBER(name, kind) Arena name;
	POVU_CTX_ARENAS(POVU_ARENA_MEMBER)
#undef POVU_ARENA_MEMBER
	// every device arena of the context in declaration order, the six of ws_sub first (as "ws_sub.<name>", all workspace):
	// f(name, arena, kind); the name is only good during the call
	template <class Ctx, class F>
	static void visit_arenas(Ctx &c, F &&f)
	{
		c.ws_sub.for_each_arena([&](const char *n, auto &a) { f((std::string("ws_sub.") + n).c_str(), a, ARENA_WORKSPACE); });
#define POVU_ARENA_VISIT(name, kind) f(#name, c.name, kind);
		POVU_CTX_ARENAS(POVU_ARENA_VISIT)
#undef POVU_ARENA_VISIT
	}
	template <class F>
	void for_each_arena(F &&f) { visit_arenas(*this, f); }
	template <class F>
	void for_each_arena(F &&f) const { visit_arenas(*this, f); }
	HostScratch host;
	std::shared_ptr<PinnedPool> pool = std::make_shared<PinnedPool>();
	StageTimer timer;
	std::vector<povu_hip_stage_time> last_times;
	uint64_t last_links = 0;
	uint64_t wide_repeats = 0; // passes of this context that ran their tree and class stages a second time with word counts (ParWs::incnt8)
	// device state of the last decompose (debug / parity hooks)
	CompState cs{};
	SeqWs sw{};
	ParWs pw{};
	TreeWs tw{};
	LastPass last;
	// the records of the last povu_hip_debug_list_rank call: their statistics and the first word of every element's record
	RankRecStats dbg_rank_stats;
	std::vector<uint32_t> dbg_rank_plane0;
	// when the resident graph is a shard (povu_hip_graph_upload_shard): ids of its components in the whole graph
	// (1-based, ascending = the shard's own component order) and the component count of the whole graph
	std::vector<uint32_t> shard_comp_ids;
	uint32_t shard_total_components = 0;
	// the tail of the last POVU_HIP_F_ASYNC pass (side-stream kernels and copies that read the stage workspace): recorded
	// behind it; the next pass waits for it before it touches that workspace, every other entry point before anything
	hipEvent_t tail_done = nullptr;
	SideStream walk_side; // the wave walks' second stream (tree stage: the two forms of the walk run side by side)
	bool tail_pending = false;
	void wait_tail()
	{
		if (tail_pending) {
			(void)hipEventSynchronize(tail_done);
			tail_pending = false;
		}
	}
	void quiesce() // debug hooks: nothing of the last pass may still be running
	{
		if (tail_pending) {
			(void)hipStreamSynchronize(stream);
			wait_tail();
		}
	}
	// povu_hip_paths_upload: the paths of the resident graph, one word a step (vertex index << 1 | '<'), and their u64 step
	// offsets (in paths_buf); they belong to upload `paths_gen` (a later graph upload leaves them stale: refused)
	uint32_t *path_steps = nullptr;
	uint64_t *path_off = nullptr;
	uint32_t n_paths = 0;
	uint64_t n_path_steps = 0, paths_gen = 0;
	bool paths_valid = false;
	// povu_hip_segments_upload: the sequences of the resident graph (u64 offsets by vertex index, then the bytes; in seq_buf), of
	// upload `seq_gen`
	uint64_t *seq_off = nullptr;
	char *seq = nullptr;
	uint64_t seq_gen = 0;
	bool seq_valid = false;
	// bytes this context moved over PCIe / to peers since it was created (povu_hip_transfer_bytes)
	uint64_t xfer_h2d = 0, xfer_d2h = 0, xfer_peer_out = 0, xfer_peer_in = 0;
	// result segments of other ranks, mapped read-only by name (povu_hip_forest_attach); unmapped with the context
	struct Mapped {
		void *p;
		size_t bytes;
	};
	std::map<std::string, Mapped> attached;
};

// adds what the calling thread moved over PCIe during one C ABI call to the context's totals
struct XferScope {
	povu_hip_ctx *ctx;
	XferTally at;
	explicit XferScope(povu_hip_ctx *c) : ctx(c), at(xfer_tally()) {}
	~XferScope()
	{
		if (!ctx)
			return;
		const XferTally now = xfer_tally();
		ctx->xfer_h2d += now.h2d - at.h2d;
		ctx->xfer_d2h += now.d2h - at.d2h;
	}
};


// `m`'s blocks, trees, hairpin boundaries and events move into `out` (m is left empty); shard.hip
void adopt_forest(povu_hip_forest &out, povu_hip_forest &m);

// Greedy longest-processing-time assignment of n weighted components to `world` ranks, the same on every rank: `order`
// gets the components heaviest first (stable), owner[c] the least-loaded rank at c's turn (each component adds weight + 1).
static inline void lpt_assign(const uint64_t *weights, uint32_t n, uint32_t world, uint32_t *order, uint32_t *owner)
{
	std::iota(order, order + n, 0u);
	std::stable_sort(order, order + n, [&](uint32_t a, uint32_t b) { return weights[a] > weights[b]; });
	std::vector<uint64_t> load(world, 0);
	for (uint32_t k = 0; k < n; k++) {
		const uint32_t c = order[k];
		uint32_t best = 0;
		for (uint32_t r = 1; r < world; r++)
			if (load[r] < load[best])
				best = r;
		owner[c] = best;
		load[best] += weights[c] + 1;
	}
}

// device block of a resident graph (link arrays + CSR); build_global_csr fills the CSR part
void alloc_resident_graph(Arena &arena, ResidentGraph &g, uint32_t n_vtx, uint32_t n_links, bool tips_given);
void free_resident_graph(ResidentGraph &g);
void check_graph_size(uint32_t n_vtx, uint32_t n_links);
void set_err(char *err, size_t errlen, const std::string &msg);

struct Sizes {
	size_t V, E, Cmax, T, B, nS, slots; // (rows A/B are sized before the component count is known: Cmax = V, T = B = 0)
	void set_components(size_t C) { Cmax = C, T = 2 * V + C, B = E + V + 2 * T; }
};
// Rows A/B in two steps (povu_hip_decompose): before the components are labelled only what the labelling writes is carved
// (rowb_carve_label); what the re-index needs follows when the component count, the order of the vertices and the
// builder are known (rowb_carve_reindex, from a second arena) -- a graph whose vertices already come grouped by component,
// without hub vertices and self loops (a pangenome GFA), needs a quarter of what the general case does.
struct RowBNeeds {
	bool identity;	// one component, or the vertices already in (component, idx) order
	bool sort_free; // no hub vertex: the builder that needs no sort
	bool self_loops;
};
size_t rowb_carve_label(Arena *ar, const Sizes &z, CompState &cs);
size_t rowb_carve_reindex(Arena *ar, const Sizes &z, size_t C, const RowBNeeds &need, CompState &cs);
size_t rowb_speculative_adj_bytes(const Sizes &z);
// The head of a pass (povu_hip.hip), shared by povu_hip_decompose and povu_hip_debug_row_b: the plan the flags make,
// the set-up ahead of row B, and row B itself -- the component count at once, the components' sizes in page-locked scratch
// once `sizes` is waited for.
struct RowB {
	uint32_t C;
	const uint32_t *voff, *eoff, *gstats;
	HostScratch::Token sizes;
};
PassPlan plan_pass(const povu_hip_opts *opts);
Sizes rowb_begin(povu_hip_ctx *ctx, const PassPlan &p);
RowB row_b(povu_hip_ctx *ctx, const PassPlan &p, const Sizes &z, StageTimer &tm);
// Workspace carving (or just measuring when `ar` is null); part 0 = rows A/B state (CompState), see context.hip
size_t carve_workspace(Arena *ar, int part, const Sizes &z, CompState &cs, SeqWs &sw, bool hairpins);
// what the stage workspace of a pass has to hold (context.hip)
StageWsOpts stage_opts(size_t V, size_t E, size_t C, size_t empty_sides, bool seq_tree, bool hairpins);
