// povu_hip.hip -- the decompose pass behind the C ABI (include/povu_hip.h): the plan of a pass, its steps from row B to the
// result fetch, povu_hip_componetize, and what the last pass of a context reports.  Mirrors
// povu::subcommands::decompose::do_decompose (app/subcommand/decompose.cpp:94-160) from "graph built" to "PVST ready to
// write".  The context and its memory: context.hip; the accessors of a finished forest: forest.hip.
#include "context.hpp"

#include <algorithm>
#include <memory>
#include <numeric>

using namespace povu_hip;

// ---- povu_hip_decompose: the plan of a pass, then its steps
namespace
{

static const char *const SUB_REDO_REFUSAL = "subflubble passes: a component went (or was sent) through the sequential redo of add_flubbles, "
					    "whose PVST layout the inserting passes do not read";

} // namespace

// Every decision a pass takes from its options, in one place.  Refusals that depend on the flags alone are made here;
// those that depend on what the pass finds (a component the laminarity check flags) where it finds it.
PassPlan plan_pass(const povu_hip_opts *opts)
{
	povu_hip_opts o{0, 1, 0};
	if (opts)
		o = *opts;
	if (o.world == 0)
		o.world = 1;
	if (o.rank >= o.world)
		throw HipError("shard rank >= world");
	auto has = [&](uint32_t flag) { return (o.flags & flag) != 0; };
	PassPlan p;
	p.rank = o.rank, p.world = o.world, p.hairpins = has(POVU_HIP_F_HAIRPINS), p.timed = !has(POVU_HIP_F_NO_STAGE_TIMES);
	p.all_seq = has(POVU_HIP_F_SEQUENTIAL), p.seq_tree = has(POVU_HIP_F_SEQ_TREE), p.par_tree = !p.all_seq && !p.seq_tree;
	p.all_sub = has(POVU_HIP_F_SUBFLUBBLES), p.leaf_sub = p.all_sub || has(POVU_HIP_F_LEAF_SUBFLUBBLES);
	p.force_redo = has(POVU_HIP_F_FORCE_REDO), p.redo_odd = has(POVU_HIP_F_REDO_ODD), p.sorted_adj = has(POVU_HIP_F_SORTED_ADJ);
	p.big_class_dfs = has(POVU_HIP_F_BIG_CLASS_DFS), p.sparse_splitters = has(POVU_HIP_F_SPARSE_SPLITTERS);
	p.all_vertex_classes = has(POVU_HIP_F_ALL_VERTEX_CLASSES), p.check_laminar = has(POVU_HIP_F_CHECK_LAMINAR);
	p.hooks = read_pass_hooks(); // (once per pass: a caller may change the environment between two passes)
	// POVU_HIP_F_ASYNC: the pass may leave its last kernels and the copies of the PVST arrays in flight when it returns
	// (and the next pass may then start under them).  Only the plain all-parallel pass has that form.
	p.overlap_tail = has(POVU_HIP_F_ASYNC) && !p.timed && p.par_tree && !p.hairpins && !p.force_redo && !p.redo_odd && !p.leaf_sub &&
			 !p.check_laminar;
	// heaviest first: the shard assignment and the launch order of the one-lane kernels (the parallel stages do not care,
	// so a single-shard parallel pass skips the sort)
	p.heaviest_first = p.world > 1 || p.all_seq || p.seq_tree || p.force_redo;
	if (p.leaf_sub && (p.all_seq || p.seq_tree))
		throw HipError("the leaf subflubble passes read the state of the parallel stages: not with the sequential tree / all-sequential test modes");
	if (p.all_sub && (p.force_redo || p.redo_odd) && !p.hairpins) // (with --hairpins a flagged component is refused first, leaf_passes)
		throw HipError(SUB_REDO_REFUSAL);
	return p;
}

namespace
{
// The tail of the pass before (POVU_HIP_F_ASYNC) reads the stage workspace (ws2) from the side stream.  A pass that may
// itself overlap waits for it ON THE STREAM, right before its own first write there (carve_stages, component_tables);
// every other pass -- and any pass whose arenas must grow, which frees them -- waits on the host.
static void reserve(povu_hip_ctx *ctx, Arena &ar, size_t bytes)
{
	if (bytes > ar.capacity())
		ctx->wait_tail();
	ar.reserve(bytes);
}

} // namespace

// ---- what a pass sets up ahead of row B: the state of the pass before is forgotten, the pinned scratch rewound, the
// labelling's arrays carved (sized before the component count is known) and the stage timer armed
Sizes rowb_begin(povu_hip_ctx *ctx, const PassPlan &p)
{
	const ResidentGraph &g = ctx->g;
	const Sizes z{g.V, g.E, g.V, 0, 0, 2 * (size_t)g.V, g.n_slots}; // (rows A/B run before the component count is known)
	ctx->last = LastPass{};
	ctx->host.reset();
	ctx->cs.host = ctx->pw.host = ctx->tw.host = &ctx->host;
	reserve(ctx, ctx->ws, rowb_carve_label(nullptr, z, ctx->cs));
	rowb_carve_label(&ctx->ws, z, ctx->cs);
	ctx->timer.reset();
	ctx->timer.enabled = p.timed;
	return z;
}

// ---- row B: labelling, speculative adjacency, re-index
// The host has to know the component count (it sizes the workspaces) and then the components' sizes (the tables of the
// stages): two reads.  Neither is waited for with the stream idle: the words are published by a kernel, an event is
// recorded behind it (HostScratch::mark), and the stream is given its next kernel before the host waits for the event --
//  (1) behind the labelling: the re-index's adjacency kernel, on the assumption that holds for nearly every GFA (vertices
//      grouped by component, no hub, no self loop: it then needs nothing the labels say but the hooks; when the
//      assumption fails its output is simply overwritten by the real re-index);
//  (2) behind the re-index: the tree stage's first kernel (it reads the re-indexed adjacency only; carve_stages).
// Not with stage timers (the kernels would be booked on the wrong stage).
RowB row_b(povu_hip_ctx *ctx, const PassPlan &p, const Sizes &z, StageTimer &tm)
{
	const ResidentGraph &g = ctx->g;
	CompState &cs = ctx->cs;
	hipStream_t s = ctx->stream;
	uint32_t *lab = label_components_enqueue(g, cs, tm, s);
	const HostScratch::Token labelled = ctx->host.mark(s);
	bool spec_adj = false;
	if (!tm.enabled && g.E && sort_free_adjacency(g, p.sorted_adj) && ctx->ws_b.capacity() >= rowb_speculative_adj_bytes(z)) {
		ctx->ws_b.reserve(0); // (rewinds the arena: the two arrays get the places rowb_carve_reindex will give them)
		uint32_t *ladj = ctx->ws_b.take<uint32_t>(2 * z.E + 8), *lle = ctx->ws_b.take<uint32_t>(2 * z.E + 8);
		reindex_speculative_adj(g, cs, ladj, lle, s);
		spec_adj = true;
	}
	ctx->host.wait(labelled);
	const uint32_t C = label_components_finish(cs, lab);
	// what the re-index of THIS graph needs, now that the count, the order and the self loops are known
	const RowBNeeds need{C == 1 || cs.comp_sorted, sort_free_adjacency(g, p.sorted_adj), cs.has_self_loops};
	const size_t need_b = rowb_carve_reindex(nullptr, z, C, need, cs);
	if (spec_adj && need_b > ctx->ws_b.capacity()) { // the arena has to grow under a kernel that writes into it: let it finish, forget it
		HIP_CHECK(hipStreamSynchronize(s));
		spec_adj = false;
	}
	reserve(ctx, ctx->ws_b, need_b);
	rowb_carve_reindex(&ctx->ws_b, z, C, need, cs);
	spec_adj = spec_adj && need.identity && need.sort_free && !need.self_loops; // (else: a kernel that wrote nonsense into arrays about to be rewritten)
	// component sizes on the host (shard assignment, launch order): the last re-index kernel writes them into pinned
	// memory itself
	uint32_t *pub = ctx->host.take<uint32_t>(2 * ((size_t)C + 1) + 4);
	HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void **>(&cs.host_pub), pub, 0));
	count_kernel_d2h((2 * ((size_t)C + 1) + 4) * 4);
	reindex_components(g, cs, C, tm, s, p.sorted_adj, spec_adj);
	return RowB{C, pub, pub + (size_t)C + 1, pub + 2 * ((size_t)C + 1), ctx->host.mark(s)};
}

// ---- povu_hip_componetize: rows A/B alone, the components handed to the host
namespace
{
struct ComponentsOwner {
	povu_hip_components view{};
	std::vector<uint32_t> voff, eoff, vid, v1, v2;
	std::vector<uint8_t> tip, s1, s2;
};
} // namespace

extern "C" povu_hip_components *povu_hip_componetize(povu_hip_ctx *ctx, char *err, size_t errlen)
{
	try {
		if (!ctx || !ctx->g.block)
			throw HipError("no graph resident: call povu_hip_graph_upload first");
		HIP_CHECK(hipSetDevice(ctx->device));
		ctx->wait_tail();
		const ResidentGraph &g = ctx->g;
		hipStream_t s = ctx->stream;
		const Sizes z{g.V, g.E, g.V, 0, 0, 2 * (size_t)g.V, g.n_slots};
		CompState &cs = ctx->cs;
		SeqWs &sw = ctx->sw;
		ctx->last.valid = false;
		ctx->host.reset();
		cs.host = &ctx->host;
		cs.host_pub = nullptr;
		ctx->ws.reserve(carve_workspace(nullptr, 0, z, cs, sw, false));
		carve_workspace(&ctx->ws, 0, z, cs, sw, false);
		StageTimer &tm = ctx->timer;
		tm.reset();
		tm.enabled = true;
		const uint32_t C = label_components(g, cs, tm, s);
		reindex_components(g, cs, C, tm, s, true); // (the builder that numbers the local edges: la / lb in local edge order)
		if (!cs.dense_edges)
			throw HipError("componetize: local edges were not numbered (internal)");
		auto o = std::make_unique<ComponentsOwner>();
		const size_t V = g.V, E = g.E;
		o->voff.resize(C + 1);
		o->eoff.resize(C + 1);
		o->vid.resize(V);
		o->tip.resize(V);
		std::vector<uint32_t> la(E), lb(E);
		HIP_CHECK(copy_async(o->voff.data(), cs.voff, (size_t)(C + 1) * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(o->eoff.data(), cs.eoff, (size_t)(C + 1) * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(o->vid.data(), cs.gid_s, V * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(o->tip.data(), cs.tip_s, V, hipMemcpyDeviceToHost, s));
		if (E) {
			HIP_CHECK(copy_async(la.data(), cs.la, E * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(copy_async(lb.data(), cs.lb, E * 4, hipMemcpyDeviceToHost, s));
		}
		HIP_CHECK(hipStreamSynchronize(s));
		o->v1.resize(E);
		o->v2.resize(E);
		o->s1.resize(E);
		o->s2.resize(E);
		for (uint32_t c = 0; c < C; c++)
			for (uint32_t e = o->eoff[c]; e < o->eoff[c + 1]; e++) { // sorted side id = 2 * position + end
				o->v1[e] = (la[e] >> 1) - o->voff[c];
				o->s1[e] = (uint8_t)(la[e] & 1);
				o->v2[e] = (lb[e] >> 1) - o->voff[c];
				o->s2[e] = (uint8_t)(lb[e] & 1);
			}
		o->view = povu_hip_components{C, g.V, g.E, o->voff.data(), o->eoff.data(), o->vid.data(), o->tip.data(),
					      o->v1.data(), o->v2.data(), o->s1.data(), o->s2.data()};
		ComponentsOwner *raw = o.release();
		return &raw->view; // view is the first member: the owner is recovered from it in _free
	} catch (const std::exception &e) {
		set_err(err, errlen, e.what());
		return nullptr;
	}
}

extern "C" void povu_hip_components_free(povu_hip_components *c)
{
	delete reinterpret_cast<ComponentsOwner *>(c);
}

namespace
{
// ---- stage workspaces, sized with the real component count (z), and the tree stage's first kernel, which goes out
// before the host waits for the component sizes.  Returns whether the stream already waits for the tail of the pass before.
static bool carve_stages(povu_hip_ctx *ctx, const PassPlan &p, const Sizes &z, uint32_t C, const StageTimer &tm)
{
	const StageWsOpts so = stage_opts(z.V, z.E, C, ctx->g.n_empty_sides, p.seq_tree, p.hairpins);
	reserve(ctx, ctx->ws2, carve_workspace(nullptr, 1, z, ctx->cs, ctx->sw, p.hairpins) + (p.all_seq ? 0 : stage_workspace_bytes(z.V, z.E, C, so)));
	carve_workspace(&ctx->ws2, 1, z, ctx->cs, ctx->sw, p.hairpins);
	if (p.all_seq)
		return false;
	TreeWs &tw = ctx->tw;
	stage_workspace_carve(ctx->ws2, ctx->pw, tw, z.V, z.E, C, so);
	tw.walk_arena = &ctx->ws_walk;
	tw.walk_stream = ctx->walk_side.stream;
	tw.walk_fork = ctx->walk_side.fork;
	tw.walk_join = ctx->walk_side.join;
	tw.tour_words_done = false;
	if (!p.par_tree || tm.enabled)
		return false;
	if (ctx->tail_pending) // first write into the stage workspace: behind the tail of the pass before
		HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->tail_done, 0));
	tree_tour_words(ctx->cs, (uint32_t)z.V, (uint32_t)z.E, tw, ctx->stream);
	return ctx->tail_pending;
}

// What the component tables tell the stages.
struct CompTables {
	uint32_t n_stack = 0, n_processed = 0;
};

// ---- component tables: launch order, owner (LPT over vertices + links, the same on every rank), processed components
// (>= 3 vertices, owned by this shard) and their running count `pc` = where a component starts in the dense PVST output,
// and where each component's candidate stack starts.  Host-built in pinned scratch: the upload needs no synchronisation.
static CompTables component_tables(povu_hip_ctx *ctx, const PassPlan &p, uint32_t C, const uint32_t *voff, const uint32_t *eoff,
				   bool tail_waited)
{
	uint32_t *tab_h = ctx->host.take<uint32_t>(5 * ((size_t)C + 1));
	uint32_t *order = tab_h, *owner = tab_h + ((size_t)C + 1), *pc = tab_h + 2 * ((size_t)C + 1), *cproc = tab_h + 3 * ((size_t)C + 1),
		 *stack_off = tab_h + 4 * ((size_t)C + 1);
	if (p.heaviest_first) {
		std::vector<uint64_t> weight(C);
		for (uint32_t c = 0; c < C; c++)
			weight[c] = (uint64_t)(eoff[c + 1] - eoff[c]) + (voff[c + 1] - voff[c]);
		lpt_assign(weight.data(), C, p.world, order, owner);
	} else {
		std::iota(order, order + C, 0u);
		std::fill(owner, owner + C, 0u);
	}
	uint64_t links = 0;
	for (uint32_t c = 0; c < C; c++)
		if (owner[c] == p.rank || p.world == 1)
			links += eoff[c + 1] - eoff[c];
	ctx->last_links = links;
	CompTables t;
	order[C] = owner[C] = cproc[C] = 0;
	pc[0] = 0;
	for (uint32_t c = 0; c < C; c++) {
		const uint32_t nv = voff[c + 1] - voff[c];
		cproc[c] = (nv >= 3 && (p.world == 1 || owner[c] == p.rank)) ? 1u : 0u;
		pc[c + 1] = pc[c] + cproc[c];
		stack_off[c] = t.n_stack;
		t.n_stack += cproc[c] ? nv : 0u; // one candidate-stack entry per segment (its black tree edge)
	}
	stack_off[C] = t.n_stack;
	t.n_processed = pc[C];
	if (ctx->tail_pending && !tail_waited) // first write into the stage workspace: behind the tail of the pass before
		HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->tail_done, 0));
	HIP_CHECK(copy_async(ctx->sw.tables, tab_h, 5 * ((size_t)C + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
	return t;
}

// The one-lane kernels' lists live in their own arena, carved -- and emptied, as the kernels expect them -- only when a
// pass runs those kernels.
struct SeqLanes {
	povu_hip_ctx *ctx;
	const Sizes &z;
	bool hairpins;
	bool carved = false;
	void carve()
	{
		if (carved)
			return;
		ctx->wait_tail();
		ctx->ws_seq.reserve(carve_workspace(nullptr, 2, z, ctx->cs, ctx->sw, hairpins));
		carve_workspace(&ctx->ws_seq, 2, z, ctx->cs, ctx->sw, hairpins);
		carved = true;
	}
	void init(hipStream_t s)
	{
		carve();
		const SeqWs &sw = ctx->sw;
		for (uint32_t *p : {sw.first_child, sw.o_head, sw.i_head, sw.bl, sw.t_hi, sw.t_cls, sw.st_head, sw.st_tail})
			HIP_CHECK(hipMemsetAsync(p, 0xFF, z.T * 4, s));
		HIP_CHECK(hipMemsetAsync(sw.ctr, 0xFF, z.nS * 4, s));
		HIP_CHECK(hipMemsetAsync(sw.cur, 0, z.nS * 4, s));
		HIP_CHECK(hipMemsetAsync(sw.selfloop, 0, z.V, s));
		HIP_CHECK(hipMemsetAsync(sw.last, 0xFF, (z.B + z.T) * 4, s));
		HIP_CHECK(hipMemsetAsync(sw.in_s, 0, z.B + z.T, s));
	}
};

// What rows C-G leave for the result fetch and the record of the pass.
struct RowsOut {
	const uint32_t *sum = nullptr; // outcome of the pass in pinned memory (pass_summary); null: read it when the pass is done
	uint32_t nbad = 0;	       // components through the sequential redo
	bool mixed = false;	       // parallel result for most components, sequential redo for the flagged ones
	bool redo_pvst_only = false, stack_export_pending = false;
	bool fast_tail = false; // the summary came with the PVST count: nothing was synchronised after the tail was enqueued
	PassTail tail;
};

// pass_summary's words, read with the stream drained; f's ev1 goes behind them (recorded again if more work follows)
static const uint32_t *read_summary(povu_hip_ctx *ctx, uint32_t C, bool with_par, const povu_hip_forest &f)
{
	uint32_t *h = ctx->host.take<uint32_t>(PassSummary::words(C));
	count_kernel_d2h(PassSummary::words(C) * 4);
	pass_summary(ctx->sw, with_par ? &ctx->pw : nullptr, C, h, ctx->stream);
	HIP_CHECK(hipEventRecord(f.ev1, ctx->stream));
	HIP_CHECK(hipStreamSynchronize(ctx->stream));
	return h;
}

// ---- rows C-G on the parallel kernels (the tree on the one-lane kernels with POVU_HIP_F_SEQ_TREE), up to the count of
// the components the laminarity check flags; returns the bracket count given to the class stage (< 0: sequential tree)
static int64_t parallel_rows(povu_hip_ctx *ctx, const PassPlan &p, uint32_t C, const uint32_t *gstats, const CompTables &t,
			     povu_hip_forest &f, SeqLanes &lanes, StageTimer &tm, RowsOut &out)
{
	SeqWs &sw = ctx->sw;
	ParWs &pw = ctx->pw;
	hipStream_t s = ctx->stream;
	int64_t dense_nb0 = -1;
	pw.cproc_ps = sw.tables + 2 * ((size_t)C + 1);
	ctx->tw.cproc = sw.tables + 3 * ((size_t)C + 1);
	pw.soff = sw.tables + 4 * ((size_t)C + 1);
	pw.narrow_ordcnt = pw.narrow_srccnt = pw.narrow_incnt = false;
	// Bracket counts per tree vertex as bytes (ParWs::ordcnt8 / srccnt8 / incnt8) when none can reach 256: a vertex sends at most
	// one back edge per link of its side (one, to the root, from a side without links), and a position of the bracket list
	// holds at most a capping and a simplifying bracket more.  Otherwise -- a hub, a fat side of the dense re-index path -- the
	// word kernels run.  The brackets that END at a vertex away from the roots are bounded by the same gate but for the
	// capping brackets that share a target: the class stage says when a byte of incnt8 would have overflowed, and the tree
	// and class stages then run again with all three counts as words (wide_again).
	// PassHooks::wide_counts (A/B hook): 1 = words for all three, 2 = words for srccnt and incnt, 3 = for incnt only.
	auto tree_stage = [&](bool wide_again) {
		const int wide = wide_again ? 1 : p.hooks.wide_counts;
		const bool fits = std::max<uint32_t>(gstats[0], 1u) + 2u <= 255u;
		pw.narrow_ordcnt = fits && wide != 1;
		pw.narrow_srccnt = pw.narrow_ordcnt && wide != 2;
		pw.narrow_incnt = pw.narrow_srccnt && wide != 3;
		dense_nb0 = run_parallel_tree(ctx->cs, sw, pw, ctx->tw, C, gstats[0], p.big_class_dfs, p.sparse_splitters, p.hooks, tm, s);
	};
	if (p.seq_tree) {
		lanes.init(s);
		tm.begin("tree_seq");
		sw.stages = SEQ_STAGE_TREE;
		launch_seq_components(sw, s);
		tm.end(1);
	} else {
		tree_stage(false);
	}
	pw.all_vertex_classes = p.all_vertex_classes;
	pw.check_laminar = p.check_laminar;
	out.tail.want_overlap = p.overlap_tail;
	out.tail.done = f.ev1;
	out.tail.done2 = ctx->tail_done;
	// the result block is allocated as soon as the number of PVST vertices is known (before the emit kernel): the parallel
	// stages write it straight into pinned host memory, there is no device-to-host copy
	auto alloc_result_block = [&f](size_t total) -> void * {
		f.release_blocks();
		void *dev = nullptr;
		HIP_CHECK(hipHostGetDevicePointer(&dev, f.alloc(total).p, 0));
		return dev;
	};
	if (!run_parallel_dg(ctx->cs, sw, pw, C, t.n_processed, t.n_stack, dense_nb0, p.hooks, alloc_result_block, tm, s, ctx->side, out.tail)) {
		// a byte of incnt8 overflowed (only a pass with narrow_incnt says so): counters cleared, both stages again with words
		ctx->wide_repeats++;
		zero_component_counters(sw, C, pw.comp_bad, pw.err, s);
		tree_stage(true);
		if (!run_parallel_dg(ctx->cs, sw, pw, C, t.n_processed, t.n_stack, dense_nb0, p.hooks, alloc_result_block, tm, s, ctx->side, out.tail))
			throw HipError("class stage: the word form of the bracket counts reported an overflow (internal)");
	}
	out.stack_export_pending = true;
	if (p.redo_odd) // (tests: flag every other component as if its stack were not laminar)
		mark_odd_u32(pw.comp_bad, C, s);
	// Everything the host needs came back with the PVST count, unless something after it can still flag a component (the
	// laminarity check, the test modes) or add to the result (labels, boundaries): then the summary is read again when all
	// of that is done.
	out.fast_tail = out.tail.summary_final && !p.leaf_sub && !p.hairpins && !p.force_redo && !p.redo_odd;
	out.sum = out.fast_tail ? out.tail.early_summary : read_summary(ctx, C, true, f);
	const PassSummary sum(C, out.sum);
	if (sum.err(PassSummary::NO_BRACKET))
		throw HipError("parallel class stage: a tree vertex has no live bracket (internal invariant broken)");
	if (sum.err(PassSummary::WALK_POOL))
		throw HipError("class walk: stack pool exhausted (internal sizing bug)");
	if (sum.err(PassSummary::FOREST_SIZE))
		throw HipError("spanning forest of the links has the wrong size (internal)");
	for (uint32_t c = 0; c < C; c++)
		out.nbad += sum.bad(c) ? 1 : 0;
	return dense_nb0;
}

// ---- the leaf subflubble passes -- find_tiny + find_parallel relabel leaf flubbles (leaf_kernels.hip): the PVSTs the
// parallel stages just emitted here, those of components that go through the redo of add_flubbles after it (redo) --
// and with -s the inserting passes
static void leaf_passes(povu_hip_ctx *ctx, const PassPlan &p, uint32_t C, uint32_t nbad, povu_hip_forest &f, LeafState &leaf_state,
			StageTimer &tm)
{
	hipStream_t s = ctx->stream;
	if (nbad && p.hairpins)
		throw HipError("leaf subflubble passes: with --hairpins a component that needs the sequential redo is rebuilt "
			       "from scratch by the one-lane kernels, whose tree state the passes do not read");
	tm.begin("leaf_subflubbles");
	leaf_prepare(ctx->cs, ctx->sw, ctx->pw, ctx->tw, C, ctx->ws_leaf, leaf_state, s);
	leaf_dense(leaf_state, ctx->sw, ctx->pw, C, s);
	const size_t n = ctx->pw.d_total;
	povu_hip_forest::Block &b = f.blocks.empty() ? f.alloc(n) : f.blocks[0]; // (the parallel stages' own)
	f.labels = n != 0;
	b.sub_ai.resize(n, ctx->pool); // (page-locked, out of the context's pool)
	b.sub_zi.resize(n, ctx->pool);
	b.sub_fam.resize(n, ctx->pool);
	if (n) {
		HIP_CHECK(copy_async(b.sub_ai.data(), leaf_state.dense.ai, n * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(b.sub_zi.data(), leaf_state.dense.zi, n * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(b.sub_fam.data(), leaf_state.dense.fam, n, hipMemcpyDeviceToHost, s));
	}
	tm.end(16);
	HIP_CHECK(hipStreamSynchronize(s));
	if (!p.all_sub)
		return;
	// find_concealed, find_midi, find_smothered insert vertices (sub_kernels.hip); they read the dense PVST the parallel
	// stages wrote, so a component that needs the sequential redo has no place here
	if (nbad || p.force_redo || p.redo_odd)
		throw HipError(SUB_REDO_REFUSAL);
	tm.begin("subflubbles_insert");
	b.subx = std::make_shared<SubForest>();
	run_subflubbles(ctx->cs, ctx->sw, ctx->pw, ctx->tw, leaf_state, C, ctx->host, *b.subx, ctx->pool, s, ctx->ws_sub);
	tm.end(40);
}

// ---- the redo decision: components whose candidate stack is not laminar go through the exact sequential kernels (every
// component with POVU_HIP_F_FORCE_REDO, or for the hairpin report, which the parallel path only has for a whole pass)
static void redo(povu_hip_ctx *ctx, const PassPlan &p, uint32_t C, int64_t dense_nb0, SeqLanes &lanes, const LeafState &leaf_state,
		 StageTimer &tm, RowsOut &out)
{
	SeqWs &sw = ctx->sw;
	hipStream_t s = ctx->stream;
	if (p.force_redo || (out.nbad && p.hairpins)) {
		fill_u32(ctx->pw.comp_bad, C, 1u, s);
		out.nbad = C;
	} else if (out.nbad) {
		out.mixed = true; // (the others keep the dense result the parallel stages wrote)
	}
	if (!out.nbad)
		return;
	tm.begin("redo_seq");
	if (dense_nb0 >= 0 && !p.hairpins) {
		// Only add_flubbles' stack machine (flubbles.cpp:316-365) cannot be evaluated in closed form on such a stack; tree,
		// classes, candidate stack and next_seen of the parallel stages stand.  They are copied into the per-component
		// layout, one lane per flagged component runs the machine.
		lanes.carve();
		export_parallel_stack(ctx->cs, sw, ctx->pw, s);
		out.stack_export_pending = false;
		HIP_CHECK(hipMemsetAsync(sw.in_s, 0, lanes.z.B + lanes.z.T, s));
		sw.stages = SEQ_STAGE_PVST | SEQ_STAGE_GIVEN_STACK;
		out.redo_pvst_only = true;
	} else {
		if (p.leaf_sub)
			throw HipError("leaf subflubble passes: this pass rebuilds the flagged components from scratch with the "
				       "one-lane kernels, whose tree state the passes do not read");
		if (dense_nb0 >= 0) // parallel tree: the one-lane kernels start from scratch
			lanes.init(s);
		sw.stages = dense_nb0 >= 0 ? SEQ_STAGE_ALL : (SEQ_STAGE_CLASSES | SEQ_STAGE_STACK | SEQ_STAGE_PVST);
	}
	sw.comp_sel = ctx->pw.comp_bad;
	if (p.leaf_sub) { // (only reached with the PVST-only redo, see above)
		sw.p_ai = leaf_state.p_ai;
		sw.p_zi = leaf_state.p_zi;
	}
	launch_seq_components(sw, s);
	sw.comp_sel = nullptr;
	if (p.leaf_sub)
		leaf_seq(leaf_state, ctx->cs, sw, ctx->pw.comp_bad, C, s);
	tm.end(1);
	out.sum = nullptr;
}

// ---- rows C-G, on the one-lane kernels (POVU_HIP_F_SEQUENTIAL) or the parallel ones with their leaf passes, hairpin
// report and redo
static RowsOut rows_c_to_g(povu_hip_ctx *ctx, const PassPlan &p, uint32_t C, const uint32_t *gstats, const CompTables &t,
			   povu_hip_forest &f, SeqLanes &lanes, LeafState &leaf_state, StageTimer &tm)
{
	const CompState &cs = ctx->cs;
	SeqWs &sw = ctx->sw;
	hipStream_t s = ctx->stream;
	sw.V = ctx->g.V, sw.E = ctx->g.E, sw.C = C, sw.rank = p.rank, sw.world = p.world, sw.want_depth = p.all_sub;
	sw.voff = cs.voff, sw.eoff = cs.eoff, sw.loff = cs.loff, sw.ladj = cs.ladj, sw.gid_s = cs.gid_s, sw.tip_s = cs.tip_s;
	sw.start_key = cs.start_key, sw.p_ai = sw.p_zi = nullptr;
	tm.begin("traversal_init");
	zero_component_counters(sw, C, p.all_seq ? nullptr : ctx->pw.comp_bad, p.all_seq ? nullptr : ctx->pw.err, s);
	if (p.all_seq)
		lanes.init(s);
	tm.end(p.all_seq ? 14 : 1);
	sw.comp_sel = nullptr;
	RowsOut out;
	if (p.all_seq) {
		tm.begin("traversal_seq");
		sw.stages = SEQ_STAGE_ALL;
		launch_seq_components(sw, s);
		tm.end(1);
		return out;
	}
	const int64_t dense_nb0 = parallel_rows(ctx, p, C, gstats, t, f, lanes, tm, out);
	if (p.leaf_sub) {
		leaf_passes(ctx, p, C, out.nbad, f, leaf_state, tm);
		out.sum = nullptr; // (read again when the pass is done: its total then includes these stages)
	}
	if (p.hairpins && !out.nbad) {
		run_parallel_hairpins(cs, sw, ctx->pw, C, tm, s);
		out.sum = nullptr;
	}
	redo(ctx, p, C, dense_nb0, lanes, leaf_state, tm, out);
	return out;
}

// One array of the one-lane kernels' per-component layout (component c's PVST starts at voff[c] + c) and where it goes:
// `dst` at every tree's `off` -- or, for the hairpin boundaries (`hp`, 16 bytes each), at its `hp_off`.
struct SeqArray {
	const void *src;
	void *dst;
	size_t esz; // bytes per entry
	bool hp = false;
};

// The spans of the trees `ts` in `arrays` to the host: for a few trees (when `spans_if_few`) one copy per span, else one
// bulk copy per array, sliced on the host.  `done`, if given, is recorded behind the copies.
static void fetch_seq(const std::vector<povu_hip_forest::Tree *> &ts, const uint32_t *voff, size_t P, const std::vector<SeqArray> &arrays,
		      bool spans_if_few, hipEvent_t done, hipStream_t s)
{
	struct Span {
		size_t src, dst, bytes;
	};
	auto span = [&](const povu_hip_forest::Tree &t, const SeqArray &x) {
		const size_t pb = (size_t)voff[t.component_id - 1] + (t.component_id - 1);
		return Span{pb * x.esz, (x.hp ? t.hp_off : t.off) * x.esz, (x.hp ? t.n_hairpins : t.n_pvst) * x.esz};
	};
	const bool spans = spans_if_few && ts.size() <= 32;
	std::vector<std::vector<char>> bulk;
	for (const SeqArray &x : arrays)
		if (!spans) {
			bulk.emplace_back(P * x.esz);
			HIP_CHECK(copy_async(bulk.back().data(), x.src, bulk.back().size(), hipMemcpyDeviceToHost, s));
		}
	for (const auto *t : ts)
		for (size_t k = 0; spans && k < arrays.size(); k++) {
			const Span sp = span(*t, arrays[k]);
			if (sp.bytes)
				HIP_CHECK(copy_async((char *)arrays[k].dst + sp.dst, (const char *)arrays[k].src + sp.src, sp.bytes, hipMemcpyDeviceToHost, s));
		}
	if (done)
		HIP_CHECK(hipEventRecord(done, s));
	HIP_CHECK(hipStreamSynchronize(s));
	for (const auto *t : ts)
		for (size_t k = 0; !spans && k < arrays.size(); k++) {
			const Span sp = span(*t, arrays[k]);
			if (sp.bytes)
				memcpy((char *)arrays[k].dst + sp.dst, bulk[k].data() + sp.src, sp.bytes);
		}
}

// the one-lane kernels' PVST arrays (and hairpin boundaries) of the trees `ts` into `dst` ...
static void fetch_seq_pvst(const std::vector<povu_hip_forest::Tree *> &ts, const uint32_t *voff, size_t P, const SeqWs &sw, bool hairpins,
			   const povu_hip_forest::Arrays &dst, size_t n_total, povu_hip_forest &f, hipStream_t s)
{
	std::vector<uint8_t> ors(n_total);
	std::vector<SeqArray> arrays{{sw.p_a, dst.a, 4}, {sw.p_z, dst.z, 4}, {sw.p_parent, dst.parent, 4}, {sw.p_or, ors.data(), 1}};
	if (hairpins)
		arrays.push_back({sw.hairpins, f.hairpins.data(), 16, true});
	fetch_seq(ts, voff, P, arrays, true, f.ev1, s);
	for (size_t i = 0; i < n_total; i++) {
		dst.aor[i] = ors[i] & 1;
		dst.zor[i] = (ors[i] >> 1) & 1;
	}
}

// ... and their subflubble labels (leaf_seq wrote them in the same per-component layout)
static void fetch_seq_labels(const std::vector<povu_hip_forest::Tree *> &ts, const uint32_t *voff, size_t P, const LeafState &ls,
			     povu_hip_forest::Block &b, hipStream_t s)
{
	b.sub_ai.assign(b.total, POVU_NIL);
	b.sub_zi.assign(b.total, POVU_NIL);
	b.sub_fam.assign(b.total, 0);
	fetch_seq(ts, voff, P, {{ls.p_ai, b.sub_ai.data(), 4}, {ls.p_zi, b.sub_zi.data(), 4}, {ls.p_fam, b.sub_fam.data(), 1}}, false, nullptr, s);
}

// ---- the result fetch: the dense layout the parallel stages wrote into f.blocks[0] (a mixed pass: plus blocks[1] for the
// redone components), or the one-lane kernels' per-component layout
static void fetch_result(povu_hip_ctx *ctx, const PassPlan &p, uint32_t C, const uint32_t *voff, const uint32_t *eoff, RowsOut &out,
			 povu_hip_forest &f, const LeafState &leaf_state, StageTimer &tm)
{
	hipStream_t s = ctx->stream;
	const size_t P = (size_t)ctx->g.V + C;
	tm.begin("pvst_d2h");
	const PassSummary sum(C, out.sum ? out.sum : read_summary(ctx, C, !p.all_seq, f));
	for (uint32_t c = 0; c < C; c++)
		if (sum.status(c) == 2)
			throw HipError("internal error: the spanning tree of component " + std::to_string(c + 1) + " did not reach every side");
	f.total_components = C;
	size_t total = 0, total_hp = 0;
	for (uint32_t c = 0; c < C; c++) {
		if (sum.npvst(c) == 0)
			continue;
		povu_hip_forest::Tree t;
		t.component_id = c + 1; // decompose.cpp:129
		t.n_vtx = voff[c + 1] - voff[c];
		t.n_links = eoff[c + 1] - eoff[c];
		t.n_pvst = sum.npvst(c);
		t.off = total;
		t.hp_off = total_hp;
		t.n_hairpins = p.hairpins ? sum.nbry(c) : 0;
		t.sub_c = c;
		total += sum.npvst(c);
		total_hp += t.n_hairpins;
		f.trees.push_back(t);
	}
	f.hairpins.resize(2 * total_hp);
	std::vector<povu_hip_forest::Tree *> redone;
	if (p.all_seq || (out.nbad && !out.mixed)) { // the one-lane kernels' layout for every tree
		if (!f.blocks.empty() && f.blocks[0].total != total)
			f.release_blocks();
		if (f.blocks.empty())
			f.alloc(total);
		for (auto &t : f.trees)
			redone.push_back(&t);
		tm.end(0);
		fetch_seq_pvst(redone, voff, P, ctx->sw, p.hairpins, f.blocks[0], total, f, s);
		f.labels = p.leaf_sub && total;
		if (p.leaf_sub)
			fetch_seq_labels(redone, voff, P, leaf_state, f.blocks[0], s);
		return;
	}
	// the parallel stages wrote every PVST back to back into f.blocks[0]
	if (!out.mixed && (sum.total() != total || total != ctx->pw.d_total))
		throw HipError("internal error: dense PVST size mismatch");
	if (f.blocks.empty())
		f.alloc(ctx->pw.d_total);
	size_t redo_total = 0;
	for (auto &t : f.trees) {
		if (out.mixed && sum.bad(t.component_id - 1)) {
			t.off = redo_total;
			redo_total += t.n_pvst;
			redone.push_back(&t);
		} else {
			t.off = sum.doff(t.component_id - 1);
		}
	}
	bool more = false;
	for (const auto &t : f.trees)
		if (t.n_hairpins) {
			const size_t pb = (size_t)voff[t.component_id - 1] + (t.component_id - 1);
			HIP_CHECK(copy_async(f.hairpins.data() + 2 * t.hp_off, ctx->sw.hairpins + 2 * pb, (size_t)t.n_hairpins * 16,
					     hipMemcpyDeviceToHost, s));
			more = true;
		}
	tm.end(0);
	if (!redone.empty()) { // the redone components get a block of their own
		const int bi = (int)f.blocks.size();
		povu_hip_forest::Block &x = f.alloc(redo_total);
		for (auto *t : redone)
			t->blk = bi;
		fetch_seq_pvst(redone, voff, P, ctx->sw, p.hairpins, x, redo_total, f, s);
		if (p.leaf_sub)
			fetch_seq_labels(redone, voff, P, leaf_state, x, s);
	} else if (out.fast_tail && out.tail.overlapped && !more) {
		// the arrays are still on their way: the caller (or the next accessor of the forest) waits for ev1
		f.pending = true;
		ctx->tail_pending = true;
	} else if (out.fast_tail && !more) {
		HIP_CHECK(hipEventSynchronize(f.ev1)); // (recorded behind the last copy by run_parallel_dg)
		if (tm.enabled)
			HIP_CHECK(hipStreamSynchronize(s)); // (the stage events themselves have to complete before they are read)
	} else if (more || tm.enabled || out.fast_tail) {
		HIP_CHECK(hipEventRecord(f.ev1, s));
		HIP_CHECK(hipStreamSynchronize(s));
	}
}

// ---- stage times, and the pass total unless its arrays are still on their way
static void stage_times(povu_hip_ctx *ctx, const StageTimer &tm, povu_hip_forest &f)
{
	ctx->last_times.clear();
	for (auto &r : tm.recs) {
		povu_hip_stage_time st{};
		snprintf(st.name, sizeof st.name, "%s", r.name.c_str());
		float ms = 0;
		HIP_CHECK(hipEventElapsedTime(&ms, r.a, r.b));
		st.ms = ms;
		st.launches = r.launches;
		ctx->last_times.push_back(st);
	}
	if (!f.pending) {
		povu_hip_stage_time st{};
		snprintf(st.name, sizeof st.name, "total");
		f.ready();
		st.ms = f.pass_ms;
		ctx->last_times.push_back(st);
	}
}

} // namespace

extern "C" povu_hip_forest *povu_hip_decompose(povu_hip_ctx *ctx, const povu_hip_opts *opts, char *err, size_t errlen)
{
	// declared outside the try block: on a failure the stream is drained BEFORE the forest returns its pinned
	// result block to the pool (kernels that write into it may still be queued)
	std::unique_ptr<povu_hip_forest> f;
	XferScope xfer(ctx);
	try {
		if (ctx && !ctx->g.block && ctx->shard_total_components) { // a shard without components: nothing to do
			f = std::make_unique<povu_hip_forest>();
			f->pool = ctx->pool;
			f->total_components = ctx->shard_total_components;
			ctx->last_times.clear();
			ctx->last_links = 0;
			return f.release();
		}
		if (!ctx || !ctx->g.block)
			throw HipError("no graph resident: call povu_hip_graph_upload first");
		HIP_CHECK(hipSetDevice(ctx->device));
		const PassPlan p = plan_pass(opts);
		if (!p.overlap_tail)
			ctx->wait_tail();
		const ResidentGraph &g = ctx->g;
		Sizes z = rowb_begin(ctx, p);
		StageTimer &tm = ctx->timer;
		// the forest owns the two events that time its pass: ev0 at the first kernel, ev1 behind the last byte that reaches the host
		f = std::make_unique<povu_hip_forest>();
		f->pool = ctx->pool;
		HIP_CHECK(hipEventCreate(&f->ev0));
		HIP_CHECK(hipEventCreate(&f->ev1));
		HIP_CHECK(hipEventRecord(f->ev0, ctx->stream));

		const RowB rb = row_b(ctx, p, z, tm);
		const uint32_t C = rb.C;
		z.set_components(C);
		const bool tail_waited = carve_stages(ctx, p, z, C, tm);
		ctx->host.wait(rb.sizes);
		const CompTables tables = component_tables(ctx, p, C, rb.voff, rb.eoff, tail_waited);
		f->meta_reserve = (size_t)C + 1; // room behind the arrays for the tree table of povu_hip_forest_share
		SeqLanes lanes{ctx, z, p.hairpins};
		LeafState leaf_state;
		RowsOut out = rows_c_to_g(ctx, p, C, rb.gstats, tables, *f, lanes, leaf_state, tm);
		fetch_result(ctx, p, C, rb.voff, rb.eoff, out, *f, leaf_state, tm);
		if (!p.leaf_sub)
			ctx->ws_leaf.release(); // (kept from one -s pass to the next, like the inserting passes' arena below: a hipMalloc of
						// several GB right after the hipFree of the pass before stalled for over a second once; a
						// pass without the leaf passes gives it back)
		if (!p.all_sub)
			ctx->ws_sub.release(); // (the inserting passes keep their phase arenas from one -s pass to the next, no longer)
		stage_times(ctx, tm, *f);
		ctx->last = LastPass{true, p, C, out.nbad, out.mixed, out.redo_pvst_only, out.stack_export_pending};
		ctx->last.narrow_counts = !p.all_seq && !p.seq_tree && ctx->pw.narrow_ordcnt;
		ctx->last.narrow_forms = !ctx->last.narrow_counts ? 0 : 1 | (ctx->pw.narrow_srccnt ? 2 : 0) | (ctx->pw.narrow_incnt ? 4 : 0);
		ctx->last.prefix_records = ctx->last.narrow_counts ? ctx->pw.prefix_records : 0;
		if (p.world == 1 && ctx->shard_comp_ids.empty()) { // (povu_hip_forest_walks: a forest of the whole resident graph)
			f->walk_ctx = ctx;
			f->walk_gen = g.gen;
		}
		return f.release();
	} catch (const std::exception &e) {
		if (ctx && ctx->stream)
			(void)hipStreamSynchronize(ctx->stream);
		if (ctx && ctx->side.stream)
			(void)hipStreamSynchronize(ctx->side.stream);
		f.reset();
		set_err(err, errlen, e.what());
		return nullptr;
	}
}

extern "C" int povu_hip_last_stage_times(const povu_hip_ctx *ctx, povu_hip_stage_time *out, int max)
{
	if (!ctx)
		return 0;
	int n = (int)ctx->last_times.size();
	if (out)
		for (int i = 0; i < n && i < max; i++)
			out[i] = ctx->last_times[i];
	return n;
}

extern "C" uint32_t povu_hip_last_seq_redo(const povu_hip_ctx *ctx) { return ctx ? ctx->last.seq_redo : 0; }

extern "C" uint64_t povu_hip_last_links_processed(const povu_hip_ctx *ctx) { return ctx ? ctx->last_links : 0; }

extern "C" int povu_hip_last_narrow_counts(const povu_hip_ctx *ctx)
{
	return ctx && ctx->last.valid && ctx->last.narrow_counts ? ctx->last.narrow_forms : 0;
}
extern "C" int povu_hip_last_prefix_records(const povu_hip_ctx *ctx) { return ctx && ctx->last.valid ? ctx->last.prefix_records : 0; }
extern "C" uint64_t povu_hip_wide_repeats(const povu_hip_ctx *ctx) { return ctx ? ctx->wide_repeats : 0; }

extern "C" int povu_hip_last_black_only_classes(const povu_hip_ctx *ctx)
{
	return ctx && ctx->last.valid && !ctx->last.plan.all_seq && ctx->pw.black_only_used ? 1 : 0;
}

extern "C" int povu_hip_last_crossings(povu_hip_ctx *ctx, uint32_t out[2])
{
	if (!ctx || !out)
		return 1;
	out[0] = out[1] = 0;
	if (!ctx->last.valid || ctx->last.plan.all_seq || !ctx->pw.laminar_checked)
		return 0;
	ctx->quiesce();
	if (hipSetDevice(ctx->device) != hipSuccess)
		return 2;
	static_assert(PW_N_CROSSED == PW_N_X + 1, "the two crossing words are copied as a pair");
	return hipMemcpy(out, ctx->pw.err + PW_N_X, 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
}

extern "C" int povu_hip_last_lsz_field(povu_hip_ctx *ctx, uint32_t out[2])
{
	if (!ctx || !out)
		return 1;
	out[0] = out[1] = 0;
	if (!ctx->last.valid || ctx->last.plan.all_seq || !ctx->pw.black_only_used)
		return 0;
	ctx->quiesce();
	if (hipSetDevice(ctx->device) != hipSuccess)
		return 2;
	try {
		out[0] = ctx->pw.lsz_field.w;
		out[1] = count_saturated(ctx->pw, ctx->stream);
	} catch (const std::exception &) {
		return 2;
	}
	return 0;
}

extern "C" int povu_hip_last_laminar_check_ran(const povu_hip_ctx *ctx)
{
	return ctx && ctx->last.valid && !ctx->last.plan.all_seq && ctx->pw.laminar_checked ? 1 : 0;
}
