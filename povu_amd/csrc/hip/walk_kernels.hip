// walk_kernels.hip -- the walks of every flubble of a forest (povu_hip_forest_walks, include/povu_hip.h).
//
// The definition is this project's own ("Flubble walks"): the reference's enum_walks is a BFS whose output
// depends on its queue cap and on std::set indices, so it is not restated.  A query is one PVST vertex (start step S, end
// step Z); its walks are what a DFS from S yields that tries the successors of a step by ascending (segment id, '>' first),
// never repeats a segment and stops at Z -- with three caps: walks (K), steps per walk (L), expansions (E).
//
// A step is kept as the side it ENTERS its segment by: (u, '>') enters through l = 2u, (u, '<') through r = 2u + 1, and
// leaves through the other side (y ^ 1).  Segment ids ascend with the vertex index (checked), so the successor order
// (id, '>' before '<') is the plain order of the entered sides, and the successors of a step are the other ends (aoth) of
// its exit side's slots, ascending -- `ssucc`, one sorted copy of the adjacency per call.  Parallel links are equal
// neighbours in that copy and count once.
//
// Shape: a count pass, an exclusive scan of walks and steps per query, an emit pass that runs the same DFS again and writes
// into the scanned offsets.  Each pass has two tiers:
//   tier 1: one lane per query, the DFS stack in LDS (T1_DEPTH frames, T1_EXPANSIONS expansions).  Leaf bubbles -- nearly
//           every query -- end here.  A query that would need more is handed over (flag + compaction);
//   tier 2: one lane per query, every lane taking its next query from an atomic work counter when it is done with one (a
//           long query does not hold up a wave of short ones), the stack in global scratch (L frames per lane) beside a
//           hash set of the segments on the path (the on-path test in O(1) at any depth).
// Both passes run the same function (dfs, walk_rules.hpp), so the emit pass writes exactly what the count pass sized; it still
// checks every write against the query's own range.
#include "query_common.hpp"
#include "walk_rules.hpp"

namespace povu_hip
{

// (walk_rules.hpp is free of HIP and of the C ABI: what it restates of them)
static_assert(WALK_TPB == Q_TPB && WALK_NONE == NO_QUERY, "walk_rules.hpp restates query_common.hpp");
static_assert(ST_MORE == POVU_HIP_WALK_MORE && ST_LONG == POVU_HIP_WALK_LONG && ST_BUDGET == POVU_HIP_WALK_BUDGET, "walk_rules.hpp restates povu_hip.h");

// ---- the sorted successor copy

// one lane per side: insertion-sort the side's other ends into ssucc when the side is small; a larger side only sets
// *hub (the host then sorts every slot with the radix sort, below)
__global__ void k_wk_ssucc(uint32_t nS, const uint32_t *__restrict__ off, const uint32_t *__restrict__ aoth,
			      uint32_t *__restrict__ ssucc, uint32_t *__restrict__ hub)
{
	const uint32_t x = blockIdx.x * Q_TPB + threadIdx.x;
	if (x >= nS)
		return;
	const uint32_t b = off[x], e = off[x + 1];
	if (e - b > SORT_IN_LANE) {
		atomicOr(hub, 1u);
		return;
	}
	for (uint32_t i = b; i < e; i++) {
		const uint32_t v = aoth[i];
		uint32_t j = i;
		while (j > b && ssucc[j - 1] > v) {
			ssucc[j] = ssucc[j - 1];
			j--;
		}
		ssucc[j] = v;
	}
}

// side of every slot (the key of the second, stable sort of the hub path)
__global__ void k_wk_slot_side(uint32_t nS, const uint32_t *__restrict__ off, uint32_t *__restrict__ side_of)
{
	const uint32_t x = blockIdx.x * Q_TPB + threadIdx.x;
	if (x >= nS)
		return;
	for (uint32_t i = off[x], e = off[x + 1]; i < e; i++)
		side_of[i] = x;
}

// ---- the DFS (both tiers, both passes): dfs<EMIT, Stack> over a LaneStack or a GlobalStack, walk_rules.hpp

// tier 1, count pass: one lane per query.  Hands over (flag) what needs more than T1_DEPTH frames or T1_EXPANSIONS.
template <bool EMIT>
__global__ __launch_bounds__(Q_TPB) void k_wk_t1(uint32_t n, const uint32_t *__restrict__ off, const uint32_t *__restrict__ ssucc,
						   const uint32_t *__restrict__ ys, const uint32_t *__restrict__ yz, WalkCaps c, uint32_t force2,
						   uint32_t *__restrict__ cntw, uint32_t *__restrict__ cnts, uint8_t *__restrict__ status,
						   uint8_t *__restrict__ handover, const uint32_t *__restrict__ woff,
						   const uint32_t *__restrict__ sbase, WalkSink sink)
{
	__shared__ uint32_t sy[T1_DEPTH * Q_TPB], sc[T1_DEPTH * Q_TPB];
	const uint32_t q = blockIdx.x * Q_TPB + threadIdx.x;
	if (q >= n)
		return;
	if (EMIT && handover[q])
		return;
	if (!EMIT && force2) {
		handover[q] = 1;
		return;
	}
	LaneStack st{sy, sc, threadIdx.x};
	if (EMIT) {
		sink.w0 = woff[q];
		sink.w_end = sink.w0 + cntw[q];
		sink.s0 = sbase[q];
		sink.s_end = sink.s0 + cnts[q];
	}
	const DfsResult r = dfs<EMIT>(st, off, ssucc, ys[q], yz[q], c, c.E < T1_EXPANSIONS ? c.E : T1_EXPANSIONS, sink);
	if (EMIT)
		return;
	handover[q] = r.handover ? 1 : 0;
	cntw[q] = r.handover ? 0 : r.walks;
	cnts[q] = r.handover ? 0 : r.steps;
	status[q] = r.handover ? 0 : r.status;
}

// tier 2: one lane per query of `list`, every lane taking its next query from `*next` (zeroed before the launch) as soon as
// it is done with one; `lanes` lanes, lane i's words in scratch at [i, i + lanes, ...): 2 L stack words, then 2^tbits path-set
// slots (zeroed before the launch; every search leaves its set empty)
template <bool EMIT>
__global__ __launch_bounds__(Q_TPB) void k_wk_t2(const uint32_t *__restrict__ list, uint32_t n2, uint32_t *__restrict__ next,
						 uint32_t lanes, uint32_t tbits, const uint32_t *__restrict__ off, const uint32_t *__restrict__ ssucc,
						 const uint32_t *__restrict__ ys, const uint32_t *__restrict__ yz, WalkCaps c, uint32_t *scratch,
						 uint32_t *__restrict__ cntw, uint32_t *__restrict__ cnts, uint8_t *__restrict__ status,
						 const uint32_t *__restrict__ woff, const uint32_t *__restrict__ sbase, WalkSink sink)
{
	const uint32_t lane = blockIdx.x * Q_TPB + threadIdx.x;
	if (lane >= lanes)
		return;
	GlobalStack st{scratch + lane, scratch + (size_t)lanes * c.L + lane, scratch + (size_t)lanes * 2 * c.L + lane, lanes, c.L, tbits};
	for (;;) {
		const uint32_t k = atomicAdd(next, 1u);
		if (k >= n2)
			break;
		const uint32_t q = list[k];
		if (EMIT) {
			sink.w0 = woff[q];
			sink.w_end = sink.w0 + cntw[q];
			sink.s0 = sbase[q];
			sink.s_end = sink.s0 + cnts[q];
		}
		const DfsResult r = dfs<EMIT>(st, off, ssucc, ys[q], yz[q], c, c.E, sink);
		if (!EMIT) {
			cntw[q] = r.walks;
			cnts[q] = r.steps;
			status[q] = r.status;
		}
	}
}

} // namespace povu_hip

// ---- C ABI

namespace
{
struct WalksOwner {
	povu_hip_walks view{}; // first member: the owner is recovered from it in povu_hip_walks_free
	PinnedVec<uint32_t> walk_off, step_off, step_id;
	PinnedVec<uint8_t> step_or, status;
};
} // namespace

extern "C" povu_hip_walks *povu_hip_forest_walks(povu_hip_ctx *ctx, povu_hip_forest *f, const povu_hip_walk_opts *opts, char *err,
						 size_t errlen)
{
	CallTimer timer;
	return guarded_call(ctx, err, errlen, (povu_hip_walks *)nullptr, [&] {
		check_query_forest(ctx, f, "walks");
		WalkCaps c{64, 1000, 65536};
		uint32_t flags = 0;
		if (opts) {
			if (opts->max_walks)
				c.K = opts->max_walks;
			if (opts->max_steps)
				c.L = opts->max_steps;
			if (opts->max_expansions)
				c.E = opts->max_expansions;
			flags = opts->flags;
		}
		if (c.L > (1u << 24))
			throw HipError("max_steps above 2^24");
		const ResidentGraph &g = ctx->g;
		hipStream_t s = ctx->stream;
		const uint32_t nS = 2 * g.V;
		const size_t slots = g.n_slots;

		// ---- the queries (tree order, then PVST vertex order, roots skipped); beside them counts, offsets, the hand-over
		// list, the sorted successors
		uint32_t *cntw, *cnts, *woff, *sbase, *list2, *ssucc;
		uint8_t *status, *handover;
		unsigned long long *tot;
		void *tmp;
		size_t tmp_b = 0;
		const QueryFront q = query_front(ctx, f, ctx->wk_ws, timer, [&](Spans &take, uint32_t n) {
			const size_t n1 = (size_t)n + 1;
			tmp_b = prim_tmp_bytes(n1, false) + 256;
			take(n1, cntw, cnts, woff, sbase, list2, status, handover);
			take(2, tot);
			take(tmp_b, tmp);
			take(slots + 8, ssucc);
		});
		const uint32_t n = q.n, *ys = q.ys, *yz = q.yz;
		uint32_t *words = q.words;
		const size_t n1 = (size_t)n + 1;
		// words: [0] the checks, [1] hand-over count, [2] / [3] tier-2 work counter of the count / emit pass, [4] a side has
		// more than SORT_IN_LANE slots
		if (nS)
			KLAUNCH(k_wk_ssucc, dim3(lane_blocks(nS)), dim3(Q_TPB), 0, s, nS, g.off, g.aoth, ssucc, words + 4);
		uint32_t hw[8] = {0};
		HIP_CHECK(copy_async(hw, words, 32, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		query_refusals(hw[0], "walks");
		if (hw[4] && slots) { // a hub side: every slot's (other end, side) pair, sorted by other end, then stably by side
			const size_t sort_b = sort_tmp_bytes(slots) + 256;
			uint32_t *side_of, *k1, *v1, *k2;
			void *sort_tmp;
			carve(ctx->wk_out, [&](Spans &take) { // (free until the count pass's tier 2)
				take(slots + 8, side_of, k1, v1, k2);
				take(sort_b, sort_tmp);
			});
			KLAUNCH(k_wk_slot_side, dim3(lane_blocks(nS)), dim3(Q_TPB), 0, s, nS, g.off, side_of);
			const unsigned bits = bits_for(nS);
			sort_pairs_u32(g.aoth, k1, side_of, v1, slots, bits, sort_tmp, sort_b, s);
			sort_pairs_u32(v1, k2, k1, ssucc, slots, bits, sort_tmp, sort_b, s);
			HIP_CHECK(hipStreamSynchronize(s)); // (the next reserve of wk_out may free these arrays)
		}

		// ---- count pass
		const bool force2 = (flags & POVU_HIP_W_FORCE_TIER2) != 0;
		WalkSink none{};
		uint32_t n2 = 0;
		if (n) {
			KLAUNCH(k_wk_t1<false>, dim3(lane_blocks(n)), dim3(Q_TPB), 0, s, n, g.off, ssucc, ys, yz, c, force2 ? 1u : 0u, cntw, cnts,
				status, handover, woff, sbase, none);
			compact_flagged_u8(handover, n, list2, words + 1, tmp, tmp_b, s);
			n2 = read_back(words + 1, s);
		}
		// tier-2 lanes: 2 L stack words + a path set of 2^tbits >= 2 L slots each, at most 16384 lanes and 256 MiB
		uint32_t lanes = 0;
		const uint32_t tbits = std::max(4u, bits_for(2 * (uint64_t)c.L - 1));
		const size_t lane_words = (size_t)2 * c.L + (size_t(1) << tbits);
		uint32_t *scratch = nullptr;
		if (n2) {
			lanes = (uint32_t)std::max<size_t>(1, std::min<size_t>({(size_t)n2, 16384, (size_t(256) << 20) / (lane_words * 4)}));
			carve(ctx->wk_out, [&](Spans &take) { take((size_t)lanes * lane_words, scratch); });
			HIP_CHECK(hipMemsetAsync(scratch + (size_t)lanes * 2 * c.L, 0, (size_t)lanes * (lane_words - 2 * (size_t)c.L) * 4, s));
			KLAUNCH(k_wk_t2<false>, dim3(lane_blocks(lanes)), dim3(Q_TPB), 0, s, list2, n2, words + 2, lanes, tbits, g.off, ssucc, ys, yz, c,
				scratch, cntw, cnts, status, woff, sbase, none);
		}
		// ---- offsets, then the emit pass into them
		uint64_t n_walks = 0, n_steps = 0;
		uint32_t *step_off = nullptr, *step_id = nullptr;
		uint8_t *step_or = nullptr;
		if (n) {
			counts_to_offsets(cntw, woff, cnts, sbase, n, tot, tmp, tmp_b, s, [&](const uint64_t *total) {
				n_walks = total[0], n_steps = total[1];
				if (n_walks >= 0xFFFFFFFFull || n_steps >= 0xFFFFFFFFull)
					throw HipError("the walks do not fit 32-bit offsets: " + std::to_string(n_walks) + " walks, " + std::to_string(n_steps) +
						       " steps (lower max_walks / max_steps)");
			});
			auto out = [&](Spans &take) {
				if (lanes)
					take((size_t)lanes * lane_words, scratch);
				take(n_walks + 1, step_off);
				take(n_steps + 1, step_id, step_or);
			};
			const size_t out_b = measure(out);
			if (out_b > ctx->wk_out.capacity()) {
				size_t free_b = 0, total_b = 0;
				(void)hipMemGetInfo(&free_b, &total_b);
				if (out_b > free_b + ctx->wk_out.capacity())
					throw HipError("the walks do not fit device memory: " + std::to_string(out_b >> 20) + " MiB needed, " +
						       std::to_string(free_b >> 20) + " MiB free");
			}
			HIP_CHECK(hipStreamSynchronize(s)); // (the count pass's tier 2 used the scratch of wk_out)
			carve(ctx->wk_out, out);
			if (lanes)
				HIP_CHECK(hipMemsetAsync(scratch + (size_t)lanes * 2 * c.L, 0, (size_t)lanes * (lane_words - 2 * (size_t)c.L) * 4, s));
			WalkSink sink{step_off, step_id, step_or, g.vid, 0, 0, 0, 0};
			KLAUNCH(k_wk_t1<true>, dim3(lane_blocks(n)), dim3(Q_TPB), 0, s, n, g.off, ssucc, ys, yz, c, 0u, cntw, cnts, status, handover,
				woff, sbase, sink);
			if (lanes)
				KLAUNCH(k_wk_t2<true>, dim3(lane_blocks(lanes)), dim3(Q_TPB), 0, s, list2, n2, words + 3, lanes, tbits, g.off, ssucc, ys, yz, c,
					scratch, cntw, cnts, status, woff, sbase, sink);
		}

		// ---- to the host
		auto o = std::make_unique<WalksOwner>();
		hand_off(o->walk_off, n1, woff, n ? n1 : 0, ctx);
		hand_off(o->status, n1, status, n, ctx);
		hand_off(o->step_off, n_walks + 1, step_off, n_walks, ctx);
		hand_off(o->step_id, n_steps, step_id, n_steps, ctx);
		hand_off(o->step_or, n_steps, step_or, n_steps, ctx);
		if (!n)
			o->walk_off[0] = 0;
		o->view.device_ms = timer.stop(s);
		o->step_off[n_walks] = (uint32_t)n_steps;
		o->view.n_queries = n;
		o->view.n_walks = n_walks;
		o->view.n_steps = n_steps;
		o->view.walk_off = o->walk_off.data();
		o->view.step_off = o->step_off.data();
		o->view.step_id = o->step_id.data();
		o->view.step_or = o->step_or.data();
		o->view.status = o->status.data();
		o->view.n_tier2 = n2;
		WalksOwner *raw = o.release();
		return &raw->view;
	});
}
extern "C" void povu_hip_walks_free(povu_hip_walks *w)
{
	delete reinterpret_cast<WalksOwner *>(w);
}
