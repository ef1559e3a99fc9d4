// walk_rules.hpp -- the search of one walks query ("Flubble walks"; restated in tests/walks_ref.py), everything
// of it that one lane does on its own: the caps, the two stacks a lane may keep its path on, and the DFS that both tiers and
// both passes of walk_kernels.hip run.  Plain C++17, free of HIP: the kernels run it on the device, a lane each;
// host/walk_check.cpp runs it under the sanitizers against std::set and a recursive enumeration.
//
// A step is kept as the side it ENTERS its segment by: (u, '>') enters through l = 2u, (u, '<') through r = 2u + 1, and leaves
// through the other side (y ^ 1).  The successors of a step are the other ends of its exit side's slots, ascending, in `ssucc`
// (one sorted copy of the adjacency, slots of side x at [off[x], off[x + 1])); parallel links are equal neighbours there and
// count once.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define WALK_FN __host__ __device__ inline
#else
#define WALK_FN inline
#endif

namespace povu_hip
{

static constexpr uint32_t T1_DEPTH = 16;	 // frames of a tier-1 stack (LDS: 16 x 256 x 8 B = 32 KiB per block)
static constexpr uint32_t T1_EXPANSIONS = 4096; // expansions tier 1 spends before it hands a query over
static constexpr uint32_t SORT_IN_LANE = 64;	 // sides up to this many slots are sorted by one lane
static constexpr uint32_t WALK_TPB = 256;	 // lanes of a workgroup (Q_TPB, query_common.hpp): the stride of a LaneStack
static constexpr uint32_t WALK_NONE = 0xFFFFFFFFu; // no step (NO_QUERY, query_common.hpp)
static constexpr uint8_t ST_MORE = 1, ST_LONG = 2, ST_BUDGET = 4; // POVU_HIP_WALK_*

struct WalkCaps {
	uint32_t K, L, E;
};

struct DfsResult {
	uint32_t walks, steps;
	uint8_t status;
	bool handover; // tier 1 only: the query needs more than the tier's limits
};

// where the emit pass writes the walks of one query
struct WalkSink {
	uint32_t *step_off, *step_id;
	uint8_t *step_or;
	const uint32_t *vid;
	uint32_t w0, w_end, s0, s_end; // walks [w0, w_end), steps [s0, s_end) of this query
};

// One lane, stack in LDS: frame k of lane t at [k * WALK_TPB + t] (consecutive lanes, consecutive banks).
struct LaneStack {
	uint32_t *sy, *sc;
	uint32_t t;
	static constexpr uint32_t cap = T1_DEPTH;
	WALK_FN uint32_t y(uint32_t k) const { return sy[k * WALK_TPB + t]; }
	WALK_FN uint32_t cur(uint32_t k) const { return sc[k * WALK_TPB + t]; }
	WALK_FN void set_cur(uint32_t k, uint32_t c) { sc[k * WALK_TPB + t] = c; }
	WALK_FN void push(uint32_t k, uint32_t yy, uint32_t c)
	{
		sy[k * WALK_TPB + t] = yy;
		sc[k * WALK_TPB + t] = c;
	}
	WALK_FN void pop(uint32_t) {}
	WALK_FN bool on_path(uint32_t u, uint32_t depth) const
	{
		for (uint32_t k = 0; k < depth; k++)
			if ((y(k) >> 1) == u)
				return true;
		return false;
	}
	WALK_FN void write_walk(const WalkSink &o, uint32_t w, uint32_t at, uint32_t depth, uint32_t yz) const
	{
		if (w >= o.w_end || at + depth + 1 > o.s_end)
			return; // (cannot happen: the count pass ran the same search)
		o.step_off[w] = at;
		for (uint32_t k = 0; k < depth; k++) {
			const uint32_t yy = y(k);
			o.step_id[at + k] = o.vid[yy >> 1];
			o.step_or[at + k] = (uint8_t)(yy & 1u);
		}
		o.step_id[at + depth] = o.vid[yz >> 1];
		o.step_or[at + depth] = (uint8_t)(yz & 1u);
	}
};

// One lane, stack in global scratch (L frames of its own): frame k at [k * stride] (the lanes of a wave side by side).  The
// segments on the path are also kept in an open-addressed set of `tmask + 1` >= 2 L slots (linear probing, key = segment + 1,
// 0 = empty, deletion by backward shift), so that "is u on the path" costs a probe or two however deep the stack is.
struct GlobalStack {
	uint32_t *sy, *sc, *tab;
	uint32_t stride;
	uint32_t cap;
	uint32_t tbits;
	WALK_FN uint32_t y(uint32_t k) const { return sy[(size_t)k * stride]; }
	WALK_FN uint32_t cur(uint32_t k) const { return sc[(size_t)k * stride]; }
	WALK_FN void set_cur(uint32_t k, uint32_t c) { sc[(size_t)k * stride] = c; }
	WALK_FN uint32_t home(uint32_t u) const { return (u * 2654435761u) >> (32 - tbits); }
	WALK_FN uint32_t &slot(uint32_t i) const { return tab[(size_t)i * stride]; }
	WALK_FN void push(uint32_t k, uint32_t yy, uint32_t c)
	{
		sy[(size_t)k * stride] = yy;
		sc[(size_t)k * stride] = c;
		const uint32_t mask = (1u << tbits) - 1u, u = yy >> 1;
		uint32_t i = home(u);
		while (slot(i) != 0)
			i = (i + 1) & mask;
		slot(i) = u + 1;
	}
	WALK_FN void pop(uint32_t yy)
	{
		const uint32_t mask = (1u << tbits) - 1u, key = (yy >> 1) + 1;
		uint32_t i = home(yy >> 1);
		while (slot(i) != key)
			i = (i + 1) & mask;
		for (uint32_t j = (i + 1) & mask;; j = (j + 1) & mask) { // backward shift: close the gap at i
			const uint32_t kj = slot(j);
			if (kj == 0)
				break;
			const uint32_t h = home(kj - 1);
			// kj may move to i when its home does not lie cyclically in (i, j]
			if (((j - h) & mask) >= ((j - i) & mask)) {
				slot(i) = kj;
				i = j;
			}
		}
		slot(i) = 0;
	}
	WALK_FN bool on_path(uint32_t u, uint32_t) const
	{
		const uint32_t mask = (1u << tbits) - 1u;
		for (uint32_t i = home(u);; i = (i + 1) & mask) {
			const uint32_t kk = slot(i);
			if (kk == 0)
				return false;
			if (kk == u + 1)
				return true;
		}
	}
	WALK_FN void write_walk(const WalkSink &o, uint32_t w, uint32_t at, uint32_t depth, uint32_t yz) const
	{
		if (w >= o.w_end || at + depth + 1 > o.s_end)
			return;
		o.step_off[w] = at;
		for (uint32_t k = 0; k < depth; k++) {
			const uint32_t yy = y(k);
			o.step_id[at + k] = o.vid[yy >> 1];
			o.step_or[at + k] = (uint8_t)(yy & 1u);
		}
		o.step_id[at + depth] = o.vid[yz >> 1];
		o.step_or[at + depth] = (uint8_t)(yz & 1u);
	}
};

// The search of one query.  `ecap` <= E expansions and `st.cap` frames are what this tier may use: needing more hands the
// query over (tier 1); tier 2 is called with ecap = E and room for L frames.
template <bool EMIT, class Stack>
WALK_FN DfsResult dfs(Stack &st, const uint32_t *__restrict__ off, const uint32_t *__restrict__ ssucc, uint32_t ys, uint32_t yz,
		      WalkCaps c, uint32_t ecap, const WalkSink &sink)
{
	DfsResult r{0, 0, 0, false};
	if (ys == WALK_NONE)
		return r;
	const uint32_t uz = yz >> 1;
	if (c.L <= 1) { // the prefix [S] already has L steps
		r.status = ST_LONG;
		return r;
	}
	st.push(0, ys, off[ys ^ 1u]);
	uint32_t depth = 1, exp = 0;
	while (depth > 0) {
		const uint32_t top = depth - 1;
		const uint32_t yt = st.y(top);
		const uint32_t beg = off[yt ^ 1u], end = off[(yt ^ 1u) + 1];
		uint32_t cur = st.cur(top), nxt = WALK_NONE;
		while (cur < end) {
			const uint32_t cand = ssucc[cur++];
			if (cur - 1 > beg && ssucc[cur - 2] == cand)
				continue; // a parallel link: the same step again
			const uint32_t u = cand >> 1;
			if (u == uz) {
				if (cand == yz) {
					nxt = cand;
					break;
				}
				continue; // Z's segment in the other orientation: a walk cannot pass through it
			}
			if (st.on_path(u, depth))
				continue;
			nxt = cand;
			break;
		}
		st.set_cur(top, cur);
		if (nxt == WALK_NONE) { // exhausted: back up
			st.pop(yt);
			depth--;
			continue;
		}
		if (exp == c.E) {
			r.status |= ST_BUDGET;
			break;
		}
		if (exp == ecap) {
			r.handover = true;
			break;
		}
		exp++;
		if (nxt == yz) {
			if (r.walks == c.K) {
				r.status |= ST_MORE;
				break;
			}
			if (EMIT)
				st.write_walk(sink, sink.w0 + r.walks, sink.s0 + r.steps, depth, yz);
			r.walks++;
			r.steps += depth + 1;
			continue;
		}
		if (depth + 1 >= c.L) { // a prefix of L steps that does not end at Z is not extended
			r.status |= ST_LONG;
			continue;
		}
		if (depth == st.cap) {
			r.handover = true;
			break;
		}
		st.push(depth, nxt, off[nxt ^ 1u]);
		depth++;
	}
	while (depth > 0) { // (stopped early: empty tier 2's path set for the next query)
		st.pop(st.y(depth - 1));
		depth--;
	}
	return r;
}

} // namespace povu_hip
