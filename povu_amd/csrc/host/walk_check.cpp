// walk_check.cpp -- the search of a walks query (hip/walk_rules.hpp) on the CPU, built with -fsanitize=address,undefined
// (make walk_check; run by tests/test_walk_rules.py).  Two parts.
//
// The path set of tier 2 (GlobalStack) against std::set: tables of 2^4, 2^5 and 2^11 slots, a lane alone (stride 1) and the
// middle lane of three (stride 3, the words of the other two holding a pattern that must still be there at the end), key pools
// whose homes coincide, lie on both sides of the wrap, or neighbour each other so that a deletion meets entries that must move
// and entries that must stay.  The 16-slot table takes every LIFO sequence over a pool of 8 keys to depth 7 (the tree of all
// stacks, every one pushed and popped); the others take 10^5 random LIFO sequences each, up to L - 1 entries.  After every
// operation on_path of every key of the sequence's pool is what std::set says, and the table is what a second deletion --
// distances from the hole, not from the entry -- leaves; after the last pop every slot is 0.  That second deletion counts four
// events: a probe that wraps, an entry left in place, an entry moved, one moved across the wrap.  In stack order the last two
// never happen (asserted; the reason stands where the sequences are run), so every pool also takes sequences that delete any
// key, and a width on which one of the four never happened there fails the check (--counts prints them).
//
// dfs<EMIT, Stack> on both stacks against a recursive enumeration with std::vector and std::set: random bidirected multigraphs
// of 4 to 24 segments with parallel links and loops, Z's segment met the wrong way round, S on Z's segment, and caps around
// every branch -- K of 1 and at the true count, L of 1, 2 and around the longest walk, E around the true count -- with tier 1's
// frames at their real number and its expansions at 8 and 64.  The hand-over flag is the enumeration's "a 17th frame, or an
// expansion after the ecap-th, before the search ends otherwise"; the emit pass writes into buffers of exactly walks + 1 and
// steps elements; after every search on a GlobalStack its table is all zero.
#include "../hip/walk_rules.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

using namespace povu_hip;

#define REQUIRE(cond) \
	do { \
		if (!(cond)) { \
			fprintf(stderr, "walk_check: %s failed (line %d)\n", #cond, __LINE__); \
			return 1; \
		} \
	} while (0)

static constexpr uint32_t PATTERN = 0xA5C3E1F7u;

static unsigned bits_for(uint64_t max_value) // (common.hpp)
{
	unsigned b = 1;
	while (b < 32 && (uint64_t(1) << b) <= max_value)
		b++;
	return b;
}
static uint32_t tbits_of(uint32_t L) { return std::max(4u, bits_for(2 * (uint64_t)L - 1)); } // (povu_hip_forest_walks)

// ---- a lane's scratch as tier 2 lays it out: `stride` lanes side by side, this lane the one at `lane`
struct LaneScratch {
	uint32_t L, tbits, stride, lane;
	std::vector<uint32_t> sy, sc, tab;
	LaneScratch(uint32_t L_, uint32_t tbits_, uint32_t stride_) : L(L_), tbits(tbits_), stride(stride_), lane(stride_ / 2)
	{
		sy.assign((size_t)L * stride, PATTERN);
		sc.assign((size_t)L * stride, PATTERN);
		tab.assign(((size_t)1 << tbits) * stride, PATTERN);
		for (uint32_t i = 0; i < slots(); i++)
			tab[(size_t)i * stride + lane] = 0;
	}
	uint32_t slots() const { return 1u << tbits; }
	GlobalStack stack() { return GlobalStack{sy.data() + lane, sc.data() + lane, tab.data() + lane, stride, L, tbits}; }
	uint32_t at(uint32_t i) const { return tab[(size_t)i * stride + lane]; }
	bool empty() const
	{
		for (uint32_t i = 0; i < slots(); i++)
			if (at(i))
				return false;
		return true;
	}
	bool others_untouched() const
	{
		for (size_t i = 0; i < tab.size(); i++)
			if (i % stride != lane && tab[i] != PATTERN)
				return false;
		for (size_t i = 0; i < sy.size(); i++)
			if (i % stride != lane && (sy[i] != PATTERN || sc[i] != PATTERN))
				return false;
		return true;
	}
};

// ---- the path set

struct Events {
	uint64_t wrap_probe = 0, shift_across = 0, moved = 0, stayed = 0;
};

// the table of one lane, plain, with the deletion written out: an entry behind the hole moves into it unless its home lies in
// the cyclic interval (hole, entry], both measured in slots forward from the hole
struct PlainSet {
	uint32_t tbits;
	std::vector<uint32_t> t;
	Events *ev;
	uint32_t n() const { return 1u << tbits; }
	uint32_t home(uint32_t u) const { return (uint32_t)(((uint64_t)u * 2654435761ull) & 0xFFFFFFFFull) >> (32 - tbits); }
	uint32_t next(uint32_t i)
	{
		if (i + 1 == n()) {
			ev->wrap_probe++;
			return 0;
		}
		return i + 1;
	}
	void insert(uint32_t u)
	{
		uint32_t i = home(u);
		while (t[i])
			i = next(i);
		t[i] = u + 1;
	}
	void erase(uint32_t u)
	{
		uint32_t hole = home(u);
		while (t[hole] != u + 1)
			hole = next(hole);
		for (uint32_t j = (hole + 1) % n(); t[j]; j = (j + 1) % n()) {
			const uint32_t h = home(t[j] - 1);
			const uint32_t to_home = (h + n() - hole) % n(), to_entry = (j + n() - hole) % n(); // slots forward from the hole
			if (to_home >= 1 && to_home <= to_entry) { // h in (hole, j]
				ev->stayed++;
				continue;
			}
			ev->moved++;
			if (j < hole)
				ev->shift_across++;
			t[hole] = t[j];
			hole = j;
		}
		t[hole] = 0;
	}
};

// a LIFO of keys on a GlobalStack beside a std::set and the plain table
struct SetRun {
	LaneScratch ws;
	GlobalStack st;
	PlainSet plain;
	std::set<uint32_t> on;
	std::vector<uint32_t> stack;
	SetRun(uint32_t L, uint32_t tbits, uint32_t stride, Events *ev) : ws(L, tbits, stride), st(ws.stack()), plain{tbits, std::vector<uint32_t>(1u << tbits, 0), ev} {}
	// `u`: the key just pushed or popped.  What an operation may change lies in the cluster of u's home, no longer than the
	// stack was: a wide table is compared over that stretch only (and as a whole when a sequence ends)
	bool same(const std::vector<uint32_t> &pool, uint32_t u) const
	{
		const uint32_t n = ws.slots(), reach = (uint32_t)stack.size() + 2;
		if (2 * reach + 1 >= n || n <= 64) {
			if (!same_tables())
				return false;
		} else {
			for (uint32_t d = 0; d <= 2 * reach; d++) {
				const uint32_t i = (plain.home(u) + n - reach + d) % n;
				if (ws.at(i) != plain.t[i])
					return false;
			}
		}
		return same_answers(pool);
	}
	bool same_tables() const
	{
		for (uint32_t i = 0; i < ws.slots(); i++)
			if (ws.at(i) != plain.t[i])
				return false;
		return true;
	}
	bool same_answers(const std::vector<uint32_t> &pool) const
	{
		for (uint32_t u : pool)
			if (st.on_path(u, (uint32_t)stack.size()) != (on.count(u) != 0))
				return false;
		return true;
	}
	void push(uint32_t u)
	{
		st.push((uint32_t)stack.size(), 2 * u + (u & 1u), 7);
		plain.insert(u);
		on.insert(u);
		stack.push_back(u);
	}
	void pop()
	{
		const uint32_t u = stack.back();
		st.pop(2 * u + (u & 1u)); // (the step as push wrote it)
		plain.erase(u);
		on.erase(u);
		stack.pop_back();
	}
};

// the first `want[k]` keys whose home is homes[k], for every k, in ascending key order
static std::vector<uint32_t> pool_of(uint32_t tbits, const std::vector<uint32_t> &homes, const std::vector<uint32_t> &want)
{
	Events none;
	PlainSet p{tbits, {}, &none};
	std::vector<uint32_t> got(homes.size(), 0), pool;
	size_t need = 0;
	for (uint32_t w : want)
		need += w;
	for (uint32_t u = 0; pool.size() < need; u++)
		for (size_t k = 0; k < homes.size(); k++)
			if (p.home(u) == homes[k] && got[k] < want[k]) {
				got[k]++;
				pool.push_back(u);
			}
	return pool;
}

static int every_sequence(SetRun &r, const std::vector<uint32_t> &pool, std::vector<bool> &used, uint32_t depth_max)
{
	if (r.stack.size() == depth_max)
		return 0;
	for (size_t k = 0; k < pool.size(); k++) {
		if (used[k])
			continue;
		used[k] = true;
		r.push(pool[k]);
		REQUIRE(r.same(pool, pool[k]));
		if (every_sequence(r, pool, used, depth_max))
			return 1;
		r.pop();
		REQUIRE(r.same(pool, pool[k]));
		used[k] = false;
	}
	return 0;
}

// `n_seq` random sequences of pushes and pops on up to L - 1 keys at a time, the popped key the top (`lifo`) or any.  A sequence
// works on a part of the pool, and every key of that part is looked up after every operation: mostly up to 15 keys, now and then
// 64, and on the pool of spread keys now and then all L - 1.  (On a pool of clustered keys a sequence of L - 1 = 1023 makes every
// look-up a scan of the cluster, 10^9 slot reads a sequence: the wide table meets its clusters 64 keys long.)
static int random_sequences(SetRun &r, const std::vector<uint32_t> &pool, uint32_t L, uint32_t n_seq, bool lifo, bool is_spread, std::mt19937 &rng)
{
	std::vector<uint32_t> keys(pool);
	for (uint32_t s = 0; s < n_seq; s++) {
		uint32_t m = 2 + rng() % 14;
		if (s % 256 == 0)
			m = 64;
		if (is_spread && s % 4096 == 1)
			m = L - 1;
		m = std::min<uint32_t>(m, L - 1);
		for (uint32_t k = 0; k < m; k++) // (m keys of the pool, drawn without replacement)
			std::swap(keys[k], keys[k + rng() % (keys.size() - k)]);
		const std::vector<uint32_t> part(keys.begin(), keys.begin() + m);
		std::vector<uint32_t> free_keys(part);
		const uint32_t ops = m > 64 ? m + 200 : 3 * m;
		for (uint32_t o = 0; o < ops || !r.stack.empty(); o++) {
			const bool can_push = o < ops && !free_keys.empty(), can_pop = !r.stack.empty();
			const bool do_push = can_push && (!can_pop || rng() % 100 < (o < m ? 80u : 45u));
			uint32_t u;
			if (do_push) {
				const size_t k = rng() % free_keys.size();
				u = free_keys[k];
				r.push(u);
				free_keys[k] = free_keys.back();
				free_keys.pop_back();
			} else {
				if (!lifo)
					std::swap(r.stack[rng() % r.stack.size()], r.stack.back());
				u = r.stack.back();
				free_keys.push_back(u);
				r.pop();
			}
			REQUIRE(r.stack.size() <= L - 1 && r.same(part, u));
		}
		if (r.ws.slots() <= 64 || s % 8 == 0 || s + 1 == n_seq) // (what a sequence leaves behind stays for the next whole look)
			REQUIRE(r.ws.empty() && r.same_tables());
	}
	return 0;
}

static int path_set(bool print_counts)
{
	std::mt19937 rng(20260612);
	for (uint32_t tbits : {4u, 5u, 11u}) {
		Events lifo, any;
		const uint32_t n = 1u << tbits, L = n / 2, last = n - 1;
		REQUIRE(tbits_of(L) == tbits && (tbits == 4 || tbits_of(L + 1) == tbits + 1));
		// homes: all one slot (the last: every probe wraps); two before and two after the wrap; neighbours in the middle and
		// around the wrap (an entry at home behind a hole stays, one pushed along moves)
		std::vector<std::vector<uint32_t>> pools;
		if (tbits == 4) {
			pools.push_back(pool_of(tbits, {last}, {8}));
			pools.push_back(pool_of(tbits, {5}, {8}));
			pools.push_back(pool_of(tbits, {last - 1, last, 0, 1}, {2, 2, 2, 2}));
			pools.push_back(pool_of(tbits, {last - 2, last - 1, last, 0, 1}, {1, 2, 2, 1, 2}));
			pools.push_back(pool_of(tbits, {6, 7, 8, 9}, {3, 2, 2, 1}));
		} else {
			const uint32_t m = L - 1;
			pools.push_back(pool_of(tbits, {last}, {m}));
			pools.push_back(pool_of(tbits, {last - 1, last, 0, 1}, {m / 4 + 1, m / 4 + 1, m / 4 + 1, m / 4 + 1}));
			std::vector<uint32_t> homes, want;
			for (uint32_t k = 0; k < 12; k++) {
				homes.push_back((last - 5 + k) % n);
				want.push_back(m / 12 + 1);
			}
			pools.push_back(pool_of(tbits, homes, want));
			std::vector<uint32_t> spread(m); // consecutive vertex indices, as a graph has them: homes all over the table
			for (uint32_t k = 0; k < m; k++)
				spread[k] = 1000 + k;
			pools.push_back(spread);
		}
		for (uint32_t stride : {1u, 3u})
			for (const auto &pool : pools) {
				const bool is_spread = tbits != 4 && &pool == &pools.back();
				SetRun r(L, tbits, stride, &lifo);
				if (tbits == 4) {
					std::vector<bool> used(pool.size(), false);
					REQUIRE(pool.size() == 8 && L == 8);
					if (every_sequence(r, pool, used, L - 1))
						return 1;
					REQUIRE(r.stack.empty() && r.ws.empty());
				} else if (random_sequences(r, pool, L, 100000 / (2 * (uint32_t)pools.size()) + 1, true, is_spread, rng)) {
					return 1;
				}
				// the set as a set: the key that leaves is any key of it.  (In stack order -- all a search does -- no entry ever
				// moves: the table is what pushing the stack from the bottom gives, so when an entry older than the one that leaves
				// was pushed, the hole was empty too, and it did not probe past it.  Only this part reaches the moves.)
				r.plain.ev = &any;
				if (random_sequences(r, pool, L, tbits == 4 ? 4000 : 2000, false, is_spread, rng))
					return 1;
				REQUIRE(r.ws.others_untouched());
			}
		if (print_counts)
			for (const Events *e : {&lifo, &any})
				printf("tbits %u, %s: wrapping probes %llu, shifts across the wrap %llu, moved %llu, left in place %llu\n", tbits,
				       e == &lifo ? "stack order" : "any order", (unsigned long long)e->wrap_probe, (unsigned long long)e->shift_across,
				       (unsigned long long)e->moved, (unsigned long long)e->stayed);
		REQUIRE(lifo.wrap_probe > 0 && lifo.stayed > 0);
		REQUIRE(lifo.moved == 0 && lifo.shift_across == 0);
		REQUIRE(any.wrap_probe > 0);
		REQUIRE(any.shift_across > 0);
		REQUIRE(any.moved > 0);
		REQUIRE(any.stayed > 0);
	}
	return 0;
}

// ---- the DFS

struct Graph {
	uint32_t V;
	std::vector<uint32_t> off, ssucc, vid;
};
static Graph random_graph(std::mt19937 &rng)
{
	Graph g;
	g.V = 4 + rng() % 21;
	const uint32_t nS = 2 * g.V;
	std::vector<std::vector<uint32_t>> adj(nS);
	auto link = [&](uint32_t a, uint32_t b) {
		adj[a].push_back(b);
		if (a != b)
			adj[b].push_back(a);
	};
	const uint32_t shape = rng() % 4;
	if (shape <= 1) // a backbone, forwards: walks as deep as the graph is long
		for (uint32_t u = 0; u + 1 < g.V; u++)
			link(2 * u + 1, 2 * (u + 1));
	const uint32_t n_links = shape == 0 ? rng() % (g.V / 2 + 1) : shape == 1 ? g.V / 2 + rng() % g.V : g.V + rng() % (g.V + 1);
	for (uint32_t k = 0; k < n_links; k++) {
		const uint32_t a = rng() % nS, b = rng() % nS;
		link(a, b);
		if (rng() % 4 == 0)
			link(a, b); // parallel
	}
	g.off.assign(nS + 1, 0);
	for (uint32_t x = 0; x < nS; x++) {
		std::sort(adj[x].begin(), adj[x].end());
		g.off[x + 1] = g.off[x] + (uint32_t)adj[x].size();
		g.ssucc.insert(g.ssucc.end(), adj[x].begin(), adj[x].end());
	}
	for (uint32_t u = 0; u < g.V; u++)
		g.vid.push_back(3 * u + 7);
	return g;
}

// the enumeration: what walks_ref.py says, recursively
struct Enum {
	const Graph &g;
	uint32_t ys, yz;
	uint64_t K, L, E;
	uint32_t frames_cap, ecap; // tier 1's limits, watched only
	std::vector<std::vector<uint32_t>> walks;
	uint8_t status = 0;
	uint64_t exp = 0;
	bool stopped = false, handover = false, wrong_way = false;
	uint32_t max_frames = 0;
	std::vector<uint32_t> path;
	std::set<uint32_t> on;
	void from_top()
	{
		const uint32_t exit = path.back() ^ 1u;
		const std::set<uint32_t> next(g.ssucc.begin() + g.off[exit], g.ssucc.begin() + g.off[exit + 1]);
		for (uint32_t cand : next) {
			const uint32_t u = cand >> 1;
			if (u == (yz >> 1) && cand != yz) {
				wrong_way = true;
				continue;
			}
			if (cand != yz && on.count(u))
				continue;
			if (exp == E) {
				status |= ST_BUDGET;
				stopped = true;
				return;
			}
			if (exp == ecap)
				handover = true; // (watched: this search goes on as tier 2 would)
			exp++;
			if (cand == yz) {
				if (walks.size() == K) {
					status |= ST_MORE;
					stopped = true;
					return;
				}
				walks.push_back(path);
				walks.back().push_back(yz);
				continue;
			}
			if (path.size() + 1 >= L) {
				status |= ST_LONG;
				continue;
			}
			if (path.size() == frames_cap)
				handover = true;
			path.push_back(cand);
			on.insert(u);
			max_frames = std::max<uint32_t>(max_frames, (uint32_t)path.size());
			from_top();
			path.pop_back();
			on.erase(u);
			if (stopped)
				return;
		}
	}
	void run()
	{
		if ((ys >> 1) == (yz >> 1))
			return;
		if (L <= 1) {
			status = ST_LONG;
			return;
		}
		path.push_back(ys);
		on.insert(ys >> 1);
		max_frames = 1;
		from_top();
	}
	uint64_t steps() const
	{
		uint64_t s = 0;
		for (const auto &w : walks)
			s += w.size();
		return s;
	}
	uint32_t longest() const
	{
		size_t l = 0;
		for (const auto &w : walks)
			l = std::max(l, w.size());
		return (uint32_t)l;
	}
};

struct DfsTally {
	uint64_t searches = 0, by_frames = 0, by_expansions = 0, full_stack_kept = 0, last_expansion_kept = 0, wrong_way = 0, same_segment = 0,
		 stopped_more = 0, stopped_budget = 0, stopped_handover = 0, budget_beats_handover = 0;
};

// count pass, then the emit pass into buffers of exactly the counted size; the walks must be the enumeration's
template <class Stack> static int both_passes(Stack &st, const Graph &g, uint32_t ys, uint32_t yz, WalkCaps c, uint32_t ecap, const Enum &want, bool &handed)
{
	const WalkSink none{};
	const DfsResult r = dfs<false>(st, g.off.data(), g.ssucc.data(), ys, yz, c, ecap, none);
	handed = r.handover;
	if (r.handover)
		return 0;
	REQUIRE(r.walks == want.walks.size() && r.steps == want.steps() && r.status == want.status);
	std::vector<uint32_t> step_off((size_t)r.walks + 1, PATTERN), step_id(r.steps, PATTERN);
	std::vector<uint8_t> step_or(r.steps, 0xEE);
	const WalkSink sink{step_off.data(), step_id.data(), step_or.data(), g.vid.data(), 0, r.walks, 0, r.steps};
	const DfsResult e = dfs<true>(st, g.off.data(), g.ssucc.data(), ys, yz, c, ecap, sink);
	REQUIRE(e.walks == r.walks && e.steps == r.steps && e.status == r.status && !e.handover);
	REQUIRE(step_off[r.walks] == PATTERN); // (the caller's: the total)
	uint32_t at = 0;
	for (size_t w = 0; w < want.walks.size(); w++) {
		REQUIRE(step_off[w] == at);
		for (uint32_t y : want.walks[w]) {
			REQUIRE(step_id[at] == g.vid[y >> 1] && step_or[at] == (y & 1u));
			at++;
		}
	}
	return 0;
}

static int one_search(const Graph &g, uint32_t ys, uint32_t yz, WalkCaps c, uint32_t ecap_t1, std::mt19937 &rng, DfsTally &t)
{
	const bool none = (ys >> 1) == (yz >> 1); // (the front end hands such a query over as "no query")
	const uint32_t ecap = std::min(c.E, ecap_t1);
	Enum want{g, ys, yz, c.K, c.L, c.E, T1_DEPTH, ecap};
	want.run();
	t.searches++;
	t.wrong_way += want.wrong_way;
	t.same_segment += none;
	// tier 2: room for L frames, all E expansions
	const uint32_t stride = rng() % 2 ? 3 : 1;
	LaneScratch ws(c.L, tbits_of(c.L), stride);
	GlobalStack gs = ws.stack();
	bool handed = false;
	if (both_passes(gs, g, none ? WALK_NONE : ys, yz, c, c.E, want, handed))
		return 1;
	REQUIRE(!handed && ws.empty() && ws.others_untouched());
	t.stopped_more += (want.status & ST_MORE) != 0;
	t.stopped_budget += (want.status & ST_BUDGET) != 0;
	// ... and stopped where tier 1 would stop: the set is left empty then too
	if (both_passes(gs, g, none ? WALK_NONE : ys, yz, c, ecap, want, handed))
		return 1;
	REQUIRE(ws.empty() && ws.others_untouched());
	t.stopped_handover += handed;
	// tier 1: its real number of frames, lane t of a workgroup
	static std::vector<uint32_t> sy((size_t)T1_DEPTH * WALK_TPB, PATTERN), sc((size_t)T1_DEPTH * WALK_TPB, PATTERN); // (a workgroup's)
	LaneStack ls{sy.data(), sc.data(), (uint32_t)(rng() % WALK_TPB)};
	if (both_passes(ls, g, none ? WALK_NONE : ys, yz, c, ecap, want, handed))
		return 1;
	REQUIRE(handed == want.handover);
	for (uint32_t k = 0; k < T1_DEPTH; k++)
		sy[k * WALK_TPB + ls.t] = sc[k * WALK_TPB + ls.t] = PATTERN;
	if (rng() % 8 == 0) // (the other lanes' frames)
		for (size_t i = 0; i < sy.size(); i++)
			REQUIRE(sy[i] == PATTERN && sc[i] == PATTERN);
	if (handed) {
		t.by_frames += want.max_frames > T1_DEPTH;
		t.by_expansions += want.exp > ecap;
	} else {
		t.full_stack_kept += want.max_frames == T1_DEPTH;
		t.last_expansion_kept += want.exp == ecap && !(want.status & ST_BUDGET);
		t.budget_beats_handover += want.exp == ecap && (want.status & ST_BUDGET) != 0;
	}
	return 0;
}

static int searches(bool print_counts)
{
	std::mt19937 rng(7);
	DfsTally t;
	const uint32_t BIG = 1u << 20;
	for (uint32_t round = 0; round < 2000; round++) {
		const Graph g = random_graph(rng);
		const uint32_t nS = 2 * g.V;
		uint32_t ys = rng() % nS, yz = rng() % nS;
		if (round % 3 == 0) // from the first segment to the last: the backbone's whole length
			ys = 0, yz = 2 * (g.V - 1);
		if (round % 97 == 0)
			yz = ys ^ 1u;
		// the search without caps worth the name
		Enum full{g, ys, yz, BIG, 1000, 20000, BIG, BIG};
		full.run();
		const uint32_t W = (uint32_t)full.walks.size(), X = (uint32_t)full.exp, LW = full.longest(), D = full.max_frames;
		const uint32_t LBIG = 40; // (more steps than a graph here has segments; a table of 128 slots)
		std::vector<WalkCaps> caps = {{BIG, 1000, 20000}, {1, LBIG, 20000}, {std::max(1u, W), LBIG, 20000}, {W + 1, LBIG, 20000},
					      {std::max(2u, W) - 1, LBIG, 20000}, {BIG, 1, 20000}, {BIG, 2, 20000}};
		for (int d = -1; d <= 1; d++) {
			if ((int)LW + d >= 1)
				caps.push_back({BIG, LW + d, 20000});
			if ((int)D + d >= 1)
				caps.push_back({BIG, D + 1 + d, 20000}); // (the deepest prefix, whether or not it ends at Z)
			if ((int)X + d >= 1)
				caps.push_back({BIG, LBIG, X + d});
		}
		for (uint32_t e : {7u, 8u, 9u, 63u, 64u, 65u})
			caps.push_back({BIG, LBIG, e}); // (the budget at tier 1's own limit: BUDGET wins over the hand-over)
		caps.push_back({1 + (uint32_t)(rng() % 4), 2 + (uint32_t)(rng() % 20), 1 + (uint32_t)(rng() % 100)});
		for (const WalkCaps &c : caps)
			for (uint32_t ecap : {8u, 64u})
				if (one_search(g, ys, yz, c, ecap, rng, t))
					return 1;
	}
	if (print_counts)
		printf("searches %llu: handed over for a 17th frame %llu, for an expansion %llu; kept with 16 frames %llu, with the ecap-th "
		       "expansion its last %llu; BUDGET at ecap %llu; Z the wrong way round %llu; S on Z's segment %llu; MORE %llu, BUDGET %llu, "
		       "tier 2 stopped at tier 1's limits %llu\n",
		       (unsigned long long)t.searches, (unsigned long long)t.by_frames, (unsigned long long)t.by_expansions,
		       (unsigned long long)t.full_stack_kept, (unsigned long long)t.last_expansion_kept, (unsigned long long)t.budget_beats_handover,
		       (unsigned long long)t.wrong_way, (unsigned long long)t.same_segment, (unsigned long long)t.stopped_more,
		       (unsigned long long)t.stopped_budget, (unsigned long long)t.stopped_handover);
	REQUIRE(t.by_frames > 0 && t.by_expansions > 0 && t.full_stack_kept > 0 && t.last_expansion_kept > 0 && t.budget_beats_handover > 0);
	REQUIRE(t.wrong_way > 0 && t.same_segment > 0 && t.stopped_more > 0 && t.stopped_budget > 0 && t.stopped_handover > 0);
	return 0;
}

int main(int argc, char **argv)
{
	const bool print_counts = argc > 1 && !strcmp(argv[1], "--counts");
	if (path_set(print_counts))
		return 1;
	if (searches(print_counts))
		return 1;
	printf("walk_check: ok\n");
	return 0;
}
