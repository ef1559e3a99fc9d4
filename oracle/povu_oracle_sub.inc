/*
 * povu_oracle_sub.inc -- TEST INFRASTRUCTURE ONLY; included by povu_oracle.c (it uses its tree_meta and text helpers).
 *
 * The three INSERTING passes of `povu decompose -s` (app/subcommand/decompose.cpp:63-70), restated sequentially and
 * literally: find_concealed (src/povu/algorithms/concealed.cpp:1198-1243), find_midi (midi.cpp:225-268) and
 * find_smothered (smothered.cpp:385-432), over gen_tree_meta (src/povu/graph/tree_utils.cpp:674-688) and the PVST
 * container of include/povu/graph/pvst.hpp:719-900 (children are vectors in insertion order; add_edge appends, del_edge
 * erases the first match).
 *
 * PARITY UNPINNED: no test, fixture or golden file of the reference holds a C, M or S line; the reference's own code is
 * the only statement of these passes, and parts of it have no defined behaviour.  What is restated LITERALLY although
 * it is plainly an accident:
 *   - add_concealed decides "is_leaf" from the SPANNING TREE's children of the vertex whose index is the flubble's
 *     PVST index (concealed.cpp:1188);
 *   - the two nestings "in relation to z" attach the CONCEALED vertex below the child flubble (add_edge(c, sl),
 *     concealed.cpp:1077,1103): the concealed vertex is then listed under two parents and the child under none;
 *   - add_conc_zi asks for cl_e::ai_branch where zi_branch is meant (concealed.cpp:1134): branch slubbles of z are
 *     never nested (the reference prints "sl type: unknown" to stderr for each);
 *   - ji_trunk returns before its validation loop (concealed.cpp:755-760);
 *   - add_midi compares spanning-tree depths at the PVST indices of the two concealed vertices (midi.cpp:31-56,
 *     MidiBubble::get_bounds pvst.hpp:693-702);
 *   - smothered::nest erases from the children vector it is iterating over (smothered.cpp:332-344): restated as
 *     libstdc++ executes it on a vector of integers (the element behind the erased one is skipped, the loop runs to the
 *     OLD end over the stale tail).
 * What the reference leaves UNDEFINED and this file DEFINES:
 *   - depth[] read at INVALID_IDX or at an index past the tree (can_contain :365 with lo = INVALID, override_ji_trunk
 *     :639 with hi = INVALID, add_midi with a PVST index >= the tree's vertex count): the depth is taken as +infinity;
 *   - find_midi's branch case (midi.cpp:186-190,207-221) pushes spanning-tree indices where gen_midi_bub expects PVST
 *     indices and casts whatever PVST vertex sits there to Concealed: no midi bubble comes out of the branch case;
 *   - ai_trunk sorts its candidates by LCA with std::sort and takes the last (concealed.cpp:508-514): with equal LCAs
 *     the source that survives only enters Concealed::bounds_, which nothing downstream reads for a vertex of that kind
 *     -- a stable sort is used.
 * compute_LoA (tree_utils.cpp:224-273) is a std::priority_queue over back-edge targets, restated with libstdc++'s own heap
 * steps (push_heap; pop_heap = __adjust_heap to the bottom, then __push_heap).  Without self-loop back edges its answers
 * do not depend on how the heap breaks ties: when vertex v is reached (descending index) every target still queued is a
 * proper ancestor of v (a target t < v < source lies on v's root path because the source is in subtree(t), an interval
 * of indices), so the depths in the heap are distinct but for copies of one vertex.  A back edge whose source is its
 * target (spanning_tree.cpp:387-395) is pushed at its own vertex and never popped: it stays in the queue as a stale
 * entry, may become lo[] of vertices it is no ancestor of, and there the order among equal depths is the heap's.
 */

/* which rule fired, summed over all calls since the last orc_sub_stats(reset): coverage evidence for the tests */
enum { SS_AI_TRUNK, SS_AI_BRANCH, SS_ZI_TRUNK, SS_ZI_BRANCH, SS_NEST_TRUNK_AI, SS_NEST_BRANCH_AI, SS_NEST_TRUNK_ZI, SS_ZI_BRANCH_UNNESTED,
       SS_LEAF_BY_TREE_IDX, SS_MIDI, SS_MIDI_SAME_KIND, SS_MIDI_NEST, SS_SMO_G_TRUNK_TGT, SS_SMO_G_TRUNK_SRC, SS_SMO_G_BRANCH,
       SS_SMO_S_TRUNK, SS_SMO_S_BRANCH_SRC, SS_SMO_S_BRANCH_TGT, SS_SMO_NEST, SS_SMO_STALE_READ, SS_DEPTH_OF_INVALID, SS_SELF_LOOP_IN_LOA,
       SS_OVERRIDE_JI, SS_NEST_OVER_PINNED, SS_N };
static uint64_t g_sub_stats[SS_N];
#define SS_INC(i) ((void)__atomic_fetch_add(&g_sub_stats[i], 1, __ATOMIC_RELAXED))
void orc_sub_stats(uint64_t *out, int reset)
{
	if (out)
		memcpy(out, g_sub_stats, sizeof g_sub_stats);
	if (reset)
		memset(g_sub_stats, 0, sizeof g_sub_stats);
}

/* how WIDE the children vectors were where the reference copies or walks one, since the last orc_sub_widths(reset): what
 * the tests of the device's splice (one wave per flubble, 64 children a round) need to know of an input.  "max" words hold
 * the greatest value seen, "calls" words count calls, "sum" words add up; an index or a round is stored + 1 (0 = never).
 * Per nesting kind NK_* (SW_NK words each, kind-major):
 *   copy_len   max   length of the copied vector the nesting runs over
 *   movers     max   children that leave in one call;     stayers  max  children that stay
 *   mover_ge64 calls with a mover at index >= 64 of the copy
 *   stay_behind_ge64 calls with a stayer at index >= 64 behind a mover (write cursor != read index in a later round)
 *   mixed_round calls where one round of 64 holds movers and stayers
 *   mover_idx  max   index + 1 of a mover;   stay_behind_idx  max  index + 1 of a stayer behind a mover
 *   mixed_rnd  max   round + 1 that holds movers and stayers
 *   tail_movers calls over more than 64 children whose last round holds movers only
 *   reserve_copy max entries the destination's vector holds when a round's movers do not fit and it is copied, under the
 *              device's rule (room for the round's movers at once, capacity doubling from 4); 0 for the z-side trunk
 *              nesting, which pushes into the children instead
 *   stay_behind_n max stayers at an index >= 64 behind a mover in one call
 * then the scalar words SW_PUSH_LEN .. (see the enum). */
enum { NK_AI_TRUNK, NK_AI_BRANCH, NK_ZI_TRUNK, NK_MIDI, NK_N };
enum { SWK_COPY_LEN, SWK_MOVERS, SWK_STAYERS, SWK_MOVER_GE64, SWK_STAY_BEHIND_GE64, SWK_MIXED_ROUND, SWK_MOVER_IDX, SWK_STAY_BEHIND_IDX,
       SWK_MIXED_RND, SWK_TAIL_MOVERS, SWK_RESERVE_COPY, SWK_STAY_BEHIND_N, SW_NK };
enum { SW_PUSH_LEN = NK_N * SW_NK, /* max length of a vector at a push onto it */
       SW_PUSH_FULL_F,	    /* max length of a FULL vector at a push, by the device's rule (capacity = seeded length, then doubling from 4): */
       SW_PUSH_FULL_C,	    /*   of a find_flubbles vertex, a concealed, a smothered one (the pushes of a nesting's movers */
       SW_PUSH_FULL_S,	    /*   under a new vertex are counted by reserve_copy instead) */
       SW_FIRST_PUSH_SEEDED, /* max length of a seeded vector at the first push onto it */
       SW_MIDI_FIRST_IDX, SW_MIDI_SECOND_IDX, /* find_midi: max index + 1 of the first / second trunk concealed child */
       SW_MIDI_NTRUNK,	    /* max trunk concealed children of one flubble */
       SW_MIDI_SPLIT_ROUNDS, /* calls: the first two in different rounds of 64 */
       SW_MIDI_THIRD_LATER,  /* calls: a third one in a later round than the first two */
       SW_MIDI_FIND_LEN,	    /* max length of a vector find_midi walks */
       SW_SMO_OLD_END, SW_SMO_ERASURES, SW_SMO_STALE, /* smothered::nest: max old_end, erasures and stale reads in one call */
       SW_CN_PER_FLUBBLE, SW_SMO_PER_CN, /* max concealed records of a flubble, smothered records of a concealed vertex */
       SW_PINNED_WIDE, SW_PINNED_LEN,	  /* nest_over_pinned: calls over >= 64 children, max length */
       SW_CN_LIST,	    /* sum: flubbles with records of their own or a pinned vertex pushed in (the device's first list) */
       SW_N_CONCEALED, SW_N_SMO_CN, /* sum: concealed vertices; those with smothered records */
       SW_N };
static uint64_t g_sub_w[SW_N];
static void sw_max(int i, uint64_t v)
{
	uint64_t o = __atomic_load_n(&g_sub_w[i], __ATOMIC_RELAXED);
	while (o < v && !__atomic_compare_exchange_n(&g_sub_w[i], &o, v, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED))
		;
}
#define SW_ADD(i, v) ((void)__atomic_fetch_add(&g_sub_w[i], (uint64_t)(v), __ATOMIC_RELAXED))
void orc_sub_widths(uint64_t *out, int reset)
{
	if (out)
		memcpy(out, g_sub_w, sizeof g_sub_w);
	if (reset)
		memset(g_sub_w, 0, sizeof g_sub_w);
}
/* one nesting: moved[k] says whether child k of the copy left */
static void sw_nesting(int kind, const uint8_t *moved, uint32_t nch)
{
	const int b = kind * SW_NK;
	uint32_t nm = 0, first_m = NIL, dn = 0, dcap = 0, n_behind = 0;
	int ge64 = 0, behind = 0, mixed = 0;
	sw_max(b + SWK_COPY_LEN, nch);
	for (uint32_t r0 = 0; r0 < nch; r0 += 64) {
		uint32_t m = 0, st = 0;
		for (uint32_t k = r0; k < nch && k < r0 + 64; k++) {
			if (moved[k]) {
				m++;
				if (first_m == NIL)
					first_m = k;
				if (k >= 64)
					ge64 = 1;
				sw_max(b + SWK_MOVER_IDX, (uint64_t)k + 1);
			} else {
				st++;
				if (first_m != NIL) {
					sw_max(b + SWK_STAY_BEHIND_IDX, (uint64_t)k + 1);
					if (k >= 64)
						behind = 1, n_behind++;
				}
			}
		}
		if (m && st) {
			mixed = 1;
			sw_max(b + SWK_MIXED_RND, (uint64_t)r0 / 64 + 1);
		}
		if (m && !st && r0 + 64 >= nch && nch > 64)
			SW_ADD(b + SWK_TAIL_MOVERS, 1);
		if (m && kind != NK_ZI_TRUNK) { /* Splice::reserve(dest, m) of the device */
			if (dn + m > dcap) {
				sw_max(b + SWK_RESERVE_COPY, dn);
				if (!dcap)
					dcap = 4;
				while (dcap < dn + m)
					dcap *= 2;
			}
			dn += m;
		}
		nm += m;
	}
	sw_max(b + SWK_MOVERS, nm);
	sw_max(b + SWK_STAYERS, nch - nm);
	sw_max(b + SWK_STAY_BEHIND_N, n_behind);
	SW_ADD(b + SWK_MOVER_GE64, ge64);
	SW_ADD(b + SWK_STAY_BEHIND_GE64, behind);
	SW_ADD(b + SWK_MIXED_ROUND, mixed);
}

/* ---- gen_tree_meta beyond the bracket table: depth (tree_utils.cpp:576-598), lo (:224-273), LCA (:330-475) */
typedef struct {
	tree_meta m;
	uint32_t *depth, *lo;
	uint32_t lg, nb; /* levels of the sparse table, blocks of SM_BLK vertices */
	uint32_t **sp;	 /* sp[k][b] = shallowest vertex of the blocks [b, b + 2^k), first one on ties (a table over the vertices
			    themselves is n lg n words: 1.6 GB for a chromosome) */
} sub_meta;

#define SM_BLK 16u
static uint32_t sm_depth(const orc_tree *t, const sub_meta *s, uint32_t v)
{
	if (v >= t->n)
		SS_INC(SS_DEPTH_OF_INVALID);
	return v < t->n ? s->depth[v] : 0xFFFFFFFFu; /* (defined here: see the header) */
}

static void sub_meta_build(const orc_tree *t, sub_meta *s)
{
	const uint32_t n = t->n;
	memset(s, 0, sizeof *s);
	tree_meta_build(t, &s->m);
	s->depth = xcalloc((size_t)n + 1, 4);
	for (uint32_t v = 1; v < n; v++) /* a parent's idx is smaller than its children's */
		s->depth[v] = t->par[v] == NIL ? 0 : s->depth[t->par[v]] + 1;
	/* compute_LoA with a binary max-heap on depth */
	s->lo = xmalloc(((size_t)n + 1) * 4);
	uint32_t *heap = xmalloc(((size_t)t->n_be + 2) * 4), hn = 0;
	for (uint32_t v = n; v-- > 0;) {
		while (hn && heap[0] == v) { /* pq.pop() as libstdc++ runs it: __pop_heap -> __adjust_heap -> __push_heap */
			const uint32_t value = heap[hn - 1], len = hn - 1; /* (the old top goes to the slot that is dropped) */
			hn = len;
			if (!len)
				break;
			uint32_t hole = 0, child = 0;
			while (child < (len - 1) / 2) {
				child = 2 * (child + 1);
				if (s->depth[heap[child]] < s->depth[heap[child - 1]])
					child--;
				heap[hole] = heap[child];
				hole = child;
			}
			if ((len & 1) == 0 && child == (len - 2) / 2) {
				child = 2 * (child + 1);
				heap[hole] = heap[child - 1];
				hole = child - 1;
			}
			while (hole > 0 && s->depth[heap[(hole - 1) / 2]] < s->depth[value]) {
				heap[hole] = heap[(hole - 1) / 2];
				hole = (hole - 1) / 2;
			}
			heap[hole] = value;
		}
		s->lo[v] = hn ? heap[0] : NIL;
		for (uint32_t b = s->m.o_off[v]; b < s->m.o_off[v + 1]; b++) {
			const uint32_t j = s->m.o_adj[b];
			if (t->be_type[j] != ORC_BE_BACK)
				continue;
			uint32_t i = hn++;
			const uint32_t x = t->be_tgt[j];
			if (x == v)
				SS_INC(SS_SELF_LOOP_IN_LOA);
			while (i && s->depth[heap[(i - 1) / 2]] < s->depth[x]) {
				heap[i] = heap[(i - 1) / 2];
				i = (i - 1) / 2;
			}
			heap[i] = x;
		}
	}
	free(heap);
	/* sparse table of the shallowest vertex over index ranges (vertex idx = pre-order rank), one entry per block */
	const uint32_t nb = (n + SM_BLK - 1) / SM_BLK;
	s->nb = nb;
	uint32_t lg = 1;
	while ((1u << lg) < nb)
		lg++;
	s->lg = lg + 1;
	s->sp = xcalloc(s->lg, sizeof *s->sp);
	s->sp[0] = xmalloc(((size_t)nb + 1) * 4);
	for (uint32_t q = 0; q < nb; q++) {
		uint32_t best = q * SM_BLK;
		for (uint32_t v = best + 1; v < n && v < (q + 1) * SM_BLK; v++)
			if (s->depth[v] < s->depth[best])
				best = v;
		s->sp[0][q] = best;
	}
	for (uint32_t k = 1; k < s->lg; k++) {
		if ((1ull << k) > nb) {
			s->lg = k;
			break;
		}
		s->sp[k] = xmalloc(((size_t)nb + 1) * 4);
		const uint32_t span = 1u << k, half = span >> 1;
		for (uint32_t i = 0; i + span <= nb; i++) {
			const uint32_t a = s->sp[k - 1][i], b = s->sp[k - 1][i + half];
			s->sp[k][i] = s->depth[b] < s->depth[a] ? b : a;
		}
	}
}
static void sub_meta_free(sub_meta *s)
{
	tree_meta_free(&s->m);
	free(s->depth);
	free(s->lo);
	for (uint32_t k = 0; k < s->lg; k++)
		free(s->sp[k]);
	free(s->sp);
}
/* pst::Tree::is_desc, spanning_tree.cpp:560-566: d is a PROPER descendant of a */
static int st_is_desc(const orc_tree *t, uint32_t a, uint32_t d)
{
	return t->pre[a] < t->pre[d] && t->post[a] > t->post[d];
}
/* find_lca of two vertices (the range minimum over the Euler tour of tree_utils.cpp:412-475 is the true LCA) */
static uint32_t sm_lca(const orc_tree *t, const sub_meta *s, uint32_t a, uint32_t b)
{
	if (a == b)
		return a;
	if (a > b) {
		uint32_t x = a;
		a = b;
		b = x;
	}
	if (st_is_desc(t, a, b))
		return a;
	/* shallowest vertex of (a, b] (the first one on ties): a child of the LCA.  Whole blocks through the table, the rest by hand */
	uint32_t lo = a + 1, hi = b + 1, c = lo; /* [lo, hi) */
	const uint32_t qb = (lo + SM_BLK - 1) / SM_BLK, qe = hi / SM_BLK; /* whole blocks [qb, qe) */
	if (qb < qe) {
		for (uint32_t v = lo; v < qb * SM_BLK; v++)
			if (s->depth[v] < s->depth[c])
				c = v;
		uint32_t k = 0;
		while ((2u << k) <= qe - qb)
			k++;
		const uint32_t x = s->sp[k][qb], y = s->sp[k][qe - (1u << k)];
		const uint32_t m = s->depth[y] < s->depth[x] ? y : x;
		if (s->depth[m] < s->depth[c])
			c = m;
		for (uint32_t v = qe * SM_BLK; v < hi; v++)
			if (s->depth[v] < s->depth[c])
				c = v;
	} else {
		for (uint32_t v = lo; v < hi; v++)
			if (s->depth[v] < s->depth[c])
				c = v;
	}
	return t->par[c];
}
#define BR_BEGIN(s, v) ((s)->m.off[v])
#define BR_END(s, v) ((s)->m.off[(v) + 1])
static uint32_t n_children(const sub_meta *s, uint32_t v) { return s->m.c_off[v + 1] - s->m.c_off[v]; }

/* ---- the PVST with its -s vertices (pvst.hpp:200-717) */
enum { CL_AI_TRUNK, CL_AI_BRANCH, CL_ZI_TRUNK, CL_ZI_BRANCH };
typedef struct {
	uint8_t fam;	  /* line letter: D F T O C S M */
	uint32_t id1, id2; /* as_str(): the two boundaries in print order */
	uint8_t or1, or2;
	char route;	  /* 'L' (s2e) 'R' (e2s), 0 = none */
	uint32_t ai, zi;  /* flubble-like */
	/* concealed (pvst.hpp:415-528) */
	uint32_t fl_idx, sl_st;
	uint8_t loc;
	uint32_t cnb_id;
	uint8_t cnb_or;
	uint32_t b_up, b_lo; /* bounds_t of a concealed / smothered vertex; g / s PVST idx of a midi bubble */
	uint32_t *ch, nch, cap;
	uint32_t dcap;	/* orc_sub_widths only: the capacity the device's vector has (seeded length, then doubling from 4) */
	uint8_t seeded; /* ... and whether it still is the seeded one */
} svtx;
typedef struct {
	svtx *v;
	uint32_t n, cap;
} spvst;

static uint32_t sp_add_vertex(spvst *p, const svtx *x)
{
	if (p->n == p->cap) {
		p->cap = p->cap ? 2 * p->cap : 64;
		p->v = realloc(p->v, (size_t)p->cap * sizeof *p->v);
		if (!p->v)
			abort();
	}
	p->v[p->n] = *x;
	p->v[p->n].ch = NULL;
	p->v[p->n].nch = p->v[p->n].cap = 0;
	p->v[p->n].dcap = 0;
	p->v[p->n].seeded = 0;
	return p->n++;
}
static void sp_add_edge_w(spvst *p, uint32_t parent, uint32_t child, int counted)
{
	svtx *v = &p->v[parent];
	if (counted)
		sw_max(SW_PUSH_LEN, v->nch);
	if (v->nch == v->dcap) { /* (the device's vector is full: it moves) */
		if (counted) {
			sw_max(v->fam == 'C' ? SW_PUSH_FULL_C : v->fam == 'S' ? SW_PUSH_FULL_S : SW_PUSH_FULL_F, v->nch);
			if (v->seeded)
				sw_max(SW_FIRST_PUSH_SEEDED, v->nch);
		}
		v->dcap = v->dcap ? 2 * v->dcap : 4;
	}
	v->seeded = 0;
	if (v->nch == v->cap) {
		v->cap = v->cap ? 2 * v->cap : 4;
		v->ch = realloc(v->ch, (size_t)v->cap * 4);
		if (!v->ch)
			abort();
	}
	v->ch[v->nch++] = child;
}
static void sp_add_edge(spvst *p, uint32_t parent, uint32_t child) { sp_add_edge_w(p, parent, child, 1); }
/* a nesting's mover goes under the new vertex: the device reserves room for a round's movers at once (sw_nesting counts it) */
static void sp_add_edge_moved(spvst *p, uint32_t parent, uint32_t child) { sp_add_edge_w(p, parent, child, 0); }
static void sp_del_edge(spvst *p, uint32_t parent, uint32_t child)
{
	svtx *v = &p->v[parent];
	for (uint32_t k = 0; k < v->nch; k++)
		if (v->ch[k] == child) {
			memmove(v->ch + k, v->ch + k + 1, (size_t)(v->nch - k - 1) * 4); /* (the last slot keeps its old value, as vector::erase leaves it) */
			v->nch--;
			return;
		}
}
static uint32_t *sp_children_copy(const spvst *p, uint32_t v, uint32_t *n)
{
	uint32_t *c = xmalloc(((size_t)p->v[v].nch + 1) * 4);
	memcpy(c, p->v[v].ch, (size_t)p->v[v].nch * 4);
	*n = p->v[v].nch;
	return c;
}
static int fl_like(uint8_t fam) { return fam == 'F' || fam == 'T' || fam == 'O'; }

/* id_or_t of a tree vertex: `fwd_is_r` = the orientation is forward when the vertex is of type r */
static void side_id_or(const orc_tree *t, uint32_t v, int fwd_is_r, uint32_t *id, uint8_t *orr)
{
	*id = t->gid[v];
	const int is_r = t->typ[v] == ORC_R;
	*orr = (uint8_t)((is_r == fwd_is_r) ? 0 : 1); /* 0 = forward '>', 1 = reverse '<' */
}

/* ---- find_concealed: the search (concealed.cpp:234-985) */
typedef struct {
	uint8_t loc;
	uint32_t sl_st, be_src;
} slub;
typedef struct {
	slub *x;
	uint32_t n, cap;
} slub_vec;
static void sv_push(slub_vec *v, uint8_t loc, uint32_t sl_st, uint32_t be_src)
{
	if (v->n == v->cap) {
		v->cap = v->cap ? 2 * v->cap : 4;
		v->x = realloc(v->x, (size_t)v->cap * sizeof *v->x);
		if (!v->x)
			abort();
	}
	v->x[v->n].loc = loc;
	v->x[v->n].sl_st = sl_st;
	v->x[v->n++].be_src = be_src;
}

/* compute_m, concealed.cpp:234-283 */
static uint32_t cn_compute_m(const orc_tree *t, const sub_meta *s, uint32_t ii, uint32_t ji)
{
	if (s->m.i_off[ii + 1] == s->m.i_off[ii])
		return ii;
	uint32_t best = NIL, best_h = 0;
	for (uint32_t b = s->m.i_off[ii]; b < s->m.i_off[ii + 1]; b++) {
		const uint32_t j = s->m.i_adj[b];
		if (t->be_type[j] != ORC_BE_BACK)
			continue;
		const uint32_t l = sm_lca(t, s, t->be_src[j], ji);
		if (s->depth[l] >= s->depth[ji])
			continue;
		if (s->depth[l] > best_h) {
			best = l;
			best_h = s->depth[l];
		}
	}
	return best == NIL ? ii : best;
}
/* compute_n, concealed.cpp:285-328 */
static uint32_t cn_compute_n(const orc_tree *t, const sub_meta *s, uint32_t ii, uint32_t ji)
{
	if (count_type(t, s->m.o_off, s->m.o_adj, ji, ORC_BE_BACK) == 0)
		return ji;
	uint32_t lowest = ii;
	for (uint32_t b = s->m.o_off[ji]; b < s->m.o_off[ji + 1]; b++) {
		const uint32_t j = s->m.o_adj[b];
		if (t->be_type[j] != ORC_BE_BACK)
			continue;
		if (s->depth[t->be_tgt[j]] > s->depth[lowest])
			lowest = t->be_tgt[j];
	}
	return lowest == ii ? ji : lowest;
}
/* can_contain, concealed.cpp:348-384 */
static int cn_can_contain(const orc_tree *t, const sub_meta *s, uint32_t ii, uint32_t ji, uint32_t m, uint32_t n)
{
	if (sm_depth(t, s, s->lo[ji]) < s->depth[ii]) /* (i) */
		return 0;
	uint32_t ibe_ii = 0;
	for (uint32_t b = s->m.i_off[ii]; b < s->m.i_off[ii + 1]; b++) {
		const uint32_t j = s->m.i_adj[b];
		ibe_ii += t->be_type[j] == ORC_BE_BACK && t->be_src[j] != ji;
	}
	if (m == ii && n == ji && ibe_ii < 2 && count_type(t, s->m.i_off, s->m.i_adj, ji, ORC_BE_BACK) == 0 && n_children(s, ji) < 3) /* (ii) */
		return 0;
	return 1;
}
/* ai_trunk, concealed.cpp:388-522: {be_src, lca} or NIL */
static int cn_ai_trunk(const orc_tree *t, const sub_meta *s, uint32_t m, uint32_t n, uint32_t ai, uint32_t zi, uint32_t *be_src_out,
		       uint32_t *lca_out)
{
	if (s->depth[m] > s->depth[n])
		return 0;
	uint32_t best_l = NIL, best_src = NIL;
	for (uint32_t b = s->m.i_off[ai]; b < s->m.i_off[ai + 1]; b++) {
		const uint32_t j = s->m.i_adj[b];
		if (t->be_type[j] != ORC_BE_BACK)
			continue;
		const uint32_t src = t->be_src[j], l = sm_lca(t, s, src, zi);
		if (s->depth[l] > s->depth[m]) /* cond i */
			continue;
		/* erased when !(all brackets of l end at ai or above) && (l has a back edge of its own or branches) */
		int ell_br = 1;
		for (uint64_t q = BR_BEGIN(s, l); q < BR_END(s, l) && ell_br; q++)
			ell_br = s->depth[t->be_tgt[s->m.be[q]]] <= s->depth[ai];
		const int cond_iii = s->m.o_off[l + 1] > s->m.o_off[l] || n_children(s, l) > 1;
		if (!ell_br && cond_iii)
			continue;
		/* sorted by lca ascending, the last one wins (a stable sort keeps the later of equals last) */
		if (best_l == NIL || l >= best_l) {
			best_l = l;
			best_src = src;
		}
	}
	if (best_l == NIL)
		return 0;
	*be_src_out = best_src;
	*lca_out = best_l;
	return 1;
}
/* LCA of the sources of the brackets of c (find_lca over br_srcs) */
static uint32_t lca_of_bracket_srcs(const orc_tree *t, const sub_meta *s, uint32_t c)
{
	uint32_t d = NIL;
	/* find_lca takes the extreme first-visit positions: the LCA of the set */
	for (uint64_t q = BR_BEGIN(s, c); q < BR_END(s, c); q++) {
		const uint32_t src = t->be_src[s->m.be[q]];
		d = d == NIL ? src : sm_lca(t, s, d, src);
	}
	return d;
}
/* ai_branches, concealed.cpp:525-583 (its else arm, :559-580, loops over an empty bracket list) */
static void cn_ai_branches(const orc_tree *t, const sub_meta *s, uint32_t ai, uint32_t zi, slub_vec *out)
{
	if (n_children(s, zi) < 2)
		return;
	for (uint32_t k = s->m.c_off[zi]; k < s->m.c_off[zi + 1]; k++) {
		const uint32_t c = s->m.c_adj[k];
		if (!(t->hi[c] == s->lo[c] && t->hi[c] == ai))
			continue;
		if (BR_END(s, c) - BR_BEGIN(s, c) < 2)
			continue;
		const uint32_t d = lca_of_bracket_srcs(t, s, c);
		if (BR_END(s, d) > BR_BEGIN(s, d))
			sv_push(out, CL_AI_BRANCH, d, NIL);
	}
}
/* override_ji_trunk, concealed.cpp:617-697 */
static uint32_t cn_override_ji_trunk(const orc_tree *t, const sub_meta *s, uint32_t m, uint32_t n, uint32_t ii, uint32_t ji)
{
	if (s->depth[m] > s->depth[n])
		return NIL;
	uint32_t min_v = n;
	for (uint32_t k = s->m.c_off[ji]; k < s->m.c_off[ji + 1]; k++) {
		const uint32_t c = s->m.c_adj[k];
		if (sm_depth(t, s, t->hi[c]) < s->depth[ii])
			continue; /* the child is j_x */
		if (BR_END(s, c) - BR_BEGIN(s, c) != 1)
			continue;
		const uint32_t y = t->be_tgt[s->m.be[BR_BEGIN(s, c)]];
		if (!(s->depth[m] < s->depth[y] && s->depth[n] > s->depth[y])) /* case (ii) (a) */
			continue;
		int valid = 1;
		for (uint64_t q = BR_BEGIN(s, y); q < BR_END(s, y) && valid; q++) {
			const uint32_t j = s->m.be[q];
			if (s->depth[t->be_src[j]] < s->depth[ji] || s->depth[t->be_tgt[j]] > s->depth[ii])
				valid = 0;
		}
		if (valid && s->depth[y] < s->depth[min_v])
			min_v = y;
	}
	if (min_v != n)
		SS_INC(SS_OVERRIDE_JI);
	return min_v == n ? NIL : min_v;
}
/* ji_trunk, concealed.cpp:699-788 (everything behind the return at :755-760 is dead) */
static uint32_t cn_ji_trunk(const orc_tree *t, const sub_meta *s, uint32_t m, uint32_t n, uint32_t ii, uint32_t ji)
{
	if (s->depth[m] > s->depth[n])
		return NIL;
	const uint32_t r = cn_override_ji_trunk(t, s, m, n, ii, ji);
	if (r != NIL)
		return r;
	/* the shallowest target of an ordinary back edge of ji that is not above n; the targets of one vertex lie on one
	 * root path, so equal depths are one vertex and std::sort's order among them does not show */
	uint32_t best = NIL;
	for (uint32_t b = s->m.o_off[ji]; b < s->m.o_off[ji + 1]; b++) {
		const uint32_t j = s->m.o_adj[b];
		if (t->be_type[j] != ORC_BE_BACK)
			continue;
		const uint32_t x = t->be_tgt[j];
		if (s->depth[x] < s->depth[n])
			continue;
		if (best == NIL || s->depth[x] < s->depth[best])
			best = x;
	}
	return best;
}
/* ji_branches, concealed.cpp:790-921 */
static void cn_ji_branches(const orc_tree *t, const sub_meta *s, uint32_t ii, uint32_t ji, uint32_t n, slub_vec *out)
{
	if (n_children(s, ji) < 2 || ji == n)
		return;
	int have_main = 0;
	for (uint32_t b = s->m.i_off[ii]; b < s->m.i_off[ii + 1] && !have_main; b++) {
		const uint32_t j = s->m.i_adj[b];
		have_main = t->be_type[j] == ORC_BE_BACK && t->be_src[j] == ji;
	}
	/* (iii) (a) for every child first, then (iii) (b): two vectors in the reference */
	for (int pass = 0; pass < 2; pass++) {
		for (uint32_t k = s->m.c_off[ji]; k < s->m.c_off[ji + 1]; k++) {
			const uint32_t c = s->m.c_adj[k];
			uint32_t count = 0;
			int into_ji = 0;
			for (uint64_t q = BR_BEGIN(s, c); q < BR_END(s, c); q++) {
				if (t->be_tgt[s->m.be[q]] != ji)
					count++;
				else
					into_ji = 1;
			}
			if (count != 1 || into_ji != (pass == 0))
				continue;
			if (pass == 0) { /* the deepest source of a bracket into ji */
				uint32_t lowest = c;
				for (uint64_t q = BR_BEGIN(s, c); q < BR_END(s, c); q++) {
					const uint32_t j = s->m.be[q];
					if (t->be_tgt[j] == ji && s->depth[t->be_src[j]] > s->depth[lowest])
						lowest = t->be_src[j];
				}
				sv_push(out, CL_ZI_BRANCH, lowest, NIL);
			} else { /* the only bracket of c */
				const uint32_t j = s->m.be[BR_BEGIN(s, c)];
				const uint32_t src = t->be_src[j], tgt = t->be_tgt[j];
				int cond_i = 0;
				uint32_t d = src;
				while (d != ji) {
					if (n_children(s, d) > 1) {
						cond_i = 1;
						break;
					}
					d = t->par[d];
				}
				const uint64_t alpha = BR_END(s, tgt) - BR_BEGIN(s, tgt);
				if (alpha != 0 && have_main)
					continue;
				if (alpha != 1)
					continue;
				if (cond_i)
					sv_push(out, CL_ZI_BRANCH, d, NIL);
			}
		}
	}
}

/* gen_ai_slubble, concealed.cpp:70-152 / gen_zi_slubble, :154-206 */
static void cn_make_vertex(const orc_tree *t, uint32_t ai, uint32_t zi, const slub *x, uint32_t fl_idx, svtx *out)
{
	memset(out, 0, sizeof *out);
	out->fam = 'C';
	out->fl_idx = fl_idx;
	out->loc = x->loc;
	out->sl_st = x->sl_st;
	const uint32_t sl = x->sl_st;
	const int sl_r = t->typ[sl] == ORC_R, black = t->pe_black[sl];
	uint32_t fl_id, sl_id = t->gid[sl];
	uint8_t fl_o, sl_o;
	if (x->loc == CL_AI_TRUNK || x->loc == CL_AI_BRANCH) {
		side_id_or(t, ai, 1, &fl_id, &fl_o);
		/* trunk: parent edge black -> forward iff r; branch: the other way round */
		const int fwd_if_r = (x->loc == CL_AI_TRUNK) == (black != 0);
		sl_o = (uint8_t)((sl_r == fwd_if_r) ? 0 : 1);
		uint32_t a_id = fl_id, g_id = sl_id;
		uint8_t a_o = fl_o, g_o = sl_o;
		if (sl_o == 1 && fl_o == 1) { /* both reverse: swapped and flipped */
			a_id = sl_id, a_o = 0;
			g_id = fl_id, g_o = 0;
		}
		out->id1 = a_id, out->or1 = a_o; /* as_str: fl_b then cn_b */
		out->id2 = g_id, out->or2 = g_o;
		out->cnb_id = g_id, out->cnb_or = g_o;
		out->route = 'R'; /* e2s */
		if (x->loc == CL_AI_TRUNK) {
			if (st_is_desc(t, ai, x->be_src))
				out->b_up = ai, out->b_lo = x->be_src;
			else
				out->b_up = x->be_src, out->b_lo = ai;
		} else {
			out->b_up = sl, out->b_lo = NIL;
		}
	} else {
		side_id_or(t, zi, 0, &fl_id, &fl_o); /* forward iff l */
		sl_o = (uint8_t)((sl_r == (black != 0)) ? 0 : 1);
		uint32_t s_id = sl_id, z_id = fl_id;
		uint8_t s_o = sl_o, z_o = fl_o;
		if (sl_o == 1 && fl_o == 1) {
			s_id = sl_id, s_o = 0;
			z_id = fl_id, z_o = 0;
		}
		out->id1 = s_id, out->or1 = s_o; /* as_str: cn_b then fl_b */
		out->id2 = z_id, out->or2 = z_o;
		out->cnb_id = s_id, out->cnb_or = s_o;
		out->route = 'L'; /* s2e */
		if (st_is_desc(t, zi, sl))
			out->b_up = zi, out->b_lo = sl;
		else
			out->b_up = sl, out->b_lo = zi;
	}
}

typedef struct {
	uint32_t fl, m, n, first, n_ai, n_zi; /* its slubbles: all[first ..), the n_ai "in relation to a" first */
} fl_sls;

/* find_concealed, concealed.cpp:1198-1243 with update_pvst::add_concealed, :925-1196 */
static void sub_find_concealed(const orc_tree *t, const sub_meta *s, spvst *p)
{
	slub_vec all = {0};
	fl_sls *fls = NULL;
	uint32_t nf = 0, capf = 0;
	const uint32_t n0 = p->n;
	for (uint32_t f = 0; f < n0; f++) {
		if (p->v[f].fam != 'F')
			continue;
		const uint32_t ai = p->v[f].ai, zi = p->v[f].zi;
		const uint32_t m = cn_compute_m(t, s, ai, zi), n = cn_compute_n(t, s, ai, zi);
		if (!cn_can_contain(t, s, ai, zi, m, n))
			continue;
		const uint32_t first = all.n;
		uint32_t be_src, l;
		if (cn_ai_trunk(t, s, m, n, ai, zi, &be_src, &l))
			sv_push(&all, CL_AI_TRUNK, l, be_src);
		cn_ai_branches(t, s, ai, zi, &all);
		const uint32_t n_ai = all.n - first;
		const uint32_t tb = cn_ji_trunk(t, s, m, n, ai, zi);
		if (tb != NIL)
			sv_push(&all, CL_ZI_TRUNK, tb, NIL);
		cn_ji_branches(t, s, ai, zi, n, &all);
		if (all.n == first)
			continue;
		if (nf == capf) {
			capf = capf ? 2 * capf : 16;
			fls = realloc(fls, (size_t)capf * sizeof *fls);
			if (!fls)
				abort();
		}
		fls[nf++] = (fl_sls){f, m, n, first, n_ai, all.n - first - n_ai};
	}
	uint8_t *listed = xcalloc((size_t)n0 + 1, 1); /* (orc_sub_widths: has records or takes a pinned vertex in) */
	for (uint32_t q = 0; q < nf; q++)
		listed[fls[q].fl] = 1;
	SW_ADD(SW_CN_LIST, nf);
	SW_ADD(SW_N_CONCEALED, all.n);
	for (uint32_t q = 0; q < nf; q++) {
		const fl_sls *F = &fls[q];
		const uint32_t f = F->fl, ai = p->v[f].ai, zi = p->v[f].zi;
		sw_max(SW_CN_PER_FLUBBLE, F->n_ai + F->n_zi);
		const int is_leaf = f < t->n && n_children(s, f) == 0; /* (sic) the SPANNING TREE's vertex f, concealed.cpp:1188 */
		const uint32_t own0 = p->n; /* f's own concealed vertices from here on: one in [n0, own0) was pushed by its parent */
		for (uint32_t k = 0; k < F->n_ai + F->n_zi; k++) {
			const slub *x = &all.x[F->first + k];
			svtx nv;
			cn_make_vertex(t, ai, zi, x, f, &nv);
			SS_INC(SS_AI_TRUNK + x->loc);
			if (is_leaf)
				SS_INC(SS_LEAF_BY_TREE_IDX);
			else if (x->loc == CL_ZI_BRANCH)
				SS_INC(SS_ZI_BRANCH_UNNESTED);
			const uint32_t sl_v = sp_add_vertex(p, &nv);
			sp_add_edge(p, f, sl_v);
			if (is_leaf)
				continue;
			uint32_t nch;
			uint32_t *ch = sp_children_copy(p, f, &nch);
			if (x->loc != CL_ZI_BRANCH) /* the nestings run over the concealed vertex of the parent's z-side trunk record */
				for (uint32_t c_k = 0; c_k < nch; c_k++)
					if (ch[c_k] >= n0 && ch[c_k] < own0) {
						SS_INC(SS_NEST_OVER_PINNED);
						sw_max(SW_PINNED_LEN, nch);
						SW_ADD(SW_PINNED_WIDE, nch >= 64);
						break;
					}
			uint8_t *moved = xcalloc((size_t)nch + 1, 1);
			for (uint32_t c_k = 0; c_k < nch; c_k++) {
				const uint32_t c = ch[c_k];
				if (!fl_like(p->v[c].fam))
					continue;
				const uint32_t c_ai = p->v[c].ai, c_zi = p->v[c].zi;
				if (x->loc == CL_AI_TRUNK) { /* nest_trunk_ai, :945-979 */
					if (s->depth[x->sl_st] > s->depth[c_zi] || st_is_desc(t, x->sl_st, c_ai)) {
						SS_INC(SS_NEST_TRUNK_AI);
						moved[c_k] = 1;
						sp_del_edge(p, f, c);
						sp_add_edge_moved(p, sl_v, c);
					}
				} else if (x->loc == CL_AI_BRANCH && k < F->n_ai) { /* nest_branch_ai, :984-1034 */
					int has_br = 0; /* a bracket of c's zi that STARTS at ai (sic: get_src, :1006) */
					for (uint64_t b = BR_BEGIN(s, c_zi); b < BR_END(s, c_zi) && !has_br; b++)
						has_br = t->be_src[s->m.be[b]] == ai;
					if (st_is_desc(t, x->sl_st, c_ai) && has_br) {
						SS_INC(SS_NEST_BRANCH_AI);
						moved[c_k] = 1;
						sp_del_edge(p, f, c);
						sp_add_edge_moved(p, sl_v, c);
					}
				} else if (x->loc == CL_ZI_TRUNK) { /* nest_trunk_zi, :1054-1081: (sic) the edge goes from the child to the slubble */
					if (st_is_desc(t, F->n, c_ai) && !st_is_desc(t, zi, c_zi)) {
						SS_INC(SS_NEST_TRUNK_ZI);
						moved[c_k] = 1;
						if (c < n0 && !listed[c]) {
							listed[c] = 1;
							SW_ADD(SW_CN_LIST, 1);
						}
						sp_del_edge(p, f, c);
						sp_add_edge(p, c, sl_v);
					}
				}
				/* zi_branch: add_conc_zi asks for ai_branch (:1134) and ends in "sl type: unknown" */
			}
			if (x->loc != CL_ZI_BRANCH)
				sw_nesting(x->loc == CL_AI_TRUNK ? NK_AI_TRUNK : x->loc == CL_AI_BRANCH ? NK_AI_BRANCH : NK_ZI_TRUNK, moved, nch);
			free(moved);
			free(ch);
		}
	}
	free(listed);
	free(all.x);
	free(fls);
}

/* find_midi, midi.cpp:225-268 (handle_fl :142-223, gen_midi_bub :63-139, add_midi :19-61) */
static void sub_find_midi(const orc_tree *t, const sub_meta *s, spvst *p)
{
	typedef struct {
		uint32_t fl, g_idx, s_idx;
	} midi;
	midi *ms = NULL;
	uint32_t nm = 0, capm = 0;
	const uint32_t n0 = p->n;
	for (uint32_t f = 0; f < n0; f++) {
		if (p->v[f].fam != 'F')
			continue;
		uint32_t n_cn = 0, trunk[2] = {NIL, NIL}, n_trunk = 0, at[2] = {0, 0};
		int third_later = 0;
		const uint32_t zi = p->v[f].zi;
		for (uint32_t k = 0; k < p->v[f].nch; k++) {
			const uint32_t c = p->v[f].ch[k];
			if (p->v[c].fam != 'C')
				continue;
			n_cn++;
			if (p->v[c].sl_st < zi) { /* in_trunk, :163-166 */
				if (n_trunk < 2)
					trunk[n_trunk] = c, at[n_trunk] = k;
				else if (k / 64 > at[1] / 64)
					third_later = 1;
				n_trunk++;
			}
			/* else: the branch case -- undefined in the reference, nothing here (see the header) */
		}
		if (n_cn) { /* (the device looks at the flubbles that got a concealed child) */
			sw_max(SW_MIDI_FIND_LEN, p->v[f].nch);
			sw_max(SW_MIDI_NTRUNK, n_trunk);
			if (n_trunk >= 1)
				sw_max(SW_MIDI_FIRST_IDX, (uint64_t)at[0] + 1);
			if (n_trunk >= 2) {
				sw_max(SW_MIDI_SECOND_IDX, (uint64_t)at[1] + 1);
				SW_ADD(SW_MIDI_SPLIT_ROUNDS, at[0] / 64 != at[1] / 64);
			}
			SW_ADD(SW_MIDI_THIRD_LATER, third_later);
		}
		if (n_cn < 2 || n_trunk != 2)
			continue;
		/* gen_midi_bub: the later of two g's (or s's) overrides the earlier; one of each is needed */
		uint32_t g_idx = NIL, s_idx = NIL;
		for (int k = 0; k < 2; k++) {
			if (p->v[trunk[k]].loc == CL_AI_BRANCH || p->v[trunk[k]].loc == CL_AI_TRUNK)
				g_idx = trunk[k];
			else
				s_idx = trunk[k];
		}
		if (g_idx == NIL || s_idx == NIL) {
			SS_INC(SS_MIDI_SAME_KIND);
			continue; /* (throws, is caught and logged) */
		}
		SS_INC(SS_MIDI);
		if (nm == capm) {
			capm = capm ? 2 * capm : 16;
			ms = realloc(ms, (size_t)capm * sizeof *ms);
			if (!ms)
				abort();
		}
		ms[nm++] = (midi){f, g_idx, s_idx};
	}
	for (uint32_t q = 0; q < nm; q++) {
		const uint32_t f = ms[q].fl;
		uint32_t nch;
		uint32_t *ch = sp_children_copy(p, f, &nch);
		const uint32_t up = ms[q].g_idx < ms[q].s_idx ? ms[q].g_idx : ms[q].s_idx;
		const uint32_t lo = ms[q].g_idx < ms[q].s_idx ? ms[q].s_idx : ms[q].g_idx;
		svtx nv;
		memset(&nv, 0, sizeof nv);
		nv.fam = 'M';
		nv.id1 = p->v[ms[q].g_idx].cnb_id, nv.or1 = p->v[ms[q].g_idx].cnb_or;
		nv.id2 = p->v[ms[q].s_idx].cnb_id, nv.or2 = p->v[ms[q].s_idx].cnb_or;
		nv.route = 'L';
		nv.b_up = up, nv.b_lo = lo;
		const uint32_t mv = sp_add_vertex(p, &nv);
		sp_add_edge(p, f, mv);
		uint8_t *moved = xcalloc((size_t)nch + 1, 1);
		for (uint32_t k = 0; k < nch; k++) {
			const uint32_t c = ch[k];
			if (p->v[c].fam != 'F')
				continue;
			/* (sic) spanning-tree depths at the PVST indices of the two concealed vertices */
			if (sm_depth(t, s, up) < s->depth[p->v[c].ai] && sm_depth(t, s, lo) > s->depth[p->v[c].zi]) {
				SS_INC(SS_MIDI_NEST);
				moved[k] = 1;
				sp_del_edge(p, f, c);
				sp_add_edge_moved(p, mv, c);
			}
		}
		sw_nesting(NK_MIDI, moved, nch);
		free(moved);
		free(ch);
	}
	free(ms);
}

/* find_smothered, smothered.cpp:385-432 */
typedef struct {
	uint32_t cn;
	svtx v;
} smo_rec;
typedef struct {
	smo_rec *x;
	uint32_t n, cap;
} smo_vec;
static void smo_push(smo_vec *v, const orc_tree *t, uint32_t cn_idx, const svtx *cn, uint32_t sm_st, int cn_is_anc, int is_g, uint32_t b_up,
		     uint32_t b_lo)
{
	if (v->n == v->cap) {
		v->cap = v->cap ? 2 * v->cap : 16;
		v->x = realloc(v->x, (size_t)v->cap * sizeof *v->x);
		if (!v->x)
			abort();
	}
	smo_rec *r = &v->x[v->n++];
	memset(r, 0, sizeof *r);
	r->cn = cn_idx;
	r->v.fam = 'S';
	const uint32_t sm_id = t->gid[sm_st];
	const uint8_t sm_or = (uint8_t)(t->typ[sm_st] == ORC_L ? 1 : 0); /* comp_e / comp_w: type l -> reverse, else forward */
	/* Smothered::as_str, pvst.hpp:612-636 */
	if (is_g && cn_is_anc) {
		r->v.id1 = cn->cnb_id, r->v.or1 = cn->cnb_or;
		r->v.id2 = sm_id, r->v.or2 = sm_or;
	} else {
		r->v.id1 = sm_id, r->v.or1 = sm_or;
		r->v.id2 = cn->cnb_id, r->v.or2 = cn->cnb_or;
	}
	r->v.route = is_g ? 'L' : 'R';
	r->v.b_up = b_up, r->v.b_lo = b_lo;
}
/* compute_bounds, smothered.cpp:37-48 */
static void smo_bounds(const orc_tree *t, uint32_t cn_st, uint32_t sm_st, uint32_t *up, uint32_t *lo)
{
	if (st_is_desc(t, cn_st, sm_st))
		*up = cn_st, *lo = sm_st;
	else
		*up = sm_st, *lo = cn_st;
}
/* distinct values of key[] over a CSR row, ascending (std::set) */
static uint32_t sorted_distinct(const uint32_t *off, const uint32_t *adj, const uint32_t *key, uint32_t v, uint32_t **out)
{
	const uint32_t n = off[v + 1] - off[v];
	uint32_t *x = xmalloc(((size_t)n + 1) * 4), k = 0;
	for (uint32_t b = off[v]; b < off[v + 1]; b++)
		x[k++] = key[adj[b]];
	for (uint32_t a = 1; a < k; a++) { /* insertion sort: the rows are short */
		uint32_t y = x[a], b = a;
		while (b && x[b - 1] > y) {
			x[b] = x[b - 1];
			b--;
		}
		x[b] = y;
	}
	uint32_t u = 0;
	for (uint32_t a = 0; a < k; a++)
		if (!u || x[u - 1] != x[a])
			x[u++] = x[a];
	*out = x;
	return u;
}
static void sub_find_smothered(const orc_tree *t, const sub_meta *s, spvst *p)
{
	smo_vec all = {0};
	const uint32_t n0 = p->n;
	for (uint32_t cv = 0; cv < n0; cv++) {
		if (p->v[cv].fam != 'C')
			continue;
		const svtx *cn = &p->v[cv];
		const uint32_t fl = cn->fl_idx, ai = p->v[fl].ai, zi = p->v[fl].zi, sl = cn->sl_st;
		switch (cn->loc) {
		case CL_AI_TRUNK: /* g::trunk, smothered.cpp:61-134 */
			for (uint32_t k = s->m.c_off[sl]; k < s->m.c_off[sl + 1]; k++) {
				const uint32_t c = s->m.c_adj[k];
				if (BR_END(s, c) == BR_BEGIN(s, c))
					continue;
				const uint32_t last = s->m.be[BR_END(s, c) - 1], src = t->be_src[last], tgt = t->be_tgt[last];
				int one_src = 1;
				for (uint64_t q = BR_BEGIN(s, c); q < BR_END(s, c) && one_src; q++)
					one_src = t->be_src[s->m.be[q]] == src;
				const uint32_t brch = sm_lca(t, s, zi, src);
				if (!(one_src && s->depth[tgt] > s->depth[ai]))
					continue;
				if (BR_END(s, src) == BR_BEGIN(s, src)) {
					SS_INC(SS_SMO_G_TRUNK_TGT);
					smo_push(&all, t, cv, cn, tgt, 0, 1, brch, src);
				} else {
					SS_INC(SS_SMO_G_TRUNK_SRC);
					smo_push(&all, t, cv, cn, src, 1, 1, brch, src);
				}
			}
			break;
		case CL_AI_BRANCH: { /* g::branch, :136-199 */
			uint32_t *tg, nt = sorted_distinct(s->m.o_off, s->m.o_adj, t->be_tgt, sl, &tg);
			const int go = nt == 1 && tg[0] == ai;
			free(tg);
			if (!go)
				break;
			for (uint64_t q = BR_BEGIN(s, sl); q < BR_END(s, sl); q++) {
				const uint32_t j = s->m.be[q];
				if (t->be_tgt[j] != ai)
					continue;
				const uint32_t src = t->be_src[j];
				for (uint64_t r = BR_BEGIN(s, src); r < BR_END(s, src); r++)
					if (t->be_tgt[s->m.be[r]] == sl) {
						uint32_t up, lo;
						smo_bounds(t, sl, src, &up, &lo);
						SS_INC(SS_SMO_G_BRANCH);
						smo_push(&all, t, cv, cn, src, 1, 1, up, lo);
					}
			}
			break;
		}
		case CL_ZI_TRUNK: { /* s::trunk, :217-270: sources grouped by their LCA with zi, ascending */
			uint32_t *srcs, ns = sorted_distinct(s->m.i_off, s->m.i_adj, t->be_src, sl, &srcs);
			uint32_t *lc = xmalloc(((size_t)ns + 1) * 4), nk = 0, *kept = xmalloc(((size_t)ns + 1) * 4);
			for (uint32_t a = 0; a < ns; a++) {
				const uint32_t src = srcs[a];
				if (s->depth[src] >= s->depth[zi])
					continue;
				const uint32_t l = sm_lca(t, s, zi, src);
				if (l == src)
					continue;
				lc[nk] = l, kept[nk++] = src;
			}
			for (;;) { /* the map's keys in ascending order */
				uint32_t best = NIL;
				for (uint32_t a = 0; a < nk; a++)
					if (lc[a] != NIL && (best == NIL || lc[a] < best))
						best = lc[a];
				if (best == NIL)
					break;
				uint32_t cnt = 0, only = NIL;
				for (uint32_t a = 0; a < nk; a++)
					if (lc[a] == best) {
						cnt++;
						only = kept[a];
						lc[a] = NIL;
					}
				if (cnt == 1) {
					SS_INC(SS_SMO_S_TRUNK);
					smo_push(&all, t, cv, cn, only, 0, 0, best, only);
				}
			}
			free(srcs);
			free(lc);
			free(kept);
			break;
		}
		case CL_ZI_BRANCH: { /* s::branch, :272-318 */
			uint32_t *srcs, ns = sorted_distinct(s->m.i_off, s->m.i_adj, t->be_src, sl, &srcs);
			for (uint32_t a = 0; a < ns; a++) {
				const uint32_t src = srcs[a];
				uint32_t *x, nx = sorted_distinct(s->m.i_off, s->m.i_adj, t->be_src, src, &x);
				for (uint32_t b = 0; b < nx; b++) {
					uint32_t up, lo;
					smo_bounds(t, x[b], sl, &up, &lo);
					SS_INC(SS_SMO_S_BRANCH_SRC);
					smo_push(&all, t, cv, cn, x[b], 1, 0, up, lo);
				}
				free(x);
				nx = sorted_distinct(s->m.o_off, s->m.o_adj, t->be_tgt, src, &x);
				for (uint32_t b = 0; b < nx; b++) {
					if (x[b] == zi)
						continue;
					uint32_t up, lo;
					smo_bounds(t, x[b], sl, &up, &lo);
					SS_INC(SS_SMO_S_BRANCH_TGT);
					smo_push(&all, t, cv, cn, x[b], 0, 0, up, lo);
				}
				free(x);
			}
			free(srcs);
			break;
		}
		}
	}
	/* add_smothered, :349-383: the records are already grouped by concealed vertex, ascending */
	for (uint32_t q = 0, run = 0; q < all.n; q++) {
		const uint32_t cv = all.x[q].cn;
		run = q && all.x[q - 1].cn == cv ? run + 1 : 1;
		sw_max(SW_SMO_PER_CN, run);
		SW_ADD(SW_N_SMO_CN, run == 1);
		uint32_t n_erased = 0, n_stale = 0;
		const uint32_t sv = sp_add_vertex(p, &all.x[q].v);
		sp_add_edge(p, cv, sv);
		/* nest, :332-347: a range-for over children_v[cv] while del_edge erases from it -- as libstdc++ runs it */
		const uint32_t up = p->v[sv].b_up, lo = p->v[sv].b_lo;
		const uint32_t old_end = p->v[cv].nch;
		for (uint32_t k = 0; k < old_end; k++) {
			const uint32_t c = p->v[cv].ch[k]; /* (slots behind the live end hold what erase left there) */
			if (k >= p->v[cv].nch) {
				SS_INC(SS_SMO_STALE_READ);
				n_stale++;
			}
			uint32_t c_up, c_lo;
			if (fl_like(p->v[c].fam))
				c_up = p->v[c].ai, c_lo = p->v[c].zi;
			else if (p->v[c].fam == 'C')
				c_up = p->v[c].b_up, c_lo = p->v[c].b_lo;
			else
				continue;
			if (c_up >= t->n || c_lo >= t->n)
				continue; /* (a concealed child with an open bound never occurs: concealed vertices have no concealed children) */
			if (st_is_desc(t, up, c_up) && st_is_desc(t, c_lo, lo)) {
				SS_INC(SS_SMO_NEST);
				n_erased++;
				sp_del_edge(p, cv, c);
				sp_add_edge(p, sv, c);
			}
		}
		sw_max(SW_SMO_OLD_END, old_end);
		sw_max(SW_SMO_ERASURES, n_erased);
		sw_max(SW_SMO_STALE, n_stale);
	}
	free(all.x);
}

/* decompose_component with -s (decompose.cpp:63-70): the five passes in order, then write_pvst (to_pvst.cpp:31-109) */
char *orc_subflubbles_text(const orc_tree *t, orc_pvst *pv, size_t *len)
{
	orc_leaf_subflubbles(t, pv);
	sub_meta s;
	sub_meta_build(t, &s);
	spvst p = {0};
	for (uint32_t v = 0; v < pv->n; v++) {
		svtx x;
		memset(&x, 0, sizeof x);
		x.fam = pv->fam[v];
		if (v) {
			x.id1 = pv->a_id[v], x.or1 = pv->a_or[v];
			x.id2 = pv->z_id[v], x.or2 = pv->z_or[v];
			x.route = 'L';
			x.ai = pv->ai[v], x.zi = pv->zi[v];
		}
		sp_add_vertex(&p, &x);
	}
	for (uint32_t v = 1; v < pv->n; v++)
		sp_add_edge_w(&p, pv->parent[v], v, 0);
	for (uint32_t v = 0; v < p.n; v++) /* (orc_sub_widths: the device seeds every vector full) */
		p.v[v].dcap = p.v[v].nch, p.v[v].seeded = 1;
	sub_find_concealed(t, &s, &p);
	sub_find_midi(t, &s, &p);
	sub_find_smothered(t, &s, &p);
	sbuf b = {0};
	sb_str(&b, "H\t0.0.3\t.\t.\t.\n");
	for (uint32_t i = 0; i < p.n; i++) {
		const svtx *v = &p.v[i];
		char l[3] = {(char)v->fam, '\t', 0};
		sb_str(&b, l);
		sb_u32(&b, i);
		sb_str(&b, "\t");
		if (v->fam == 'D') {
			sb_str(&b, ".");
		} else {
			sb_str(&b, v->or1 ? "<" : ">");
			sb_u32(&b, v->id1);
			sb_str(&b, v->or2 ? "<" : ">");
			sb_u32(&b, v->id2);
		}
		sb_str(&b, "\t");
		if (v->nch == 0) {
			sb_str(&b, ".");
		} else {
			for (uint32_t k = 0; k < v->nch; k++) {
				sb_u32(&b, v->ch[k]);
				if (k + 1 < v->nch)
					sb_str(&b, ", ");
			}
		}
		if (v->route) {
			char r[4] = {'\t', v->route, '\n', 0};
			sb_str(&b, r);
		} else {
			sb_str(&b, "\t.\n");
		}
	}
	for (uint32_t i = 0; i < p.n; i++)
		free(p.v[i].ch);
	free(p.v);
	sub_meta_free(&s);
	sb_need(&b, 1);
	b.b[b.n] = 0;
	*len = b.n;
	return b.b;
}
