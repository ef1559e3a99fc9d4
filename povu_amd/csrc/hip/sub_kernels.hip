// sub_kernels.hip -- the three INSERTING passes of `povu decompose -s` on the state of an all-parallel pass:
// find_concealed (src/povu/algorithms/concealed.cpp:1198-1243), find_midi (midi.cpp:225-268) and find_smothered
// (smothered.cpp:385-432), after find_tiny / find_parallel (leaf_kernels.hip) have relabelled the leaves.
//
// The reference walks every flubble of a PVST and asks its spanning tree and gen_tree_meta (src/povu/graph/
// tree_utils.cpp:674-688: depths, LoA, LCA, the per-vertex bracket table) a few dozen questions; what it finds it then
// splices into the PVST one vertex after the other.  Here:
//   tables    depth (the tree stage writes it), literal hi (flubbles.cpp:552,640: a simplifying edge resets it to the root,
//             which every ancestor then inherits), back edges by source and by target (all three types); the BRACKETS of a
//             vertex (count_brackets / collect_backedges_by_vertex, tree_utils.cpp:167-216, 531-574) are not materialised
//             as the reference's table is (one entry per back edge and vertex it spans: 10^10 on a graph with large
//             tangles) but enumerated where a row is asked for, through a segment tree over the targets of the edges in
//             source order; where the reference's row ORDER shows (back-edge idx = creation order in from_bd) the
//             "creation key" below decides; LoA (tree_utils.cpp:224-273) in closed form from a max-tree over the edges'
//             intervals -- by the reference's own heap, one lane per component, only where a self-loop back edge (the
//             root of a tip-less component has one) leaves stale entries in it (oracle/povu_oracle_sub.inc) --, LCA =
//             parent of the shallowest vertex of an index range (a segment tree over the depths: vertex idx = pre-order
//             rank);
//   search    one lane per flubble (concealed.cpp:234-921) and one per concealed vertex (smothered.cpp:61-318), each run
//             twice -- count, scan, emit;
//   splice    add_concealed, find_midi / add_midi and add_smothered change the children vectors of the PVST in an order
//             that shows in the output (vector::push_back / erase, pvst.hpp:860-885) and reach across families (a
//             concealed vertex is appended to the children of a CHILD flubble, concealed.cpp:1077): they run literally,
//             one WAVE per component, over vectors in a bump arena; the loops over a flubble's children are shared out
//             over the lanes.
// Accidents of the reference that are kept and behaviour it leaves undefined are those listed at the top of
// oracle/povu_oracle_sub.inc, decided the same way here.  PARITY UNPINNED: the reference holds no C / M / S line; the
// tests compare with the oracle's sequential restatement.
//
// Creation key of an ordinary back edge (the reference's rows are in back-edge idx order = the order from_bd created
// them): an edge of source u is created while u's adjacency is scanned -- between the discoveries of two of its children,
// or behind the last.  tn = the next vertex discovered after it (the child, or the vertex behind u's subtree); edges with
// the same tn were created while the recursion unwound towards parent(tn): deeper sources first, then in the source's own
// scan order (b_ord).  So (tn ascending, source descending, b_ord ascending) is the idx order.
#include "sub_kernels.hpp"

#include "context.hpp"

#include "segtree.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace povu_hip
{

#ifndef NIL
#define NIL POVU_NIL
#endif

namespace
{
enum : uint32_t { CL_AI_TRUNK = 0, CL_AI_BRANCH = 1, CL_ZI_TRUNK = 2, CL_ZI_BRANCH = 3 };
enum : uint32_t { E_POOL = 2u, E_LAYOUT = 8u };

// device view of the spanning forest (T-space: global tree vertex idx) and of the dense PVST output
struct SubT {
	uint32_t T, C, NB0, NB;
	const uint32_t *voff, *c_ntree, *doff, *c_npvst;
	const uint32_t *size, *gp, *nchild, *depth, *gid;
	const uint8_t *flags;
	const uint32_t *b_src, *b_tgt, *b_ord;
	const uint32_t *o_off, *o_adj, *i_off, *i_adj; // back edges of all types by source / by target (edge = slot of the dense list)
	const uint32_t *br_cnt;	       // |brackets(v)|
	const uint32_t *O, *slot_s;	       // the ordinary edges in source order: position O[u] + r = the r-th edge of u, its slot in the dense list
	SegTree segT;			       // over the targets of the edges in source order
	const uint32_t *lo, *hi;
	const unsigned long long *ekey; // [NB0] creation key: tn << 32 | ~source
	SegTree segD;
	const uint32_t *p_ai, *p_zi, *p_parent, *p_a, *p_z;
	const uint8_t *p_fam, *p_aor, *p_zor;
	uint32_t *err;
	__device__ __forceinline__ uint32_t base_of(uint32_t c) const { return 2 * voff[c] + c; }
	__device__ __forceinline__ bool ordinary(uint32_t j) const { return j < NB0; }
	__device__ __forceinline__ uint32_t dep(uint32_t v) const { return (v < T && size[v]) ? depth[v] : 0xFFFFFFFFu; }
	// pst::Tree::is_desc, spanning_tree.cpp:560-566: d is a proper descendant of a
	__device__ __forceinline__ bool is_desc(uint32_t a, uint32_t d) const { return a < d && d < a + size[a]; }
	__device__ __forceinline__ uint32_t n_br(uint32_t v) const { return br_cnt[v]; }
	// The brackets of v (tm.get_brackets, tree_utils.hpp:64-77): the ordinary edges whose source lies strictly below v and
	// whose target lies above it = among the edges of the sources (v, v + size) those with a target idx below v, found one
	// after the other in the segment tree over the targets.  The reference MATERIALISES the table, one entry per edge and
	// vertex it spans -- 10^10 entries on a graph with large tangles; here a row is enumerated when it is asked for, in
	// source order (what needs the reference's back-edge idx order asks created_before).  The root has none.
	struct BrRange {
		uint32_t pos, hi, v;
	};
	__device__ __forceinline__ BrRange brackets(uint32_t v) const
	{
		if (v >= T || !size[v] || gp[v] == NIL)
			return BrRange{0u, 0u, v};
		return BrRange{O[v + 1], O[v + size[v]], v};
	}
	__device__ __forceinline__ uint32_t br_next(BrRange &r) const // next bracket (slot of the dense list), NIL at the end
	{
		if (r.pos >= r.hi)
			return NIL;
		const uint32_t p = seg_first_less(segT, r.pos, r.hi, r.v);
		if (p == NIL) {
			r.pos = r.hi;
			return NIL;
		}
		r.pos = p + 1;
		return slot_s[p];
	}
	__device__ uint32_t lca(uint32_t a, uint32_t b) const
	{
		if (a == b)
			return a;
		if (a > b) {
			const uint32_t x = a;
			a = b;
			b = x;
		}
		if (is_desc(a, b))
			return a;
		const uint32_t m = seg_min(segD, a + 1, b + 1);
		const uint32_t c = seg_first_less(segD, a + 1, b + 1, m + 1);
		return gp[c];
	}
	__device__ uint32_t count_ord(const uint32_t *off, const uint32_t *adj, uint32_t v) const
	{
		uint32_t k = 0;
		for (uint32_t b = off[v]; b < off[v + 1]; b++)
			k += ordinary(adj[b]) ? 1u : 0u;
		return k;
	}
	// creation order of two ordinary back edges
	__device__ __forceinline__ bool created_before(uint32_t j1, uint32_t j2) const
	{
		const unsigned long long k1 = ekey[j1], k2 = ekey[j2];
		return k1 != k2 ? k1 < k2 : b_ord[j1] < b_ord[j2];
	}
};
struct CompAt { // component of a global tree vertex / of a dense PVST slot
	const uint32_t *voff, *doff;
	uint32_t C;
	__device__ __forceinline__ uint32_t of_tree(uint32_t t) const { return CompSpans{voff, C}.of_tree(t); }
	// last c with doff[c] <= q (components without a PVST own no slot)
	__device__ __forceinline__ uint32_t of_slot(uint32_t q) const { return span_of(doff, C, q); }
};

// ------------------------------------------------------------------ tables
__global__ void k_sub_depth_hi0(uint32_t T, const uint32_t *__restrict__ t_size, const uint32_t *__restrict__ t_depth,
				uint32_t *__restrict__ depth, uint32_t *__restrict__ hi0, uint32_t *__restrict__ eat)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t > T)
		return;
	depth[t] = (t < T && t_size[t]) ? t_depth[t] : 0xFFFFFFFFu;
	hi0[t] = NIL;
	eat[t] = NIL;
}
// by-source and by-target counts of all back edges; hi_0 of every vertex (ordinary edges only: the others do not exist yet
// when handle_vertex reads OBE, flubbles.cpp:515-519); first slot of every source's ordinary edges in the dense list
__global__ void k_sub_edge_counts(uint32_t NB, uint32_t NB0, const uint32_t *__restrict__ b_src, const uint32_t *__restrict__ b_tgt,
				  const uint32_t *__restrict__ b_ord, uint32_t *__restrict__ ocnt, uint32_t *__restrict__ icnt,
				  uint32_t *__restrict__ hi0, uint32_t *__restrict__ eat)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= NB)
		return;
	const uint32_t u = b_src[j], w = b_tgt[j];
	atomicAdd(&ocnt[u], 1u);
	atomicAdd(&icnt[w], 1u);
	if (j < NB0) {
		atomicMin(&hi0[u], w);
		if (b_ord[j] == 0)
			eat[u] = j;
	}
}
__global__ void k_sub_edge_fill(uint32_t NB, const uint32_t *__restrict__ b_src, const uint32_t *__restrict__ b_tgt,
				const uint32_t *__restrict__ o_off, const uint32_t *__restrict__ i_off, uint32_t *__restrict__ ocur,
				uint32_t *__restrict__ icur, uint32_t *__restrict__ o_adj, uint32_t *__restrict__ i_adj)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= NB)
		return;
	const uint32_t u = b_src[j], w = b_tgt[j];
	o_adj[o_off[u] + atomicAdd(&ocur[u], 1u)] = j;
	i_adj[i_off[w] + atomicAdd(&icur[w], 1u)] = j;
}
// literal hi of every vertex: min over the subtree of hi_0, the root once a simplifying edge was added at or below
__global__ void k_sub_hi(uint32_t T, const uint32_t *__restrict__ size, const SegTree segH, const uint32_t *__restrict__ simp_ps,
			 const CompAt comp, uint32_t *__restrict__ hi)
{
	const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= T)
		return;
	const uint32_t sz = size[v];
	if (!sz) {
		hi[v] = NIL;
		return;
	}
	if (simp_ps[v + sz] != simp_ps[v]) {
		const uint32_t c = comp.of_tree(v);
		hi[v] = 2 * comp.voff[c] + c;
		return;
	}
	hi[v] = seg_min(segH, v, v + sz);
}
// creation keys: one lane per vertex hands its ordinary edges (a stretch of the dense list in scan order) their tn
__global__ void k_sub_edge_keys(uint32_t T, const uint32_t *__restrict__ size, const uint32_t *__restrict__ out_ord,
				const uint32_t *__restrict__ eat, const uint32_t *__restrict__ wbefore, unsigned long long *__restrict__ ekey)
{
	const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
	if (u >= T || !size[u] || !out_ord[u])
		return;
	const uint32_t at = eat[u], n = out_ord[u], end = u + size[u];
	uint32_t r = 0;
	for (uint32_t c = u + 1; c < end && r < n; c += max(size[c], 1u)) {
		const uint32_t k = min(wbefore[c], n - r); // edges of u created right before c was discovered
		for (uint32_t x = 0; x < k; x++)
			ekey[at + r + x] = ((unsigned long long)c << 32) | (0xFFFFFFFFu - u);
		r += k;
	}
	for (; r < n; r++)
		ekey[at + r] = ((unsigned long long)end << 32) | (0xFFFFFFFFu - u);
}
// |brackets(v)| (count_brackets, tree_utils.cpp:531-574): ordinary edges from strictly below v to strictly above it; the
// root has none (the fill loop stops at it), self loops are in nobody's table (oracle: "leaf subflubble passes")
__global__ void k_sub_br_counts(uint32_t T, const uint32_t *__restrict__ size, const uint32_t *__restrict__ gp, const uint32_t *__restrict__ P,
				const uint32_t *__restrict__ out_ord, const uint32_t *__restrict__ nself, uint32_t *__restrict__ cnt)
{
	const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v > T)
		return;
	uint32_t n = 0;
	if (v < T && size[v] && gp[v] != NIL)
		n = (P[v + size[v]] - P[v]) - (out_ord[v] - nself[v]);
	cnt[v] = n;
}
// the ordinary edges in source order (a source's edges are a stretch of the dense list in scan order; the stretches
// themselves lie in no order): position O[u] + r holds the r-th edge of u
__global__ void k_sub_edges_by_source(uint32_t T, const uint32_t *__restrict__ size, const uint32_t *__restrict__ out_ord,
				      const uint32_t *__restrict__ eat, const uint32_t *__restrict__ O, const uint32_t *__restrict__ b_tgt,
				      uint32_t *__restrict__ tgt_s, uint32_t *__restrict__ slot_s)
{
	const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
	if (u >= T || !size[u])
		return;
	const uint32_t n = out_ord[u], at = eat[u], o = O[u];
	for (uint32_t r = 0; r < n; r++) {
		tgt_s[o + r] = b_tgt[at + r];
		slot_s[o + r] = at + r;
	}
}
// LoA without self-loop back edges (see the proof in oracle/povu_oracle_sub.inc): lo[v] = the deepest target t < v of an
// ordinary edge whose source lies behind v -- the largest left end among the intervals (t, s) that hold v.  Every edge marks
// the canonical nodes of its interval in a max-tree over the vertex indices, every vertex reads the nodes above its leaf.
__global__ void k_sub_lo_mark(uint32_t NB0, const uint32_t *__restrict__ b_src, const uint32_t *__restrict__ b_tgt, uint32_t P2,
			      uint32_t *__restrict__ tree)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= NB0)
		return;
	const uint32_t sv = b_src[j], tv = b_tgt[j];
	if (sv <= tv + 1)
		return;
	for (uint32_t l = tv + 1 + P2, r = sv + P2; l < r; l >>= 1, r >>= 1) {
		// (the nodes near the root are everybody's: most edges find a larger mark there already and need no atomic)
		if (l & 1) {
			if (tree[l] < tv + 1)
				atomicMax(&tree[l], tv + 1);
			l++;
		}
		if (r & 1) {
			--r;
			if (tree[r] < tv + 1)
				atomicMax(&tree[r], tv + 1);
		}
	}
}
__global__ void k_sub_lo_query(uint32_t T, const uint32_t *__restrict__ size, uint32_t P2, const uint32_t *__restrict__ tree,
			       const uint32_t *__restrict__ nself, const CompAt comp, uint32_t *__restrict__ lo, uint32_t *__restrict__ has_self)
{
	const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= T)
		return;
	if (!size[v]) {
		lo[v] = NIL;
		return;
	}
	// A back edge whose source is its own target stays in the reference's heap as a stale entry (it is pushed AFTER lo[v] is
	// taken and never popped).  The only one from_bd ever makes is the 0 -> 0 edge of a tip-less root (spanning_tree.cpp:433-438;
	// a self loop of the graph is stored as (side, other side): two vertices): pushed at the first tree vertex, which the
	// descending sweep visits LAST -- nobody reads the heap after it, the closed form stands.  Only a self edge anywhere else
	// (none can arise; kept as the defined answer should one ever) sends its component through the literal heap below.
	if (nself[v]) {
		const uint32_t c = comp.of_tree(v);
		if (v != 2 * comp.voff[c] + c)
			has_self[c] = 1; // (this component's values are overwritten by the literal heap below)
	}
	uint32_t m = 0;
	for (uint32_t x = v + P2; x >= 1; x >>= 1)
		m = max(m, tree[x]);
	lo[v] = m ? m - 1 : NIL;
}
// compute_LoA, tree_utils.cpp:224-273, with the heap steps of libstdc++ (push_heap; pop_heap = __adjust_heap to the bottom,
// then __push_heap): one lane per component THAT HAS a self-loop back edge, its heap in the stretch of `heap` its ordinary
// edges number
__global__ void k_sub_lo(uint32_t C, const uint32_t *__restrict__ voff, const uint32_t *__restrict__ c_ntree,
			 const uint32_t *__restrict__ size, const uint32_t *__restrict__ depth, const uint32_t *__restrict__ out_ord,
			 const uint32_t *__restrict__ eat, const uint32_t *__restrict__ b_tgt, const uint32_t *__restrict__ O,
			 const uint32_t *__restrict__ has_self, uint32_t *__restrict__ heap_all, uint32_t *__restrict__ lo)
{
	const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= C || !c_ntree[c] || !has_self[c])
		return;
	const uint32_t base = 2 * voff[c] + c, N = c_ntree[c];
	uint32_t *heap = heap_all + O[base];
	uint32_t hn = 0;
	for (uint32_t v = base + N; v-- > base;) {
		if (!size[v]) {
			lo[v] = NIL;
			continue;
		}
		while (hn && heap[0] == v) {
			const uint32_t value = heap[hn - 1], len = hn - 1;
			hn = len;
			if (!len)
				break;
			uint32_t hole = 0, child = 0;
			while (child < (len - 1) / 2) {
				child = 2 * (child + 1);
				if (depth[heap[child]] < depth[heap[child - 1]])
					child--;
				heap[hole] = heap[child];
				hole = child;
			}
			if ((len & 1) == 0 && child == (len - 2) / 2) {
				child = 2 * (child + 1);
				heap[hole] = heap[child - 1];
				hole = child - 1;
			}
			while (hole > 0 && depth[heap[(hole - 1) / 2]] < depth[value]) {
				heap[hole] = heap[(hole - 1) / 2];
				hole = (hole - 1) / 2;
			}
			heap[hole] = value;
		}
		lo[v] = hn ? heap[0] : NIL;
		const uint32_t n = out_ord[v], at = eat[v];
		for (uint32_t r = 0; r < n; r++) { // OBE(v) in back-edge idx order = the source's scan order
			const uint32_t x = b_tgt[at + r];
			uint32_t i = hn++;
			while (i && depth[heap[(i - 1) / 2]] < depth[x]) {
				heap[i] = heap[(i - 1) / 2];
				i = (i - 1) / 2;
			}
			heap[i] = x;
		}
	}
}

// ------------------------------------------------------------------ find_concealed: the search (concealed.cpp:234-921)
struct Slub {
	uint32_t q, loc, sl, be_src; // flubble (dense slot), cl_e, the slubble's tree vertex, ai_trunk: the back edge's source
};
// compute_m, concealed.cpp:234-283
__device__ uint32_t cn_compute_m(const SubT &t, uint32_t ii, uint32_t ji)
{
	if (t.i_off[ii + 1] == t.i_off[ii])
		return ii;
	uint32_t best = NIL, best_h = 0;
	for (uint32_t b = t.i_off[ii]; b < t.i_off[ii + 1]; b++) {
		const uint32_t j = t.i_adj[b];
		if (!t.ordinary(j))
			continue;
		const uint32_t l = t.lca(t.b_src[j], ji);
		if (t.depth[l] >= t.depth[ji])
			continue;
		if (t.depth[l] > best_h) {
			best = l;
			best_h = t.depth[l];
		}
	}
	return best == NIL ? ii : best;
}
// compute_n, concealed.cpp:285-328
__device__ uint32_t cn_compute_n(const SubT &t, uint32_t ii, uint32_t ji)
{
	if (t.count_ord(t.o_off, t.o_adj, ji) == 0)
		return ji;
	uint32_t lowest = ii;
	for (uint32_t b = t.o_off[ji]; b < t.o_off[ji + 1]; b++) {
		const uint32_t j = t.o_adj[b];
		if (!t.ordinary(j))
			continue;
		if (t.depth[t.b_tgt[j]] > t.depth[lowest])
			lowest = t.b_tgt[j];
	}
	return lowest == ii ? ji : lowest;
}
// can_contain, concealed.cpp:348-384
__device__ bool cn_can_contain(const SubT &t, uint32_t ii, uint32_t ji, uint32_t m, uint32_t n)
{
	if (t.dep(t.lo[ji]) < t.depth[ii])
		return false;
	uint32_t ibe_ii = 0;
	for (uint32_t b = t.i_off[ii]; b < t.i_off[ii + 1]; b++) {
		const uint32_t j = t.i_adj[b];
		ibe_ii += (t.ordinary(j) && t.b_src[j] != ji) ? 1u : 0u;
	}
	if (m == ii && n == ji && ibe_ii < 2 && t.count_ord(t.i_off, t.i_adj, ji) == 0 && t.nchild[ji] < 3)
		return false;
	return true;
}
// ai_trunk, concealed.cpp:388-522
__device__ bool cn_ai_trunk(const SubT &t, uint32_t m, uint32_t n, uint32_t ai, uint32_t zi, uint32_t &be_src, uint32_t &l_out)
{
	if (t.depth[m] > t.depth[n])
		return false;
	uint32_t best_l = NIL, best_src = NIL;
	for (uint32_t b = t.i_off[ai]; b < t.i_off[ai + 1]; b++) {
		const uint32_t j = t.i_adj[b];
		if (!t.ordinary(j))
			continue;
		const uint32_t src = t.b_src[j], l = t.lca(src, zi);
		if (t.depth[l] > t.depth[m])
			continue;
		bool ell_br = true;
		{
			SubT::BrRange br = t.brackets(l);
			for (uint32_t e = t.br_next(br); e != NIL && ell_br; e = t.br_next(br))
				ell_br = t.depth[t.b_tgt[e]] <= t.depth[ai];
		}
		const bool cond_iii = t.o_off[l + 1] > t.o_off[l] || t.nchild[l] > 1;
		if (!ell_br && cond_iii)
			continue;
		// (the reference keeps the last of equal LCAs in back-edge idx order; which source survives shows nowhere -- it only
		// enters Concealed::bounds_, oracle/povu_oracle_sub.inc -- so any fixed choice does: the largest source)
		if (best_l == NIL || l > best_l || (l == best_l && src > best_src)) {
			best_l = l;
			best_src = src;
		}
	}
	if (best_l == NIL)
		return false;
	be_src = best_src;
	l_out = best_l;
	return true;
}
__device__ uint32_t lca_of_bracket_srcs(const SubT &t, uint32_t c)
{
	uint32_t d = NIL;
	SubT::BrRange br = t.brackets(c);
	for (uint32_t e = t.br_next(br); e != NIL; e = t.br_next(br)) {
		const uint32_t src = t.b_src[e];
		d = d == NIL ? src : t.lca(d, src);
	}
	return d;
}
// the searches push their slubbles through this: out == null counts
struct SlubOut {
	Slub *out;
	uint32_t n;
	__device__ __forceinline__ void push(uint32_t q, uint32_t loc, uint32_t sl, uint32_t be_src)
	{
		if (out)
			out[n] = Slub{q, loc, sl, be_src};
		n++;
	}
};
// ai_branches, concealed.cpp:525-583
__device__ void cn_ai_branches(const SubT &t, uint32_t q, uint32_t ai, uint32_t zi, SlubOut &o)
{
	if (t.nchild[zi] < 2)
		return;
	const uint32_t end = zi + t.size[zi];
	for (uint32_t c = zi + 1; c < end; c += max(t.size[c], 1u)) {
		if (!(t.hi[c] == t.lo[c] && t.hi[c] == ai))
			continue;
		if (t.n_br(c) < 2)
			continue;
		const uint32_t d = lca_of_bracket_srcs(t, c);
		if (t.n_br(d) > 0)
			o.push(q, CL_AI_BRANCH, d, NIL);
	}
}
// override_ji_trunk, concealed.cpp:617-697
__device__ uint32_t cn_override_ji_trunk(const SubT &t, uint32_t m, uint32_t n, uint32_t ii, uint32_t ji)
{
	if (t.depth[m] > t.depth[n])
		return NIL;
	uint32_t min_v = n;
	const uint32_t end = ji + t.size[ji];
	for (uint32_t c = ji + 1; c < end; c += max(t.size[c], 1u)) {
		if (t.dep(t.hi[c]) < t.depth[ii])
			continue;
		if (t.n_br(c) != 1)
			continue;
		SubT::BrRange br1 = t.brackets(c);
		const uint32_t y = t.b_tgt[t.br_next(br1)];
		if (!(t.depth[m] < t.depth[y] && t.depth[n] > t.depth[y]))
			continue;
		bool valid = true;
		SubT::BrRange bry = t.brackets(y);
		for (uint32_t j = t.br_next(bry); j != NIL && valid; j = t.br_next(bry))
			if (t.depth[t.b_src[j]] < t.depth[ji] || t.depth[t.b_tgt[j]] > t.depth[ii])
				valid = false;
		if (valid && t.depth[y] < t.depth[min_v])
			min_v = y;
	}
	return min_v == n ? NIL : min_v;
}
// ji_trunk, concealed.cpp:699-760 (the rest of the function is behind a return)
__device__ uint32_t cn_ji_trunk(const SubT &t, uint32_t m, uint32_t n, uint32_t ii, uint32_t ji)
{
	if (t.depth[m] > t.depth[n])
		return NIL;
	const uint32_t r = cn_override_ji_trunk(t, m, n, ii, ji);
	if (r != NIL)
		return r;
	uint32_t best = NIL;
	for (uint32_t b = t.o_off[ji]; b < t.o_off[ji + 1]; b++) {
		const uint32_t j = t.o_adj[b];
		if (!t.ordinary(j))
			continue;
		const uint32_t x = t.b_tgt[j];
		if (t.depth[x] < t.depth[n])
			continue;
		if (best == NIL || t.depth[x] < t.depth[best])
			best = x;
	}
	return best;
}
// ji_branches, concealed.cpp:790-921
__device__ void cn_ji_branches(const SubT &t, uint32_t q, uint32_t ii, uint32_t ji, uint32_t n, SlubOut &o)
{
	if (t.nchild[ji] < 2 || ji == n)
		return;
	bool have_main = false;
	for (uint32_t b = t.i_off[ii]; b < t.i_off[ii + 1] && !have_main; b++) {
		const uint32_t j = t.i_adj[b];
		have_main = t.ordinary(j) && t.b_src[j] == ji;
	}
	const uint32_t end = ji + t.size[ji];
	for (int pass = 0; pass < 2; pass++) {
		for (uint32_t c = ji + 1; c < end; c += max(t.size[c], 1u)) {
			uint32_t count = 0;
			bool into_ji = false;
			{
				SubT::BrRange br = t.brackets(c);
				for (uint32_t e = t.br_next(br); e != NIL; e = t.br_next(br)) {
					if (t.b_tgt[e] != ji)
						count++;
					else
						into_ji = true;
				}
			}
			if (count != 1 || into_ji != (pass == 0))
				continue;
			if (pass == 0) {
				// the deepest source of a bracket into ji; among equally deep ones the reference keeps the first in back-edge
				// idx order (depth[src] > depth[lowest], concealed.cpp:846)
				uint32_t lowest = c, low_e = NIL;
				SubT::BrRange br = t.brackets(c);
				for (uint32_t j = t.br_next(br); j != NIL; j = t.br_next(br)) {
					if (t.b_tgt[j] != ji)
						continue;
					const uint32_t sv = t.b_src[j];
					if (t.depth[sv] > t.depth[lowest] || (low_e != NIL && t.depth[sv] == t.depth[lowest] && t.created_before(j, low_e))) {
						lowest = sv;
						low_e = j;
					}
				}
				o.push(q, CL_ZI_BRANCH, lowest, NIL);
			} else {
				SubT::BrRange br = t.brackets(c);
				const uint32_t j = t.br_next(br); // (its only bracket)
				const uint32_t src = t.b_src[j], tgt = t.b_tgt[j];
				bool cond_i = false;
				uint32_t d = src;
				while (d != ji) {
					if (t.nchild[d] > 1) {
						cond_i = true;
						break;
					}
					d = t.gp[d];
				}
				const uint32_t alpha = t.n_br(tgt);
				if (alpha != 0 && have_main)
					continue;
				if (alpha != 1)
					continue;
				if (cond_i)
					o.push(q, CL_ZI_BRANCH, d, NIL);
			}
		}
	}
}
// find_concealed's loop body for the flubble in dense slot q (concealed.cpp:1203-1237); returns its slubbles
__device__ uint32_t cn_search(const SubT &t, const CompAt &comp, uint32_t q, Slub *out, uint32_t *mn)
{
	if (t.p_fam[q] != FAM_FLUBBLE)
		return 0;
	const uint32_t c = comp.of_slot(q), base = t.base_of(c);
	const uint32_t ai = base + t.p_ai[q], zi = base + t.p_zi[q];
	const uint32_t m = cn_compute_m(t, ai, zi), n = cn_compute_n(t, ai, zi);
	if (mn) {
		mn[2 * (size_t)q] = m;
		mn[2 * (size_t)q + 1] = n;
	}
	if (!cn_can_contain(t, ai, zi, m, n))
		return 0;
	SlubOut o{out, 0};
	uint32_t be_src, l;
	if (cn_ai_trunk(t, m, n, ai, zi, be_src, l))
		o.push(q, CL_AI_TRUNK, l, be_src);
	cn_ai_branches(t, q, ai, zi, o);
	const uint32_t tb = cn_ji_trunk(t, m, n, ai, zi);
	if (tb != NIL)
		o.push(q, CL_ZI_TRUNK, tb, NIL);
	cn_ji_branches(t, q, ai, zi, n, o);
	return o.n;
}
__global__ void k_sub_cn_count(uint32_t Q, const SubT t, const CompAt comp, uint32_t *__restrict__ cnt, uint32_t *__restrict__ mn)
{
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q > Q)
		return;
	cnt[q] = q < Q ? cn_search(t, comp, q, nullptr, mn) : 0u;
}
__global__ void k_sub_cn_emit(uint32_t Q, const SubT t, const CompAt comp, const uint32_t *__restrict__ off, Slub *__restrict__ out)
{
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= Q || off[q + 1] == off[q])
		return;
	cn_search(t, comp, q, out + off[q], nullptr);
}

// ------------------------------------------------------------------ find_smothered: the search (smothered.cpp:61-318)
struct Smo {
	uint32_t sm_st, b_up, b_lo, flags; // flags: 1 = cn_b is the ancestor, 2 = the concealed vertex is a g
};
struct SmoOut {
	Smo *out;
	uint32_t n;
	__device__ __forceinline__ void push(uint32_t sm_st, bool anc, bool is_g, uint32_t up, uint32_t lo)
	{
		if (out)
			out[n] = Smo{sm_st, up, lo, (anc ? 1u : 0u) | (is_g ? 2u : 0u)};
		n++;
	}
};
// compute_bounds, smothered.cpp:37-48
__device__ __forceinline__ void smo_bounds(const SubT &t, uint32_t cn_st, uint32_t sm_st, uint32_t &up, uint32_t &lo)
{
	if (t.is_desc(cn_st, sm_st))
		up = cn_st, lo = sm_st;
	else
		up = sm_st, lo = cn_st;
}
// the next distinct value above `last` of key[adj[..]] over a row, NIL when there is none (std::set iteration without a set)
__device__ uint32_t next_distinct(const uint32_t *off, const uint32_t *adj, const uint32_t *key, uint32_t v, uint32_t last, bool first)
{
	uint32_t best = NIL;
	for (uint32_t b = off[v]; b < off[v + 1]; b++) {
		const uint32_t x = key[adj[b]];
		if ((first || x > last) && (best == NIL || x < best))
			best = x;
	}
	return best;
}
__device__ uint32_t smo_search(const SubT &t, const CompAt &comp, const Slub &cn, Smo *out)
{
	SmoOut o{out, 0};
	const uint32_t c = comp.of_slot(cn.q), base = t.base_of(c);
	const uint32_t ai = base + t.p_ai[cn.q], zi = base + t.p_zi[cn.q], sl = cn.sl;
	switch (cn.loc) {
	case CL_AI_TRUNK: { // g::trunk, smothered.cpp:61-134
		const uint32_t end = sl + t.size[sl];
		for (uint32_t ch = sl + 1; ch < end; ch += max(t.size[ch], 1u)) {
			if (t.n_br(ch) == 0)
				continue;
			// the LAST bracket of the row in back-edge idx order (be_idx_, smothered.cpp:94-101) and whether all have its source
			uint32_t last = NIL;
			{
				SubT::BrRange br = t.brackets(ch);
				for (uint32_t e = t.br_next(br); e != NIL; e = t.br_next(br))
					if (last == NIL || t.created_before(last, e))
						last = e;
			}
			const uint32_t src = t.b_src[last], tgt = t.b_tgt[last];
			bool one_src = true;
			{
				SubT::BrRange br = t.brackets(ch);
				for (uint32_t e = t.br_next(br); e != NIL && one_src; e = t.br_next(br))
					one_src = t.b_src[e] == src;
			}
			if (!(one_src && t.depth[tgt] > t.depth[ai]))
				continue;
			const uint32_t brch = t.lca(zi, src);
			if (t.n_br(src) == 0)
				o.push(tgt, false, true, brch, src);
			else
				o.push(src, true, true, brch, src);
		}
		break;
	}
	case CL_AI_BRANCH: { // g::branch, :136-199
		const uint32_t t0 = next_distinct(t.o_off, t.o_adj, t.b_tgt, sl, 0, true);
		if (t0 == NIL || t0 != ai || next_distinct(t.o_off, t.o_adj, t.b_tgt, sl, t0, false) != NIL)
			break;
		// the brackets of sl that end at ai, in back-edge idx order (the row is enumerated in source order: the next one is
		// the earliest created behind the last); each gives one vertex per bracket of its source that ends at sl
		uint32_t prev_e = NIL;
		for (;;) {
			uint32_t best = NIL;
			SubT::BrRange br = t.brackets(sl);
			for (uint32_t j = t.br_next(br); j != NIL; j = t.br_next(br)) {
				if (t.b_tgt[j] != ai)
					continue;
				if (prev_e != NIL && !t.created_before(prev_e, j))
					continue;
				if (best == NIL || t.created_before(j, best))
					best = j;
			}
			if (best == NIL)
				break;
			prev_e = best;
			const uint32_t src = t.b_src[best];
			SubT::BrRange br2 = t.brackets(src);
			for (uint32_t r = t.br_next(br2); r != NIL; r = t.br_next(br2))
				if (t.b_tgt[r] == sl) {
					uint32_t up, lo;
					smo_bounds(t, sl, src, up, lo);
					o.push(src, true, true, up, lo);
				}
		}
		break;
	}
	case CL_ZI_TRUNK: { // s::trunk, :217-270: the sources by their LCA with zi, ascending; an LCA with one source gives a vertex
		uint32_t last_l = 0;
		bool first_l = true;
		for (;;) {
			// the next LCA value above last_l among the kept sources
			uint32_t best_l = NIL;
			for (uint32_t b = t.i_off[sl]; b < t.i_off[sl + 1]; b++) {
				const uint32_t src = t.b_src[t.i_adj[b]];
				if (t.depth[src] >= t.depth[zi])
					continue;
				const uint32_t l = t.lca(zi, src);
				if (l == src)
					continue;
				if ((first_l || l > last_l) && (best_l == NIL || l < best_l))
					best_l = l;
			}
			if (best_l == NIL)
				break;
			// its distinct sources
			uint32_t cnt = 0, only = NIL, last_s = 0;
			bool first_s = true;
			for (;;) {
				uint32_t best_s = NIL;
				for (uint32_t b = t.i_off[sl]; b < t.i_off[sl + 1]; b++) {
					const uint32_t src = t.b_src[t.i_adj[b]];
					if (t.depth[src] >= t.depth[zi])
						continue;
					const uint32_t l = t.lca(zi, src);
					if (l != best_l || l == src)
						continue;
					if ((first_s || src > last_s) && (best_s == NIL || src < best_s))
						best_s = src;
				}
				if (best_s == NIL)
					break;
				cnt++;
				only = best_s;
				last_s = best_s;
				first_s = false;
			}
			if (cnt == 1)
				o.push(only, false, false, best_l, only);
			last_l = best_l;
			first_l = false;
		}
		break;
	}
	case CL_ZI_BRANCH: { // s::branch, :272-318
		uint32_t last = 0;
		bool first = true;
		for (;;) {
			const uint32_t src = next_distinct(t.i_off, t.i_adj, t.b_src, sl, last, first);
			if (src == NIL)
				break;
			uint32_t l2 = 0;
			bool f2 = true;
			for (;;) {
				const uint32_t x = next_distinct(t.i_off, t.i_adj, t.b_src, src, l2, f2);
				if (x == NIL)
					break;
				uint32_t up, lo;
				smo_bounds(t, x, sl, up, lo);
				o.push(x, true, false, up, lo);
				l2 = x;
				f2 = false;
			}
			l2 = 0;
			f2 = true;
			for (;;) {
				const uint32_t x = next_distinct(t.o_off, t.o_adj, t.b_tgt, src, l2, f2);
				if (x == NIL)
					break;
				if (x != zi) {
					uint32_t up, lo;
					smo_bounds(t, x, sl, up, lo);
					o.push(x, false, false, up, lo);
				}
				l2 = x;
				f2 = false;
			}
			last = src;
			first = false;
		}
		break;
	}
	}
	return o.n;
}
__global__ void k_sub_smo_count(uint32_t NC, const SubT t, const CompAt comp, const Slub *__restrict__ cn, uint32_t *__restrict__ cnt)
{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k > NC)
		return;
	cnt[k] = k < NC ? smo_search(t, comp, cn[k], nullptr) : 0u;
}
__global__ void k_sub_smo_emit(uint32_t NC, const SubT t, const CompAt comp, const Slub *__restrict__ cn, const uint32_t *__restrict__ off,
			       Smo *__restrict__ out)
{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= NC || off[k + 1] == off[k])
		return;
	smo_search(t, comp, cn[k], out + off[k]);
}

// ------------------------------------------------------------------ the splice, one wave per component
// The extended PVST of component c lives in X-space: x = xoff[c] + (index inside the component).  Children of a vertex: a
// vector {begin, size, capacity} in the component's stretch of the pool, doubled when full (pvst.hpp:860-885).
struct XArrays {
	uint8_t *fam, *or1, *or2, *route, *loc;
	uint32_t *id1, *id2, *ai, *zi, *sl, *b_up, *b_lo; // ai / zi: global tree vertex; b_up / b_lo: bounds_t (global tree vertex, or PVST idx for a midi)
	uint32_t *vbeg, *vn, *vcap;
	uint32_t *pool;
};
// One WAVE works on the children vectors of ONE vertex and of the vertices it creates (see "the splice, in parallel"
// below).  The control flow is the reference's, followed by all 64 lanes alike (every decision is read from the same address
// by every lane); lane 0 does the stores, and the two loops that are long on a flubble with very many children -- copying a
// vector that grows, filtering the children that leave -- are shared out over the lanes.
struct Splice {
	XArrays x;
	uint32_t xb;	    // first X slot of the component
	uint32_t *pool_top; // bump pointer inside the component's stretch of the pool: shared by the waves of the component
	uint32_t pool_end;
	uint32_t *err;
	uint32_t lane;
	__device__ __forceinline__ void sync() const { __syncthreads(); } // (one wave a workgroup)
	// room for `extra` more entries in the vector of `parent`
	__device__ bool reserve(uint32_t parent, uint32_t extra)
	{
		const uint32_t p = xb + parent, n = x.vn[p], cap = x.vcap[p];
		if (n + extra <= cap)
			return true;
		uint32_t ncap = cap ? cap : 4;
		while (ncap < n + extra)
			ncap *= 2;
		uint32_t at = 0;
		if (lane == 0)
			at = ncap < n ? NIL : atomicAdd(pool_top, ncap);
		at = __shfl(at, 0);
		if (at == NIL || at + ncap > pool_end || at + ncap < at) {
			if (lane == 0)
				atomicOr(err, E_POOL);
			return false;
		}
		const uint32_t from = x.vbeg[p];
		for (uint32_t k = lane; k < n; k += 64)
			x.pool[at + k] = x.pool[from + k];
		sync();
		if (lane == 0) {
			x.vbeg[p] = at;
			x.vcap[p] = ncap;
		}
		sync();
		return true;
	}
	__device__ bool push(uint32_t parent, uint32_t child)
	{
		if (!reserve(parent, 1))
			return false;
		const uint32_t p = xb + parent;
		if (lane == 0) {
			x.pool[x.vbeg[p] + x.vn[p]] = child;
			x.vn[p] = x.vn[p] + 1;
		}
		sync();
		return true;
	}
	// del_edge: erase the first match; the slot behind the new end keeps its old value, as vector::erase leaves it
	__device__ void erase(uint32_t parent, uint32_t child)
	{
		const uint32_t p = xb + parent, b = x.vbeg[p], n = x.vn[p];
		if (lane == 0)
			for (uint32_t k = 0; k < n; k++)
				if (x.pool[b + k] == child) {
					for (uint32_t a = k; a + 1 < n; a++)
						x.pool[b + a] = x.pool[b + a + 1];
					x.vn[p] = n - 1;
					break;
				}
		sync();
	}
	__device__ __forceinline__ bool fl_like(uint32_t v) const
	{
		const uint8_t f = x.fam[xb + v];
		return f == FAM_FLUBBLE || f == FAM_TINY || f == FAM_PARALLEL;
	}
	// The nestings of add_concealed / add_midi run over a COPY of the first nch children of f and move those that `leaves`
	// says so, in order, under `dest` (to_child: the other way round -- `dest` is pushed into the vector of each of them,
	// concealed.cpp:1077: that push is the CHILD's, see k_sub_pin; here the child only leaves the vector of f).  A stable
	// filter, 64 children a round; returns false when the pool ran out.
	template <typename Leaves>
	__device__ bool filter(uint32_t f, uint32_t nch, uint32_t dest, bool to_child, Leaves &&leaves)
	{
		const uint32_t pf = xb + f;
		uint32_t w = 0;
		for (uint32_t r0 = 0; r0 < nch; r0 += 64) {
			const uint32_t r = r0 + lane, fb = x.vbeg[pf];
			const bool valid = r < nch;
			const uint32_t ch = valid ? x.pool[fb + r] : 0u;
			const bool moved = valid && leaves(ch);
			const unsigned long long mm = __ballot(moved), km = __ballot(valid && !moved);
			const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
			sync(); // (every lane holds its child: the slots may be written now)
			if (valid && !moved)
				x.pool[fb + w + (uint32_t)__popcll(km & below)] = ch;
			w += (uint32_t)__popcll(km);
			if (mm) {
				if (!to_child) {
					const uint32_t cnt = (uint32_t)__popcll(mm);
					if (!reserve(dest, cnt))
						return false;
					const uint32_t pd = xb + dest;
					if (moved)
						x.pool[x.vbeg[pd] + x.vn[pd] + (uint32_t)__popcll(mm & below)] = ch;
					sync();
					if (lane == 0)
						x.vn[pd] = x.vn[pd] + cnt;
					sync();
				}
			}
			sync();
		}
		if (lane == 0)
			x.vn[pf] = w;
		sync();
		return true;
	}
};
__device__ __forceinline__ void side_id_or(const SubT &t, uint32_t v, bool fwd_is_r, uint32_t &id, uint8_t &orr)
{
	id = t.gid[v];
	const bool is_r = (t.flags[v] & TF_TYPE_MASK) == 1u;
	orr = (is_r == fwd_is_r) ? 0 : 1;
}
// the PVST as find_flubbles left it, in X-space: fields of every vertex and the capacity of its children vector (one lane
// per dense PVST slot); then the vectors themselves, children in ascending idx (add_flubbles attaches them in that order)
__global__ void k_sub_x_init(uint32_t Q, const SubT t, const CompAt comp, const uint32_t *__restrict__ xoff, XArrays X)
{
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= Q)
		return;
	const uint32_t c = comp.of_slot(q), v = q - t.doff[c], x = xoff[c] + v, base = t.base_of(c);
	X.fam[x] = t.p_fam[q];
	X.loc[x] = 0;
	X.sl[x] = X.b_up[x] = X.b_lo[x] = NIL;
	if (v) {
		X.id1[x] = t.p_a[q], X.or1[x] = t.p_aor[q];
		X.id2[x] = t.p_z[q], X.or2[x] = t.p_zor[q];
		X.route[x] = 'L';
		X.ai[x] = base + t.p_ai[q], X.zi[x] = base + t.p_zi[q];
	} else {
		X.id1[x] = X.id2[x] = NIL;
		X.or1[x] = X.or2[x] = 0;
		X.route[x] = 0;
		X.ai[x] = X.zi[x] = NIL;
	}
}
// POVU_HIP_SUB_SERIAL_SPLICE (tests): X-space as a pass on another graph may have left it, before k_sub_x_init writes the
// PVST slots.  Every slot gets a flubble whose bounds make cn_leaves say "leaves" for as many records as can be: zi the
// component's root (depth 0, no bracket, below no vertex), ai its last vertex in preorder (below every vertex of the
// rightmost path).  Each index stays inside the slot's own component (one lane per X slot; of_slot over xoff gives the
// component that owns the slot: the stretches of components without a PVST are empty), so no stale read leaves an array.
__global__ void k_sub_x_poison(uint32_t NX, const SubT t, const CompAt comp_x, const uint32_t *__restrict__ xoff, XArrays X)
{
	const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= NX)
		return;
	const uint32_t c = comp_x.of_slot(x), base = t.base_of(c), N = t.c_ntree[c];
	if (!N) { // (no tree: a slot nobody reads as a flubble)
		X.fam[x] = FAM_DUMMY;
		X.ai[x] = X.zi[x] = X.sl[x] = X.b_up[x] = X.b_lo[x] = NIL;
		X.id1[x] = X.id2[x] = NIL;
		X.loc[x] = 0, X.or1[x] = X.or2[x] = 0, X.route[x] = 0;
		return;
	}
	const uint32_t root = base, last = base + N - 1;
	X.fam[x] = FAM_FLUBBLE;
	X.loc[x] = (uint8_t)((x - xoff[c]) & 3u);
	X.ai[x] = last, X.zi[x] = root;
	X.sl[x] = last, X.b_up[x] = root, X.b_lo[x] = last;
	X.id1[x] = t.gid[root], X.id2[x] = t.gid[last];
	X.or1[x] = 1, X.or2[x] = 1, X.route[x] = 'R';
}
// where the children of X slot x begin among the sorted (parent slot, child) pairs = how many pairs have a smaller key: a
// binary search per slot (counting them with atomics put a million adds on the word of a chromosome's root)
__global__ void k_sub_x_vbeg(uint32_t Q, const SubT t, const CompAt comp, const uint32_t *__restrict__ xoff,
			     const uint32_t *__restrict__ poff, const uint32_t *__restrict__ key, uint32_t *__restrict__ cap_ps, XArrays X)
{
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= Q)
		return;
	const uint32_t c = comp.of_slot(q), x = xoff[c] + (q - t.doff[c]);
	const uint32_t b = lower_bound(key, 0u, Q, x), e = lower_bound(key, 0u, Q, x + 1), b0 = lower_bound(key, 0u, Q, xoff[c]);
	cap_ps[x] = b;
	X.vbeg[x] = poff[c] + (b - b0);
	X.vn[x] = X.vcap[x] = e - b;
}
// children in ascending idx: a stable sort of (X slot of the parent, child) over the dense slots, which are in ascending
// idx already (one lane sorting the million children of a chromosome's root took seconds)
__global__ void k_sub_x_keys(uint32_t Q, uint32_t NX, const SubT t, const CompAt comp, const uint32_t *__restrict__ xoff,
			     uint32_t *__restrict__ key, uint32_t *__restrict__ val)
{
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= Q)
		return;
	const uint32_t c = comp.of_slot(q), v = q - t.doff[c];
	key[q] = v ? xoff[c] + t.p_parent[q] : NX; // (the roots have no parent: behind everything)
	val[q] = v;
}
__global__ void k_sub_x_place(uint32_t Q, uint32_t NX, const uint32_t *__restrict__ key, const uint32_t *__restrict__ val,
			      const uint32_t *__restrict__ cap_ps, XArrays X)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= Q)
		return;
	const uint32_t x = key[i];
	if (x >= NX)
		return;
	X.pool[X.vbeg[x] + (i - cap_ps[x])] = val[i];
}
// ------------------------------------------------------------------ the splice, in parallel
// Until round 5 one wave spliced a whole component, flubble after flubble (94 ms for the whole-genome workload: 10^4
// flubbles of a chromosome with a concealed bubble, some ten dependent trips to memory each).  What add_concealed does to
// one flubble f depends on nothing another flubble's turn writes (the one vertex of another turn in f's vector, the one its
// parent pushes, is known by its index alone: cn_leaves; tests/test_gpu_splice_schedule.py runs the turns in either order):
//  * its records (cn[]: found before, in ascending idx) each become the vertex n0 + (index of the record in the
//    component) -- no counter;
//  * a record's nesting moves children of f under the new vertex, or (z-side trunk) pushes the new vertex into the vector
//    of the children that qualify and drops them from f's vector.  Whether a child qualifies is a function of the trees
//    alone (cn_leaves), so the CHILD can work out by itself which vertex its parent's records push into its vector: it
//    walks the parent's records in order until one takes it (k_sub_pin, one lane per PVST vertex; at most one vertex ever
//    arrives, because the record that pushes it also drops the child from the parent's vector).  The parent has the
//    smaller idx, its turn comes first: the pushed vertex stands in front of the child's own concealed vertices;
//  * the vectors grow out of the component's pool by an atomic bump.
// So: one wave per flubble that has records or takes a vertex in (k_sub_splice_cn); the flubbles that got a concealed child
// are flagged instead of listed.  find_midi looks at each of them (k_sub_midi_find, all before the first is added, as in the
// reference), a scan over their flags numbers the midi bubbles in ascending idx, k_sub_midi_add attaches them; add_smothered
// works on the vector of one concealed vertex (k_sub_smothered, one wave per concealed vertex that has records).
struct SpliceArgs {
	SubT t;
	CompAt comp;
	const uint32_t *xoff, *poff;
	uint32_t *ptop; // [C] bump pointers
	const uint32_t *cn_off;
	const Slub *cn;
	const uint32_t *mn;
	const uint32_t *smo_off;
	const Smo *smo;
	XArrays X;
	uint32_t *pin;	  // [Q] the concealed vertex the parent's records push into the vector of this one (NIL: none)
	uint8_t *act;	  // [Q] has records or takes a vertex in
	uint8_t *touched; // [Q] got a concealed vertex as a child
	uint8_t *md;	  // [Q] gets a midi bubble
	const uint32_t *md_ps; // [Q + 1] exclusive scan of md
};
// what the nestings of add_concealed ask of a child of the flubble (ai, zi, n_of_f) for the slubble sl.  A child past the
// PVST (ch >= n0) is a concealed vertex -- the flubble's own, or the one its parent's z-side trunk record pushed (k_sub_pin)
// -- and never F / T / O: decided by its index, since the parent's wave writes the fields of that one in the same launch
__device__ bool cn_leaves(const SubT &t, const XArrays &X, uint32_t xb, uint32_t n0, const Slub &sl, uint32_t ai, uint32_t zi, uint32_t n_of_f,
			  uint32_t ch)
{
	if (ch >= n0)
		return false;
	const uint8_t fam = X.fam[xb + ch];
	if (!(fam == FAM_FLUBBLE || fam == FAM_TINY || fam == FAM_PARALLEL))
		return false;
	const uint32_t c_ai = X.ai[xb + ch], c_zi = X.zi[xb + ch];
	if (sl.loc == CL_AI_TRUNK) // nest_trunk_ai, :945-979
		return t.depth[sl.sl] > t.depth[c_zi] || t.is_desc(sl.sl, c_ai);
	if (sl.loc == CL_AI_BRANCH) { // nest_branch_ai, :984-1034
		bool has_br = false;  // a bracket of the child's zi that STARTS at ai (sic: get_src, :1006)
		SubT::BrRange br = t.brackets(c_zi);
		for (uint32_t e = t.br_next(br); e != NIL && !has_br; e = t.br_next(br))
			has_br = t.b_src[e] == ai;
		return t.is_desc(sl.sl, c_ai) && has_br;
	}
	// nest_trunk_zi, :1054-1081: (sic) the edge goes from the child to the slubble
	return t.is_desc(n_of_f, c_ai) && !t.is_desc(zi, c_zi);
}
// PVST vertices, concealed and smothered records of every component (what the host lays the splice out by)
__global__ void k_sub_comp_counts(uint32_t C, const uint32_t *__restrict__ doff, const uint32_t *__restrict__ c_npvst,
				  const uint32_t *__restrict__ cn_off, const uint32_t *__restrict__ smo_off, uint32_t *__restrict__ out)
{
	const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= C)
		return;
	const uint32_t n0 = c_npvst[c], q0 = doff[c];
	uint32_t ncn = 0, nsm = 0;
	if (n0) {
		const uint32_t b = cn_off[q0], e = cn_off[q0 + n0];
		ncn = e - b;
		nsm = smo_off[e] - smo_off[b];
	}
	out[3 * c] = n0, out[3 * c + 1] = ncn, out[3 * c + 2] = nsm;
}
__global__ void k_sub_ptop(uint32_t C, const uint32_t *__restrict__ poff, const uint32_t *__restrict__ c_npvst, uint32_t *__restrict__ ptop)
{
	const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c < C) // (the vectors of find_flubbles' vertices are in place: k_sub_x_init .. k_sub_x_place)
		ptop[c] = poff[c] + (c_npvst[c] ? c_npvst[c] - 1 : 0u);
}
__global__ void k_sub_pin(uint32_t Q, const SpliceArgs A)
{
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= Q)
		return;
	const SubT &t = A.t;
	const uint32_t c = A.comp.of_slot(q), q0 = t.doff[c], ch = q - q0;
	uint32_t pin = NIL;
	const bool own = A.cn_off[q + 1] != A.cn_off[q];
	if (ch) { // (the root has no parent)
		const uint32_t f = t.p_parent[q], qf = q0 + f;
		const uint32_t kb = A.cn_off[qf], ke = A.cn_off[qf + 1];
		if (kb != ke) {
			const uint32_t xb = A.xoff[c], base = t.base_of(c), N = t.c_ntree[c], n0 = t.c_npvst[c], cn_b = A.cn_off[q0];
			const bool is_leaf = f < N && t.nchild[base + f] == 0; // (sic) the SPANNING TREE's vertex f, concealed.cpp:1188
			if (!is_leaf) {
				const uint32_t ai = A.X.ai[xb + f], zi = A.X.zi[xb + f], n_of_f = A.mn[2 * (size_t)qf + 1];
				for (uint32_t k = kb; k < ke; k++) {
					const Slub sl = A.cn[k];
					if (sl.loc == CL_ZI_BRANCH)
						continue;
					if (cn_leaves(t, A.X, xb, n0, sl, ai, zi, n_of_f, ch)) { // this record takes it out of f's vector
						if (sl.loc == CL_ZI_TRUNK)
							pin = n0 + (k - cn_b);
						break;
					}
				}
			}
		}
	}
	A.pin[q] = pin;
	A.act[q] = (own || pin != NIL) ? 1 : 0;
	A.touched[q] = 0;
	A.md[q] = 0;
}
static constexpr unsigned SPLICE_WAVES = 8192; // waves of a splice kernel: each takes every SPLICE_WAVES-th entry of its list
// POVU_HIP_SUB_SERIAL_SPLICE=reverse (tests): the compacted list back to front, so one wave takes every child before its parent
__global__ void k_sub_reverse_list(uint32_t cap, const uint32_t *__restrict__ n_list, uint32_t *__restrict__ list)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n = min(*n_list, cap);
	if (i >= n / 2)
		return;
	const uint32_t a = list[i];
	list[i] = list[n - 1 - i];
	list[n - 1 - i] = a;
}
// ---- add_concealed, concealed.cpp:925-1196: one wave per flubble on the list
__global__ void __launch_bounds__(64) k_sub_splice_cn(const uint32_t *__restrict__ n_list, const uint32_t *__restrict__ list, const SpliceArgs A)
{
	const SubT &t = A.t;
	const XArrays &X = A.X;
	const uint32_t lane = threadIdx.x, n = *n_list;
	for (uint32_t it = blockIdx.x; it < n; it += gridDim.x) {
		const uint32_t q = list[it], c = A.comp.of_slot(q), q0 = t.doff[c], n0 = t.c_npvst[c], f = q - q0;
		const uint32_t base = t.base_of(c), N = t.c_ntree[c], cn_b = A.cn_off[q0];
		Splice S{X, A.xoff[c], A.ptop + c, A.poff[c + 1], t.err, lane};
		const uint32_t xb = S.xb, pin = A.pin[q], par = f ? t.p_parent[q] : 0u;
		bool got = false;
		if (pin != NIL && par < f) { // pushed by the parent's turn, which came first (a parent has the smaller idx)
			if (!S.push(f, pin))
				return;
			got = true;
		}
		const uint32_t kb = A.cn_off[q], ke = A.cn_off[q + 1];
		if (kb != ke) {
			const uint32_t ai = X.ai[xb + f], zi = X.zi[xb + f], n_of_f = A.mn[2 * (size_t)q + 1];
			const bool is_leaf = f < N && t.nchild[base + f] == 0; // (sic) the SPANNING TREE's vertex f, concealed.cpp:1188
			for (uint32_t k = kb; k < ke; k++) {
				const Slub sl = A.cn[k];
				const uint32_t v = n0 + (k - cn_b); // the k-th slubble of the component becomes its k-th concealed vertex
				if (lane == 0) {
					const uint32_t x = xb + v;
					X.fam[x] = FAM_CONCEALED;
					X.vn[x] = X.vcap[x] = 0;
					X.vbeg[x] = 0;
					X.ai[x] = X.zi[x] = NIL;
					// gen_ai_slubble, concealed.cpp:70-152 / gen_zi_slubble, :154-206
					const bool sl_r = (t.flags[sl.sl] & TF_TYPE_MASK) == 1u, black = (t.flags[sl.sl] & TF_BLACK) != 0;
					uint32_t fl_id;
					uint8_t fl_o;
					const uint32_t sl_id = t.gid[sl.sl];
					X.loc[x] = (uint8_t)sl.loc;
					X.sl[x] = sl.sl;
					if (sl.loc == CL_AI_TRUNK || sl.loc == CL_AI_BRANCH) {
						side_id_or(t, ai, true, fl_id, fl_o);
						const bool fwd_if_r = (sl.loc == CL_AI_TRUNK) == black;
						const uint8_t sl_o = (sl_r == fwd_if_r) ? 0 : 1;
						if (sl_o == 1 && fl_o == 1) {
							X.id1[x] = sl_id, X.or1[x] = 0;
							X.id2[x] = fl_id, X.or2[x] = 0;
						} else {
							X.id1[x] = fl_id, X.or1[x] = fl_o;
							X.id2[x] = sl_id, X.or2[x] = sl_o;
						}
						X.route[x] = 'R';
						if (sl.loc == CL_AI_TRUNK) {
							if (t.is_desc(ai, sl.be_src))
								X.b_up[x] = ai, X.b_lo[x] = sl.be_src;
							else
								X.b_up[x] = sl.be_src, X.b_lo[x] = ai;
						} else {
							X.b_up[x] = sl.sl, X.b_lo[x] = NIL;
						}
					} else {
						side_id_or(t, zi, false, fl_id, fl_o);
						const uint8_t sl_o = (sl_r == black) ? 0 : 1;
						X.id1[x] = sl_id, X.or1[x] = (sl_o == 1 && fl_o == 1) ? 0 : sl_o;
						X.id2[x] = fl_id, X.or2[x] = (sl_o == 1 && fl_o == 1) ? 0 : fl_o;
						X.route[x] = 'L';
						if (t.is_desc(zi, sl.sl))
							X.b_up[x] = zi, X.b_lo[x] = sl.sl;
						else
							X.b_up[x] = sl.sl, X.b_lo[x] = zi;
					}
				}
				S.sync();
				if (!S.push(f, v))
					return;
				got = true;
				if (is_leaf || sl.loc == CL_ZI_BRANCH) // zi_branch: add_conc_zi asks for ai_branch (:1134) and ends in "sl type: unknown"
					continue;
				// the nestings: which of the children (the new vertex among them: it is no flubble) leave for the slubble
				const uint32_t nch = X.vn[xb + f];
				if (!S.filter(f, nch, v, sl.loc == CL_ZI_TRUNK, [&](uint32_t ch) { return cn_leaves(t, X, xb, n0, sl, ai, zi, n_of_f, ch); }))
					return;
			}
		}
		if (pin != NIL && par >= f) { // (never, with the PVST numbered parents first; the order of the reference all the same)
			if (!S.push(f, pin))
				return;
			got = true;
		}
		if (got && lane == 0)
			A.touched[q] = 1; // find_midi looks at it
		S.sync();
	}
}
// ---- find_midi, midi.cpp:225-268 (the branch case is undefined in the reference: nothing comes of it): one wave per
// flubble that got a concealed vertex as a child
__global__ void __launch_bounds__(64) k_sub_midi_find(const uint32_t *__restrict__ n_list, const uint32_t *__restrict__ list, const SpliceArgs A)
{
	const SubT &t = A.t;
	const XArrays &X = A.X;
	const uint32_t lane = threadIdx.x, n = *n_list;
	for (uint32_t it = blockIdx.x; it < n; it += gridDim.x) {
		const uint32_t q = list[it], c = A.comp.of_slot(q), f = q - t.doff[c], xb = A.xoff[c];
		if (X.fam[xb + f] != FAM_FLUBBLE)
			continue;
		uint32_t n_c = 0, n_trunk = 0, trunk[2] = {NIL, NIL};
		const uint32_t zi = X.zi[xb + f], nch = X.vn[xb + f], fb = X.vbeg[xb + f];
		for (uint32_t r0 = 0; r0 < nch; r0 += 64) { // the concealed children, 64 children a round, in order
			const uint32_t r = r0 + lane;
			const uint32_t ch = r < nch ? X.pool[fb + r] : 0u;
			const bool is_c = r < nch && X.fam[xb + ch] == FAM_CONCEALED;
			const bool in_trunk = is_c && X.sl[xb + ch] < zi; // in_trunk, :163-166
			n_c += (uint32_t)__popcll(__ballot(is_c));
			for (unsigned long long m = __ballot(in_trunk); m; m &= m - 1) {
				if (n_trunk < 2)
					trunk[n_trunk] = __shfl(ch, __ffsll((long long)m) - 1);
				n_trunk++;
			}
		}
		if (n_c < 2 || n_trunk != 2)
			continue;
		uint32_t g_idx = NIL, s_idx = NIL;
		for (int k = 0; k < 2; k++) {
			const uint8_t loc = X.loc[xb + trunk[k]];
			if (loc == CL_AI_BRANCH || loc == CL_AI_TRUNK)
				g_idx = trunk[k];
			else
				s_idx = trunk[k];
		}
		if (g_idx == NIL || s_idx == NIL)
			continue;
		// (all midi bubbles are found before the first is added: the pair is remembered in the flubble's spare fields)
		if (lane == 0) {
			X.b_up[xb + f] = g_idx;
			X.b_lo[xb + f] = s_idx;
			A.md[q] = 1;
		}
	}
}
// ---- add_midi, midi.cpp:19-61: the flubbles in ascending idx get the vertices behind the concealed ones
__global__ void __launch_bounds__(64) k_sub_midi_add(const uint32_t *__restrict__ n_list, const uint32_t *__restrict__ list, const SpliceArgs A)
{
	const SubT &t = A.t;
	const XArrays &X = A.X;
	const uint32_t lane = threadIdx.x, n = *n_list;
	for (uint32_t it = blockIdx.x; it < n; it += gridDim.x) {
		const uint32_t q = list[it];
		if (!A.md[q])
			continue;
		const uint32_t c = A.comp.of_slot(q), q0 = t.doff[c], n0 = t.c_npvst[c], f = q - q0, base = t.base_of(c), N = t.c_ntree[c];
		Splice S{X, A.xoff[c], A.ptop + c, A.poff[c + 1], t.err, lane};
		const uint32_t xb = S.xb;
		const uint32_t g_idx = X.b_up[xb + f], s_idx = X.b_lo[xb + f];
		const uint32_t up = min(g_idx, s_idx), lo = max(g_idx, s_idx);
		const uint32_t nch = X.vn[xb + f]; // children before the midi bubble is attached
		const uint32_t v = n0 + (A.cn_off[q0 + n0] - A.cn_off[q0]) + (A.md_ps[q] - A.md_ps[q0]);
		if (lane == 0) {
			const uint32_t x = xb + v;
			X.fam[x] = FAM_MIDI;
			X.vn[x] = X.vcap[x] = 0;
			X.vbeg[x] = 0;
			X.ai[x] = X.zi[x] = X.sl[x] = NIL;
			X.loc[x] = 0;
			// cn_b of a concealed vertex: the second boundary when it was formed with a, the first with z (Concealed::as_str)
			X.id1[x] = X.id2[xb + g_idx], X.or1[x] = X.or2[xb + g_idx];
			X.id2[x] = X.id1[xb + s_idx], X.or2[x] = X.or1[xb + s_idx];
			X.route[x] = 'L';
			X.b_up[x] = up, X.b_lo[x] = lo;
		}
		S.sync();
		// (sic) spanning-tree depths at the PVST indices of the two concealed vertices; past the tree: +infinity
		const uint32_t d_up = up < N ? t.dep(base + up) : 0xFFFFFFFFu, d_lo = lo < N ? t.dep(base + lo) : 0xFFFFFFFFu;
		// the children before the bubble (a copy in the reference) are filtered, then the bubble itself goes behind them
		const bool ok = S.filter(f, nch, v, false, [&](uint32_t ch) {
			return X.fam[xb + ch] == FAM_FLUBBLE && d_up < t.depth[X.ai[xb + ch]] && d_lo > t.depth[X.zi[xb + ch]];
		});
		if (!ok || !S.push(f, v))
			return;
	}
}
// ---- add_smothered, smothered.cpp:349-383: one wave per concealed vertex, its records in search order
__global__ void __launch_bounds__(64) k_sub_smothered(uint32_t NC, const SpliceArgs A)
{
	const SubT &t = A.t;
	const XArrays &X = A.X;
	const uint32_t lane = threadIdx.x;
	for (uint32_t k = blockIdx.x; k < NC; k += gridDim.x) {
		const uint32_t rb = A.smo_off[k], re = A.smo_off[k + 1];
		if (rb == re)
			continue;
		const uint32_t q = A.cn[k].q, c = A.comp.of_slot(q), q0 = t.doff[c], n0 = t.c_npvst[c];
		const uint32_t cn_b = A.cn_off[q0], cn_e = A.cn_off[q0 + n0];
		Splice S{X, A.xoff[c], A.ptop + c, A.poff[c + 1], t.err, lane};
		const uint32_t xb = S.xb;
		const uint32_t cv = n0 + (k - cn_b); // the k-th slubble became the k-th concealed vertex
		const uint32_t v0 = n0 + (cn_e - cn_b) + (A.md_ps[q0 + n0] - A.md_ps[q0]) - A.smo_off[cn_b]; // + r: behind the midi bubbles, in search order
		const bool is_g = A.cn[k].loc == CL_AI_TRUNK || A.cn[k].loc == CL_AI_BRANCH;
		const uint32_t cnb_id = is_g ? X.id2[xb + cv] : X.id1[xb + cv];
		const uint8_t cnb_or = is_g ? X.or2[xb + cv] : X.or1[xb + cv];
		for (uint32_t r = rb; r < re; r++) {
			const Smo m = A.smo[r];
			const uint32_t v = v0 + r;
			if (lane == 0) {
				const uint32_t x = xb + v;
				X.fam[x] = FAM_SMOTHERED;
				X.vn[x] = X.vcap[x] = 0;
				X.vbeg[x] = 0;
				X.ai[x] = X.zi[x] = X.sl[x] = NIL;
				X.loc[x] = 0;
				const uint32_t sm_id = t.gid[m.sm_st];
				const uint8_t sm_or = (t.flags[m.sm_st] & TF_TYPE_MASK) == 0u ? 1 : 0; // comp_e / comp_w: type l -> reverse
				if ((m.flags & 2u) && (m.flags & 1u)) { // Smothered::as_str, pvst.hpp:612-636
					X.id1[x] = cnb_id, X.or1[x] = cnb_or;
					X.id2[x] = sm_id, X.or2[x] = sm_or;
				} else {
					X.id1[x] = sm_id, X.or1[x] = sm_or;
					X.id2[x] = cnb_id, X.or2[x] = cnb_or;
				}
				X.route[x] = (m.flags & 2u) ? 'L' : 'R';
				X.b_up[x] = m.b_up, X.b_lo[x] = m.b_lo;
			}
			S.sync();
			if (!S.push(cv, v))
				return;
			// nest, :332-347: a range-for over children_v[cv] while del_edge erases from it, as libstdc++ runs it: the loop
			// goes to the OLD end, the slots behind the live end hold what erase left there
			const uint32_t old_end = X.vn[xb + cv];
			for (uint32_t i = 0; i < old_end; i++) {
				const uint32_t ch = X.pool[X.vbeg[xb + cv] + i];
				uint32_t c_up, c_lo;
				if (S.fl_like(ch))
					c_up = X.ai[xb + ch], c_lo = X.zi[xb + ch];
				else if (X.fam[xb + ch] == FAM_CONCEALED)
					c_up = X.b_up[xb + ch], c_lo = X.b_lo[xb + ch];
				else
					continue;
				if (c_up == NIL || c_lo == NIL)
					continue;
				if (t.is_desc(m.b_up, c_up) && t.is_desc(c_lo, m.b_lo)) {
					S.erase(cv, ch);
					if (!S.push(v, ch))
						return;
				}
			}
		}
	}
}
__global__ void k_sub_counts(uint32_t C, const SpliceArgs A, uint32_t *__restrict__ counts)
{
	const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= C)
		return;
	const uint32_t n0 = A.t.c_npvst[c], q0 = A.t.doff[c];
	uint32_t n_cn = 0, n_md = 0, n_sm = 0;
	if (n0) {
		const uint32_t cn_b = A.cn_off[q0], cn_e = A.cn_off[q0 + n0];
		n_cn = cn_e - cn_b;
		n_md = A.md_ps[q0 + n0] - A.md_ps[q0];
		n_sm = A.smo_off[cn_e] - A.smo_off[cn_b];
	}
	counts[3 * c] = n_cn, counts[3 * c + 1] = n_md, counts[3 * c + 2] = n_sm;
}
// sizes of the final children lists (one lane per X slot), then the lists themselves into one compact array
__global__ void k_sub_child_counts(uint32_t NX, const uint32_t *__restrict__ xoff, const uint32_t *__restrict__ counts,
				   const uint32_t *__restrict__ c_npvst, const CompAt comp_x, const uint32_t *__restrict__ vn,
				   uint32_t *__restrict__ out)
{
	const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x > NX)
		return;
	uint32_t n = 0;
	if (x < NX) {
		const uint32_t c = comp_x.of_slot(x); // (doff = xoff here)
		const uint32_t nt = c_npvst[c] ? c_npvst[c] + counts[3 * c] + counts[3 * c + 1] + counts[3 * c + 2] : 0;
		if (x - xoff[c] < nt)
			n = vn[x];
	}
	out[x] = n;
}
// one lane per child entry (a chromosome's root has a million children: one lane per LIST took 0.1 s): the list that owns
// output slot i is the last vertex whose offset is <= i
__global__ void k_sub_child_gather(uint32_t NCH, uint32_t NX, const uint32_t *__restrict__ coff, const uint32_t *__restrict__ vbeg,
				   const uint32_t *__restrict__ pool, uint32_t *__restrict__ out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= NCH)
		return;
	const uint32_t x = span_of(coff, NX, i);
	out[i] = pool[vbeg[x] + (i - coff[x])];
}
// the vertices of every component without the spare slots of X-space: dense slot d = dvoff[c] + (index inside the component)
__global__ void k_sub_compact(uint32_t NV, uint32_t C, const uint32_t *__restrict__ dvoff, const uint32_t *__restrict__ xoff, const XArrays X,
			      const uint32_t *__restrict__ coff, uint8_t *__restrict__ fam, uint8_t *__restrict__ or1, uint8_t *__restrict__ or2,
			      uint8_t *__restrict__ route, uint32_t *__restrict__ id1, uint32_t *__restrict__ id2, uint32_t *__restrict__ coff_d)
{
	const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
	if (d >= NV)
		return;
	const uint32_t c = span_of(dvoff, C, d); // (components without a PVST own no slot)
	const uint32_t x = xoff[c] + (d - dvoff[c]);
	fam[d] = X.fam[x], or1[d] = X.or1[x], or2[d] = X.or2[x], route[d] = X.route[x];
	id1[d] = X.id1[x], id2[d] = X.id2[x];
	coff_d[d] = coff[x];
}

// ------------------------------------------------------------------ the driver: switches, phase layouts, named steps
// The test and debug switches of the stage, read from the environment at the top of EVERY call (the tests change them between
// two passes on one context).
struct SubSwitches {
	// POVU_HIP_SUB_SERIAL_SPLICE=forward|reverse (tests): X-space filled with a stale forest first, and the splice kernels on
	// one wave that walks its list in order (reverse: children before their parents) -- the schedule the parallel splice
	// must not depend on
	enum { SPLICE_PARALLEL, SPLICE_FORWARD, SPLICE_REVERSE } sched = SPLICE_PARALLEL;
	bool times = false;	  // POVU_HIP_SUB_TIMES=1: wall-clock of the phases on stderr (each mark synchronises the stream)
	bool literal_loa = false; // POVU_HIP_SUB_LITERAL_LOA (tests): the reference's heap on every component, whatever its edges
	bool forbid_heap = false; // POVU_HIP_SUB_FORBID_HEAP (tests): fail when any component would take the one-lane heap
	static SubSwitches from_env()
	{
		SubSwitches o;
		if (const char *e = getenv("POVU_HIP_SUB_SERIAL_SPLICE"); e && *e) {
			if (!strcmp(e, "forward"))
				o.sched = SPLICE_FORWARD;
			else if (!strcmp(e, "reverse"))
				o.sched = SPLICE_REVERSE;
			else
				throw HipError(std::string("POVU_HIP_SUB_SERIAL_SPLICE: forward or reverse, not ") + e);
		}
		o.times = getenv("POVU_HIP_SUB_TIMES") != nullptr;
		o.literal_loa = getenv("POVU_HIP_SUB_LITERAL_LOA") != nullptr;
		o.forbid_heap = getenv("POVU_HIP_SUB_FORBID_HEAP") != nullptr;
		return o;
	}
};
struct PhaseTimer {
	bool on;
	hipStream_t s;
	double t_prev = now();
	static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
	void mark(const char *what)
	{
		if (!on)
			return;
		HIP_CHECK(hipStreamSynchronize(s));
		const double t_now = now();
		fprintf(stderr, "[subflubbles] %-22s %9.1f ms\n", what, t_now - t_prev);
		t_prev = t_now;
	}
};

// The device tables of the stage.  Their sizes become known at six points of the pass, so there are six layouts, each
// declared once (measured, then carved into an arena of its own: SubArenas) when its sizes are there.  Every span carries 16
// entries more than its user asks for, kept from before (the allocator this replaced added them to every table); what a
// kernel or a scan needs beyond the plain count is said at the span, any other surplus is kept from before as well.
struct SubSizes {
	size_t T, NB0, NB, Q, C;		// (a) at entry: tree vertices, ordinary / all back edges, dense PVST slots, components
	size_t NC = 0, NS = 0;			// (b), (c) concealed and smothered records, from the scans of their counts
	size_t NX = 0, ps = 0, NCH = 0, NV = 0; // (d) X slots and pool entries, (e) children, (f) vertices of the result
};
// (a) sized by T, NB0, NB, Q, C: the tables the searches ask (SubT points into them) and the concealed counts
struct SubTables {
	void *scan; // scratch of every scan over T, NB or Q entries
	size_t scan_bytes;
	uint32_t *err;
	uint32_t *depth, *hi0, *eat;
	uint32_t *ocnt, *icnt, *o_off, *i_off, *o_adj, *i_adj;
	uint32_t *segH, *segD, *segT; // trees of the segment trees over hi0, depth, tgt_s
	uint32_t *simp_ps, *hi, *lo, *br_cnt;
	unsigned long long *ekey;
	uint32_t *wbefore, *wtail;
	uint32_t *heap, *has_self, *mx;
	uint32_t *tgt_s, *slot_s;
	uint32_t *cn_cnt, *cn_off, *mn;
};
void tables_spans(SubTables &t, const SubSizes &n, Spans &take)
{
	t.scan_bytes = scan_tmp_bytes(std::max(std::max(n.T, n.NB), n.Q) + 8);
	take(t.scan_bytes + 16, t.scan);
	take(4 + 16, t.err); // four words are cleared, the E_ bits are read from word 0
	take(n.T + 16 + 16, t.depth, t.hi0, t.eat); // T + 1 entries (k_sub_depth_hi0); the segment trees over depth and hi0 read whole blocks of 16
	take(n.T + 2 + 16, t.ocnt, t.icnt, t.o_off, t.i_off); // scanned over T + 1 entries, cleared over T + 2
	take(n.NB + 1 + 16, t.o_adj, t.i_adj);
	take(SegTree::tree_words(n.T + 1) + 16 + 16, t.segH, t.segD);
	take(n.T + 4 + 16, t.simp_ps, t.hi, t.lo, t.br_cnt); // simp_ps, br_cnt: T + 1 entries (scan, k_sub_br_counts)
	take(n.NB0 + 2 + 16, t.ekey);
	take(n.T + 8 + 16, t.wbefore, t.wtail); // cleared over T + 8.  wtail: edge_id_weights writes it, nobody here reads it
	take(n.NB0 + 4 + 16, t.heap);
	take(n.C + 4 + 16, t.has_self); // cleared over C + 4
	take(2 * (size_t)SegTree::pow2(n.T + 1) + 4 + 16, t.mx); // max-tree with pow2(T + 1) leaves, cleared with 4 words more
	take(n.NB0 + 32 + 16, t.tgt_s, t.slot_s); // tgt_s: the segment tree over it reads whole blocks of 16
	take(SegTree::tree_words(n.NB0 + 1) + 16 + 16, t.segT);
	take(n.Q + 4 + 16, t.cn_cnt, t.cn_off); // Q + 1 entries: launch and scan over Q + 1
	take(2 * n.Q + 4 + 16, t.mn);
}
// (b) sized by NC: the concealed records and the smothered counts, one per record
struct SubConcealed {
	Slub *cn;
	uint32_t *sm_cnt, *sm_off;
};
void concealed_spans(SubConcealed &t, const SubSizes &n, Spans &take)
{
	take(n.NC + 1 + 16, t.cn);
	take(n.NC + 4 + 16, t.sm_cnt, t.sm_off); // NC + 1 entries: launch and scan over NC + 1
}
// (c) sized by NS: the smothered records; with them the three counts a component the host lays the splice out by
struct SubSmothered {
	Smo *smo;
	uint32_t *comp_counts;
};
void smothered_spans(SubSmothered &t, const SubSizes &n, Spans &take)
{
	take(n.NS + 1 + 16, t.smo);
	take(3 * n.C + 4 + 16, t.comp_counts);
}
// (d) sized by NX and ps (and Q, C): X-space with its pool of children vectors, the sort that seeds the vectors, the
// scratch of the splice and the children counts.  What only a pass with C && Q uses (ptop .. ctmp) is carved with the rest:
// a few bytes per PVST slot.
struct SubXspace {
	uint32_t *xoff, *poff; // [C + 1]
	XArrays X;
	uint32_t *cap_ps;
	void *scan; // scratch of the scan over NX entries
	size_t scan_bytes;
	uint32_t *k0, *k1, *v0, *v1;
	void *sort;
	size_t sort_bytes;
	uint32_t *counts; // [3 C] concealed, midi, smothered vertices per component
	uint32_t *ptop, *pin, *md_ps, *list, *n_list;
	uint8_t *act, *touched, *md;
	void *ctmp;
	size_t ctmp_bytes;
	uint32_t *ccnt, *coff;
};
void xspace_spans(SubXspace &t, const SubSizes &n, Spans &take)
{
	XArrays &X = t.X;
	take(n.C + 2 + 16, t.xoff, t.poff);
	take(n.NX + 4 + 16, X.fam, X.or1, X.or2, X.route, X.loc);
	take(n.NX + 4 + 16, X.id1, X.id2, X.ai, X.zi, X.sl, X.b_up, X.b_lo, X.vbeg, X.vn, X.vcap); // vn, vcap: cleared over NX + 4
	take(n.ps + 4 + 16, X.pool);
	take(n.NX + 4 + 16, t.cap_ps, t.ccnt, t.coff); // ccnt, coff: NX + 1 entries (launch and scan over NX + 1)
	t.scan_bytes = scan_tmp_bytes(n.NX + 8);
	take(t.scan_bytes + 16, t.scan);
	take(n.Q + 4 + 16, t.k0, t.k1, t.v0, t.v1, t.pin);
	t.sort_bytes = sort_tmp_bytes(n.Q + 8);
	take(t.sort_bytes + 16, t.sort);
	take(3 * n.C + 4 + 16, t.counts);
	take(n.C + 4 + 16, t.ptop);
	take(n.Q + 16 + 16, t.act, t.touched, t.md); // md: Q + 1 entries, md[Q] is cleared for the scan over Q + 1
	take(n.Q + 8 + 16, t.md_ps, t.list);	     // md_ps: Q + 1 entries
	take(8 + 16, t.n_list);
	t.ctmp_bytes = compact_tmp_bytes(n.Q + 8);
	take(t.ctmp_bytes + 16, t.ctmp);
}
// (e) sized by NCH: the children lists, compact
struct SubChildren {
	uint32_t *child;
};
void children_spans(SubChildren &t, const SubSizes &n, Spans &take) { take(n.NCH + 4 + 16, t.child); }
// (f) sized by NV: the vertices without the spare slots of X-space, as they go to the host
struct SubOut {
	uint32_t *dvoff; // [C + 1]
	uint8_t *fam, *or1, *or2, *route;
	uint32_t *id1, *id2, *coff;
};
void out_spans(SubOut &t, const SubSizes &n, Spans &take)
{
	take(n.C + 2 + 16, t.dvoff);
	take(n.NV + 4 + 16, t.fam, t.or1, t.or2, t.route);
	take(n.NV + 4 + 16, t.id1, t.id2, t.coff);
}

// One pass of the stage: the inputs, the sizes as they become known, the phase tables, the view the kernels take (SubT).
// The steps run in the order of run_subflubbles below, all on the stream s.
struct SubPass {
	const CompState &cs;
	const SeqWs &sw;
	const ParWs &pw;
	const TreeWs &tw;
	const LeafState &ls;
	const LeafIn &in;
	HostScratch &host;
	SubArenas &ar;
	hipStream_t s;
	const SubSwitches opt;
	PhaseTimer timer;
	SubSizes n;
	const uint32_t T, NB0, NB, Q, C; // (n's entry sizes as the kernels take them)
	uint32_t NC = 0, NS = 0, NX = 0, NCH = 0;
	SubTables tb{};
	SubConcealed cn{};
	SubSmothered sm{};
	SubXspace xs{};
	SubChildren ch{};
	SubOut o{};
	SubT t{};
	CompAt comp{}, comp_x{};	    // component of a dense PVST slot / of an X slot
	uint32_t *h_cc = nullptr; // [3 C] page-locked: PVST vertices, concealed and smothered records per component

	SubPass(const CompState &cs_, const SeqWs &sw_, const ParWs &pw_, const TreeWs &tw_, const LeafState &ls_, uint32_t C_, HostScratch &host_,
		SubArenas &ar_, hipStream_t s_)
	    : cs(cs_), sw(sw_), pw(pw_), tw(tw_), ls(ls_), in(ls_.in), host(host_), ar(ar_), s(s_), opt(SubSwitches::from_env()),
	      timer{opt.times, s_}, T(2 * sw_.V + C_), NB0(pw_.nb0), NB(pw_.nb0 + pw_.ncap + pw_.nsimp), Q((uint32_t)pw_.d_total), C(C_)
	{
		n.T = T, n.NB0 = NB0, n.NB = NB, n.Q = Q, n.C = C;
		comp = CompAt{cs.voff, pw.doff, C};
	}

	// carves (a).  Writes depth, hi0 -> segH, segD; the back edges by source and by target (o_off / o_adj, i_off / i_adj), eat
	// = first slot of a vertex's ordinary edges; hi.  Reads the tree stage's sizes and depths, the dense edge list, in.simp.
	void edge_tables_hi()
	{
		carve(ar.tables, [&](Spans &take) { tables_spans(tb, n, take); });
		HIP_CHECK(hipMemsetAsync(tb.err, 0, 16, s));
		LAUNCH(k_sub_depth_hi0, (size_t)T + 1, s, T, sw.t_size, sw.t_depth, tb.depth, tb.hi0, tb.eat);
		HIP_CHECK(hipMemsetAsync(tb.ocnt, 0, ((size_t)T + 2) * 4, s));
		HIP_CHECK(hipMemsetAsync(tb.icnt, 0, ((size_t)T + 2) * 4, s));
		LAUNCH(k_sub_edge_counts, NB, s, NB, NB0, pw.b_src, pw.b_tgt, pw.b_ord, tb.ocnt, tb.icnt, tb.hi0, tb.eat);
		scan_exclusive_u32(tb.ocnt, tb.o_off, (size_t)T + 1, tb.scan, tb.scan_bytes, s);
		scan_exclusive_u32(tb.icnt, tb.i_off, (size_t)T + 1, tb.scan, tb.scan_bytes, s);
		HIP_CHECK(hipMemsetAsync(tb.ocnt, 0, ((size_t)T + 2) * 4, s));
		HIP_CHECK(hipMemsetAsync(tb.icnt, 0, ((size_t)T + 2) * 4, s));
		LAUNCH(k_sub_edge_fill, NB, s, NB, pw.b_src, pw.b_tgt, tb.o_off, tb.i_off, tb.ocnt, tb.icnt, tb.o_adj, tb.i_adj);
		// (the rows are in whatever order the atomics came: every question asked of them is about a set -- any, count, deepest --
		// and sorting them cost 0.6 s on a segment with 2*10^5 links, one lane on its row)
		SegTree segH;
		segH.tree = tb.segH;
		t.segD.tree = tb.segD;
		seg_build(segH, tb.hi0, (size_t)T + 1, s);
		seg_build(t.segD, tb.depth, (size_t)T + 1, s);
		scan_exclusive_u8(in.simp, tb.simp_ps, (size_t)T + 1, nullptr, nullptr, 0, tb.scan, tb.scan_bytes, s);
		LAUNCH(k_sub_hi, T, s, T, sw.t_size, segH, tb.simp_ps, comp, tb.hi);
		timer.mark("edge tables, hi");
	}
	// Writes ekey (the creation keys of the ordinary edges) and lo (LoA: closed form from the max-tree mx, the reference's
	// heap where has_self says so).  Reads eat, depth, the tree stage's state (edge_id_weights), in.out_ord / nself / O.
	void creation_keys_lo()
	{
		HIP_CHECK(hipMemsetAsync(tb.wbefore, 0, ((size_t)T + 8) * 4, s));
		HIP_CHECK(hipMemsetAsync(tb.wtail, 0, ((size_t)T + 8) * 4, s));
		edge_id_weights(cs, sw, tw, tb.wbefore, tb.wtail, s);
		LAUNCH(k_sub_edge_keys, T, s, T, sw.t_size, in.out_ord, tb.eat, tb.wbefore, tb.ekey);
		const uint32_t P2 = SegTree::pow2((size_t)T + 1);
		HIP_CHECK(hipMemsetAsync(tb.mx, 0, (2 * (size_t)P2 + 4) * 4, s));
		HIP_CHECK(hipMemsetAsync(tb.has_self, 0, ((size_t)C + 4) * 4, s));
		LAUNCH(k_sub_lo_mark, NB0, s, NB0, pw.b_src, pw.b_tgt, P2, tb.mx);
		LAUNCH(k_sub_lo_query, T, s, T, sw.t_size, P2, tb.mx, in.nself, comp, tb.lo, tb.has_self);
		if (opt.literal_loa)
			fill_u32(tb.has_self, C, 1u, s);
		if (opt.forbid_heap) {
			uint32_t *hs = host.take<uint32_t>(C);
			HIP_CHECK(copy_async(hs, tb.has_self, (size_t)C * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipStreamSynchronize(s));
			for (uint32_t c = 0; c < C; c++)
				if (hs[c])
					throw HipError("subflubble passes: component " + std::to_string(c + 1) + " takes the literal LoA heap (POVU_HIP_SUB_FORBID_HEAP is set)");
		}
		LAUNCH(k_sub_lo, C, s, C, cs.voff, sw.c_ntree, sw.t_size, tb.depth, in.out_ord, tb.eat, pw.b_tgt, in.O, tb.has_self, tb.heap, tb.lo);
		timer.mark("creation keys, lo");
	}
	// Writes br_cnt (closed form) and the ordinary edges in source order (tgt_s, slot_s) -> segT.  Reads eat, in.gp / P / O.
	void bracket_rows()
	{
		LAUNCH(k_sub_br_counts, (size_t)T + 1, s, T, sw.t_size, in.gp, in.P, in.out_ord, in.nself, tb.br_cnt);
		LAUNCH(k_sub_edges_by_source, T, s, T, sw.t_size, in.out_ord, tb.eat, in.O, pw.b_tgt, tb.tgt_s, tb.slot_s);
		t.segT.tree = tb.segT;
		seg_build(t.segT, tb.tgt_s, NB0, s);
		timer.mark("bracket rows");
	}
	// the view of (a) and of the dense PVST that every later kernel takes (segD and segT were built in place above)
	void fill_view()
	{
		t.T = T, t.C = C, t.NB0 = NB0, t.NB = NB;
		t.voff = cs.voff, t.c_ntree = sw.c_ntree, t.doff = pw.doff, t.c_npvst = sw.c_npvst;
		t.size = sw.t_size, t.gp = in.gp, t.nchild = in.nchild, t.depth = tb.depth, t.gid = sw.t_gid, t.flags = sw.t_flags;
		t.b_src = pw.b_src, t.b_tgt = pw.b_tgt, t.b_ord = pw.b_ord;
		t.o_off = tb.o_off, t.o_adj = tb.o_adj, t.i_off = tb.i_off, t.i_adj = tb.i_adj;
		t.br_cnt = tb.br_cnt, t.O = in.O, t.slot_s = tb.slot_s, t.lo = tb.lo, t.hi = tb.hi, t.ekey = tb.ekey;
		t.p_ai = ls.dense.ai, t.p_zi = ls.dense.zi, t.p_fam = ls.dense.fam;
		t.p_parent = pw.d_parent, t.p_a = pw.d_a, t.p_z = pw.d_z, t.p_aor = pw.d_aor, t.p_zor = pw.d_zor;
		t.err = tb.err;
	}
	// find_concealed: count per dense slot (cn_cnt, mn), scan (cn_off), NC to the host, carves (b), emit (cn)
	void search_concealed()
	{
		LAUNCH(k_sub_cn_count, (size_t)Q + 1, s, Q, t, comp, tb.cn_cnt, tb.mn);
		scan_exclusive_u32(tb.cn_cnt, tb.cn_off, (size_t)Q + 1, tb.scan, tb.scan_bytes, s);
		n.NC = NC = host.read_u32(tb.cn_off + Q, s);
		carve(ar.concealed, [&](Spans &take) { concealed_spans(cn, n, take); });
		LAUNCH(k_sub_cn_emit, Q, s, Q, t, comp, tb.cn_off, cn.cn);
		timer.mark("find_concealed search");
	}
	// find_smothered: count per concealed record (sm_cnt), scan (sm_off), NS to the host, carves (c), emit (smo)
	void search_smothered()
	{
		LAUNCH(k_sub_smo_count, (size_t)NC + 1, s, NC, t, comp, cn.cn, cn.sm_cnt);
		scan_exclusive_u32(cn.sm_cnt, cn.sm_off, (size_t)NC + 1, tb.scan, tb.scan_bytes, s);
		n.NS = NS = host.read_u32(cn.sm_off + NC, s);
		carve(ar.smothered, [&](Spans &take) { smothered_spans(sm, n, take); });
		LAUNCH(k_sub_smo_emit, NC, s, NC, t, comp, cn.cn, cn.sm_off, sm.smo);
		timer.mark("find_smothered search");
	}
	// Layout of the splice: per component its stretch of X-space and of the vector pool.  The host needs three numbers a
	// component (PVST vertices, concealed and smothered records: h_cc), worked out on the device and read through page-locked
	// scratch (the whole offset array of the records, 4 bytes per PVST vertex into a pageable vector, took 5 - 20 ms on the
	// whole-genome workload).  Gives NX and ps, carves (d), uploads xoff and poff.
	void layout_splice()
	{
		h_cc = host.take<uint32_t>(3 * (size_t)C + 4);
		if (C) {
			LAUNCH(k_sub_comp_counts, C, s, C, pw.doff, sw.c_npvst, tb.cn_off, cn.sm_off, sm.comp_counts);
			HIP_CHECK(copy_async(h_cc, sm.comp_counts, 3 * (size_t)C * 4, hipMemcpyDeviceToHost, s));
		}
		HIP_CHECK(hipStreamSynchronize(s));
		uint32_t *h_xoff = host.take<uint32_t>((size_t)C + 1), *h_poff = host.take<uint32_t>((size_t)C + 1);
		uint64_t x = 0, p = 0;
		for (uint32_t c = 0; c < C; c++) {
			h_xoff[c] = (uint32_t)x;
			h_poff[c] = (uint32_t)p;
			if (const uint64_t n0 = h_cc[3 * (size_t)c]) {
				const uint64_t ncn = h_cc[3 * (size_t)c + 1], nsm = h_cc[3 * (size_t)c + 2];
				x += 2 * n0 + ncn + nsm;
				p += 32 * n0 + 16 * (ncn + nsm) + 256;
			}
			if (x > 0xFFFFFFF0ull || p > 0xFFFFFFF0ull)
				throw HipError("subflubble passes: more than 2^32 PVST vertices or child slots in one pass");
		}
		h_xoff[C] = (uint32_t)x;
		h_poff[C] = (uint32_t)p;
		n.NX = NX = (uint32_t)x;
		n.ps = p;
		carve(ar.xspace, [&](Spans &take) { xspace_spans(xs, n, take); });
		HIP_CHECK(copy_async(xs.xoff, h_xoff, ((size_t)C + 1) * 4, hipMemcpyHostToDevice, s));
		HIP_CHECK(copy_async(xs.poff, h_poff, ((size_t)C + 1) * 4, hipMemcpyHostToDevice, s));
		comp_x = CompAt{cs.voff, xs.xoff, C};
	}
	// The PVST of find_flubbles into X-space: the fields of every vertex (k_sub_x_init; under a serial schedule a stale forest
	// in every slot first) and its children vector in ascending idx, by a sort of (X slot of the parent, child).
	void seed_vectors()
	{
		const XArrays &X = xs.X;
		HIP_CHECK(hipMemsetAsync(X.vn, 0, ((size_t)NX + 4) * 4, s));
		HIP_CHECK(hipMemsetAsync(X.vcap, 0, ((size_t)NX + 4) * 4, s));
		if (opt.sched != SubSwitches::SPLICE_PARALLEL)
			LAUNCH(k_sub_x_poison, NX, s, NX, t, comp_x, xs.xoff, X);
		LAUNCH(k_sub_x_init, Q, s, Q, t, comp, xs.xoff, X);
		LAUNCH(k_sub_x_keys, Q, s, Q, NX, t, comp, xs.xoff, xs.k0, xs.v0);
		sort_pairs_u32(xs.k0, xs.k1, xs.v0, xs.v1, Q, bits_for(NX), xs.sort, xs.sort_bytes, s);
		LAUNCH(k_sub_x_vbeg, Q, s, Q, t, comp, xs.xoff, xs.poff, xs.k1, xs.cap_ps, X);
		LAUNCH(k_sub_x_place, Q, s, Q, NX, xs.k1, xs.v1, xs.cap_ps, X);
		timer.mark("layout, PVST vectors");
	}
	// add_concealed, find_midi / add_midi, add_smothered on X-space, one wave per listed flubble (one wave in all under a serial
	// schedule); writes counts = inserted vertices per component and kind.  Reads the records (cn, mn, smo) and the view.
	void splice()
	{
		if (C && Q) {
			SpliceArgs A{};
			A.t = t, A.comp = comp, A.xoff = xs.xoff, A.poff = xs.poff, A.ptop = xs.ptop;
			A.cn_off = tb.cn_off, A.cn = cn.cn, A.mn = tb.mn, A.smo_off = cn.sm_off, A.smo = sm.smo, A.X = xs.X;
			A.pin = xs.pin, A.act = xs.act, A.touched = xs.touched, A.md = xs.md, A.md_ps = xs.md_ps;
			uint32_t *list = xs.list, *n_list = xs.n_list;
			LAUNCH(k_sub_ptop, C, s, C, xs.poff, sw.c_npvst, A.ptop);
			LAUNCH(k_sub_pin, Q, s, Q, A);
			const bool reverse = opt.sched == SubSwitches::SPLICE_REVERSE;
			const unsigned waves = opt.sched == SubSwitches::SPLICE_PARALLEL ? SPLICE_WAVES : 1u;
			compact_flagged_u8(A.act, Q, list, n_list, xs.ctmp, xs.ctmp_bytes, s);
			if (reverse)
				LAUNCH(k_sub_reverse_list, Q / 2 + 1, s, Q, n_list, list);
			KLAUNCH(k_sub_splice_cn, dim3(waves), dim3(64), 0, s, n_list, list, A);
			compact_flagged_u8(A.touched, Q, list, n_list, xs.ctmp, xs.ctmp_bytes, s);
			if (reverse)
				LAUNCH(k_sub_reverse_list, Q / 2 + 1, s, Q, n_list, list);
			KLAUNCH(k_sub_midi_find, dim3(waves), dim3(64), 0, s, n_list, list, A);
			HIP_CHECK(hipMemsetAsync(A.md + Q, 0, 1, s));
			scan_exclusive_u8(A.md, xs.md_ps, (size_t)Q + 1, nullptr, nullptr, 0, tb.scan, tb.scan_bytes, s);
			KLAUNCH(k_sub_midi_add, dim3(waves), dim3(64), 0, s, n_list, list, A);
			if (NS)
				KLAUNCH(k_sub_smothered, dim3(std::min<unsigned>(NC, waves)), dim3(64), 0, s, NC, A);
			LAUNCH(k_sub_counts, C, s, C, A, xs.counts);
		} else if (C) {
			HIP_CHECK(hipMemsetAsync(xs.counts, 0, 3 * (size_t)C * 4, s));
		}
		timer.mark("splice");
		ar.pool_off = xs.poff, ar.pool_top = C && Q ? xs.ptop : nullptr, ar.pool_comps = C;
		const uint32_t e = host.read_u32(tb.err, s);
		if (e & E_POOL)
			throw HipError("subflubble passes: the children vectors outgrew their pool (internal sizing bug)");
		if (e & E_LAYOUT)
			throw HipError("subflubble passes: more inserted vertices than the layout has room for (internal sizing bug)");
	}
	// The final children lists, compact and in vertex order: sizes per X slot (ccnt), scan (coff), NCH to the host, carves (e),
	// gather (child).
	void compact_children()
	{
		LAUNCH(k_sub_child_counts, (size_t)NX + 1, s, NX, xs.xoff, xs.counts, sw.c_npvst, comp_x, xs.X.vn, xs.ccnt);
		scan_exclusive_u32(xs.ccnt, xs.coff, (size_t)NX + 1, xs.scan, xs.scan_bytes, s);
		n.NCH = NCH = host.read_u32(xs.coff + NX, s);
		carve(ar.children, [&](Spans &take) { children_spans(ch, n, take); });
		LAUNCH(k_sub_child_gather, NCH, s, NCH, NX, xs.coff, xs.X.vbeg, xs.X.pool, ch.child);
		timer.mark("children lists");
	}
	// To the host: counts gives the vertices of every component (out.voff, NV), carves (f); the vertices are compacted on the
	// device (X-space has spare slots behind every component), then one copy per array into one page-locked block of `pool`.
	void to_host(SubForest &out, const std::shared_ptr<::PinnedPool> &pool)
	{
		uint32_t *h_counts = host.take<uint32_t>(3 * (size_t)C), *h_dvoff = host.take<uint32_t>((size_t)C + 1);
		if (C)
			HIP_CHECK(copy_async(h_counts, xs.counts, 3 * (size_t)C * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		out.voff.assign((size_t)C + 1, 0);
		uint64_t n_vtx = 0;
		for (uint32_t c = 0; c < C; c++) {
			out.voff[c] = n_vtx;
			h_dvoff[c] = (uint32_t)n_vtx;
			if (const uint32_t n0 = h_cc[3 * (size_t)c])
				n_vtx += (uint64_t)n0 + h_counts[3 * c] + h_counts[3 * c + 1] + h_counts[3 * c + 2];
		}
		out.voff[C] = n_vtx;
		h_dvoff[C] = (uint32_t)n_vtx;
		out.counts.assign(h_counts, h_counts + 3 * (size_t)C);
		const uint32_t NV = (uint32_t)n_vtx;
		n.NV = NV;
		carve(ar.out, [&](Spans &take) { out_spans(o, n, take); });
		HIP_CHECK(copy_async(o.dvoff, h_dvoff, ((size_t)C + 1) * 4, hipMemcpyHostToDevice, s));
		LAUNCH(k_sub_compact, NV, s, NV, C, o.dvoff, xs.xoff, xs.X, xs.coff, o.fam, o.or1, o.or2, o.route, o.id1, o.id2, o.coff);
		// one page-locked block: fam | or1 | or2 | route | id1 | id2 | coff (+ 1) | child, one spare entry each
		const forest_wire::SubBlockLayout L(NV, NCH, 0, 1);
		if (!pool)
			throw HipError("subflubble passes: no pool of page-locked memory (internal)");
		out.pool = pool;
		out.blk = pool->get(L.end + 64, out.blk_cap, &out.blk_seg);
		char *hb = static_cast<char *>(out.blk);
		auto d2h = [&](size_t at, const void *src, size_t bytes) {
			if (bytes)
				HIP_CHECK(copy_async(hb + at, src, bytes, hipMemcpyDeviceToHost, s));
		};
		d2h(L.fam, o.fam, NV);
		d2h(L.or1, o.or1, NV);
		d2h(L.or2, o.or2, NV);
		d2h(L.route, o.route, NV);
		d2h(L.id1, o.id1, (size_t)NV * 4);
		d2h(L.id2, o.id2, (size_t)NV * 4);
		d2h(L.coff, o.coff, (size_t)NV * 4);
		d2h(L.child, ch.child, (size_t)NCH * 4); // (the lists are compact already, in vertex order)
		HIP_CHECK(hipStreamSynchronize(s));
		reinterpret_cast<uint32_t *>(hb + L.coff)[NV] = NCH;
		out.n_vtx = n_vtx, out.n_child = NCH;
		out.point(hb, L);
		timer.mark("to the host");
	}
};
} // namespace

SubForest::~SubForest()
{
	if (blk && pool)
		pool->put(blk, blk_cap, blk_seg);
}

void SubArenas::release()
{
	for_each_arena([](const char *, Arena &a) { a.release(); });
	pool_off = pool_top = nullptr;
	pool_comps = 0;
}
size_t SubArenas::capacity() const
{
	size_t bytes = 0;
	for_each_arena([&](const char *, const Arena &a) { bytes += a.capacity(); });
	return bytes;
}

void run_subflubbles(const CompState &cs, const SeqWs &sw, const ParWs &pw, const TreeWs &tw, const LeafState &ls, uint32_t C,
		     HostScratch &host, SubForest &out, const std::shared_ptr<::PinnedPool> &pool, hipStream_t s, SubArenas &arenas)
{
	SubPass p(cs, sw, pw, tw, ls, C, host, arenas, s);
	arenas.pool_off = arenas.pool_top = nullptr; // (until this pass has spliced)
	arenas.pool_comps = 0;
	p.edge_tables_hi();
	p.creation_keys_lo();
	p.bracket_rows();
	p.fill_view();
	p.search_concealed();
	p.search_smothered();
	p.layout_splice();
	p.seed_vectors();
	p.splice();
	p.compact_children();
	p.to_host(out, pool);
	if (p.opt.times)
		fprintf(stderr, "[subflubbles] %-22s %9.1f MiB\n", "phase arenas", (double)arenas.capacity() / (1 << 20));
}

} // namespace povu_hip
