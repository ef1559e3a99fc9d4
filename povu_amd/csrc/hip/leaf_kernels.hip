// leaf_kernels.hip -- the two relabelling passes of `povu decompose -s` on the state of an all-parallel pass.
//
// The reference runs five passes after find_flubbles when -s is given (app/subcommand/decompose.cpp:63-70).  The first
// two only relabel LEAF flubbles of the PVST (their line letter becomes T or O): find_tiny (src/povu/algorithms/
// tiny.cpp:100-129) and find_parallel (src/povu/algorithms/parallel.cpp:263-287).  Both ask questions about the
// spanning tree around a flubble's inner boundary vertices ai / zi (compute_ai_zi, flubbles.cpp:264-290) and about
// gen_tree_meta's bracket table (src/povu/graph/tree_utils.cpp:531-690): for a tree vertex c, the back edges of type
// back_edge that start strictly below c and end strictly above it.  The reference materialises that table per vertex
// (quadratic on deep trees); here every question has a closed form over pre-order intervals [v, v + size(v)):
//
//   |brackets(c)|         = sum over subtree(c) of (ordinary edges leaving - arriving) - those leaving c itself
//   a bracket of c ends at ai, for the only c that is ever asked (one descendant, c+1)
//                         = an ordinary back edge of c+1 ends at ai                       (two flag bytes per vertex)
//   back-edge INDEX of an edge of OBE(c) equals ai  (sic: tiny.cpp:52-56 compares indices with a vertex)
//                         : from_bd creates the ordinary edges of such a c right after those of c+1, so their indices
//                           are a RANGE that starts at (back edges created before c was discovered) + |OBE(c+1)|; the
//                           simplifying edge of c has index n_be0 + (capping / simplifying edges of later vertices)
//   child counts, |OBE|, |IBE| by type: atomics over the dense edge list.
//
// Undefined behaviour of the reference that the oracle DEFINES and this file follows (oracle/povu_oracle.c, "leaf
// subflubble passes"): in_branch without a gray child of zi answers "no"; a back edge whose source is its target is in
// no bracket table.  The three inserting passes (concealed, midi, smothered) run after these two: sub_kernels.hip.
// PARITY UNPINNED: the reference holds no T or O line anywhere; tests compare with the oracle's literal restatement.
#include "leaf_kernels.hpp"

namespace povu_hip
{

#define NIL POVU_NIL

// (component of a tree vertex, of a slot of the one-lane layout: CompSpans, common.hpp)

// global parent and child counts
__global__ void k_leaf_tree(uint32_t T, const uint32_t *__restrict__ t_size, const uint32_t *__restrict__ t_par, const CompSpans comp,
			    uint32_t *__restrict__ gp, uint32_t *__restrict__ nchild)
{
	uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= T)
		return;
	uint32_t g = NIL;
	if (t_size[t] && t_par[t] != NIL) {
		const uint32_t c = comp.of_tree(t);
		g = 2 * comp.voff[c] + c + t_par[t];
		atomicAdd(&nchild[g], 1u);
	}
	gp[t] = g;
}

// counts per tree vertex over the dense edge list: [0, NB0) ordinary, [NB0, NB0 + ncap) capping, the rest simplifying
__global__ void k_leaf_edges(uint32_t NB, uint32_t NB0, uint32_t ncap, const uint32_t *__restrict__ b_src,
			     const uint32_t *__restrict__ b_tgt, const uint32_t *__restrict__ t_size, const uint8_t *__restrict__ t_flags,
			     const uint32_t *__restrict__ gp, uint32_t *__restrict__ out_ord, uint32_t *__restrict__ in_ord,
			     uint32_t *__restrict__ nself, uint32_t *__restrict__ in_ext, uint8_t *__restrict__ capf,
			     uint8_t *__restrict__ simp, uint8_t *__restrict__ hit1, uint8_t *__restrict__ hit3)
{
	uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= NB)
		return;
	const uint32_t sv = b_src[j], tv = b_tgt[j];
	if (j < NB0) {
		atomicAdd(&out_ord[sv], 1u);
		atomicAdd(&in_ord[tv], 1u);
		if (sv == tv)
			atomicAdd(&nself[sv], 1u);
		// sv = c + 1 for a gray child c with exactly one descendant: does this edge end right above c's parent zi
		// (ai = zi - 1) or three above it (ai = zi - 3)?  Those are the only two ai find_tiny ever asks about.
		if (sv > 0) {
			const uint32_t c = sv - 1;
			if (t_size[c] == 2 && !(t_flags[c] & TF_BLACK)) {
				const uint32_t zi = gp[c];
				if (zi != NIL) {
					if (tv + 1 == zi)
						hit1[c] = 1;
					if (tv + 3 == zi)
						hit3[c] = 1;
				}
			}
		}
	} else {
		if (j < NB0 + ncap)
			capf[sv] = 1;
		else
			simp[sv] = 1;
		atomicAdd(&in_ext[tv], 1u);
	}
}
__global__ void k_leaf_extra_counts(uint32_t T, const uint8_t *__restrict__ capf, const uint8_t *__restrict__ simp, uint8_t *__restrict__ nx)
{
	uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t <= T)
		nx[t] = t < T ? (uint8_t)(capf[t] + simp[t]) : 0;
}
// w[t] = ordinary back edges created just before t is discovered (by its parent); add the ones created after the last
// child of every vertex whose subtree ends right before t.  The tails of subtrees that end with their component are
// created after the component's last discovery and count for nobody.
__global__ void k_leaf_closed(uint32_t T, const uint32_t *__restrict__ t_size, const uint32_t *__restrict__ tail, const CompSpans comp,
			      const uint32_t *__restrict__ c_ntree, uint32_t *__restrict__ w)
{
	uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= T)
		return;
	const uint32_t sz = t_size[t], tl = tail[t];
	if (!sz || !tl)
		return;
	const uint32_t c = comp.of_tree(t), base = 2 * comp.voff[c] + c, end = t + sz;
	if (end < base + c_ntree[c])
		atomicAdd(&w[end], tl);
}


// branches, tiny.cpp:33-73 (trunk, :76-97, is false on every path)
__device__ static bool leaf_tiny(const LeafIn &in, uint32_t ai, uint32_t zi, uint32_t d, uint32_t base, uint32_t N)
{
	const uint32_t end = zi + in.t_size[zi], ai_l = ai - base;
	for (uint32_t c = zi + 1; c < end; c += max(in.t_size[c], 1u)) { // Y = the gray children of zi
		if (in.t_flags[c] & TF_BLACK)
			continue;
		if (in.t_size[c] != 2) // has_one_descendants: post - pre == 3
			return false;
		bool hit = d == 1 ? in.hit1[c] != 0 : in.hit3[c] != 0; // a bracket of c (= an ordinary edge of c + 1) ends at ai
		if (!hit) { // (sic) the back-edge indices of OBE(c) against the vertex idx ai
			const uint32_t b0 = in.B[c + 1] - in.B[base] + in.out_ord[c + 1];
			hit = ai_l >= b0 && ai_l - b0 < in.out_ord[c];
			if (!hit && in.simp[c]) {
				const uint32_t idx = (in.O[base + N] - in.O[base]) + (in.X[base + N] - in.X[c + 1]) + in.capf[c];
				hit = idx == ai_l;
			}
		}
		if (!hit)
			return false;
	}
	return true;
}
// in_branch, parallel.cpp:186-261
__device__ static bool leaf_in_branch(const LeafIn &in, uint32_t ai, uint32_t zi, uint32_t d)
{
	if (d != 1)
		return false;
	const uint32_t end = zi + in.t_size[zi];
	uint32_t c = NIL;
	for (uint32_t x = zi + 1; x < end; x += max(in.t_size[x], 1u)) {
		if (in.t_flags[x] & TF_BLACK)
			continue;
		if (c != NIL)
			return false;
		c = x;
	}
	if (c == NIL) // undefined in the reference (tm.off[INVALID_IDX]); defined as "no" by the oracle
		return false;
	const uint32_t br = (in.P[c + in.t_size[c]] - in.P[c]) - (in.out_ord[c] - in.nself[c]);
	const uint32_t ch_obe = in.out_ord[c] + in.capf[c] + in.simp[c];
	if (br <= 2)
		return false;
	if (in.in_ord[ai] >= br + ch_obe)
		return true;
	return in.out_ord[zi] + in.capf[zi] + in.simp[zi] >= br + ch_obe;
}
// in_trunk + inspect_trunk, parallel.cpp:15-184
__device__ static bool leaf_in_trunk(const LeafIn &in, uint32_t ai, uint32_t zi, uint32_t d)
{
	if (d <= 3 && in.in_ord[ai] + in.in_ext[ai] <= 1) // condition i
		return false;
	if (in.nchild[zi] != 1) // condition iii
		return false;
	// condition iv: no branching vertex from zi up to (not including) ai, or exactly one that has a child behind zi
	// with a single descendant
	uint32_t branching = NIL;
	for (uint32_t v = zi; v != ai; v = in.gp[v]) {
		if (in.gp[v] == NIL)
			return false;
		if (in.nchild[v] > 1) {
			if (branching != NIL)
				return false;
			branching = v;
		}
	}
	if (branching != NIL) {
		bool ok = false;
		const uint32_t end = branching + in.t_size[branching];
		for (uint32_t x = branching + 1; x < end && !ok; x += max(in.t_size[x], 1u))
			ok = x > zi && in.t_size[x] == 2;
		if (!ok)
			return false;
	}
	const uint32_t in_ai = in.in_ord[ai];
	if (2 * in_ai >= d - 3) // u32 on purpose: wraps like the reference when zi - ai < 3
		return true;
	if (in_ai != 0)
		return false;
	return 2 * in.out_ord[zi] >= d - 3;
}

// the letter of a flubble with inner boundary vertices ai / zi (global tree vertex idx) of the component at `base`
__device__ static uint8_t leaf_label(const LeafIn &in, uint32_t ai, uint32_t zi, uint32_t base, uint32_t N, bool leaf)
{
	if (!leaf)
		return FAM_FLUBBLE;
	const uint32_t d = zi - ai;
	if ((d == 1 || d == 3) && leaf_tiny(in, ai, zi, d, base, N)) // find_tiny first; find_parallel skips what it relabelled
		return FAM_TINY;
	if (leaf_in_branch(in, ai, zi, d) || leaf_in_trunk(in, ai, zi, d))
		return FAM_PARALLEL;
	return FAM_FLUBBLE;
}
__device__ __forceinline__ void sort4(uint32_t (&v)[4])
{
#pragma unroll
	for (int a = 0; a < 3; a++)
#pragma unroll
		for (int b = 0; b < 3 - a; b++)
			if (v[b] > v[b + 1]) {
				const uint32_t x = v[b];
				v[b] = v[b + 1];
				v[b + 1] = x;
			}
}

__global__ void k_leaf_flubbles(const LeafIn in, LeafOut out)
{
	uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= in.NE)
		return;
	const uint32_t i = in.e_i[j], c = in.comp_of(i), base = 2 * in.voff[c] + c, N = in.c_ntree[c];
	const uint32_t va = in.s_vtx[i], vz = in.s_vtx[in.ns[i]];
	// compute_ai_zi, flubbles.cpp:264-290: the middle two of the four end vertices of the two boundary tree edges
	uint32_t v[4] = {va, in.gp[va], vz, in.gp[vz]};
	sort4(v);
	const uint32_t ai = v[1], zi = v[2];
	const uint64_t q = (uint64_t)j + in.cproc_ps[c] + 1;
	out.ai[q] = ai - base;
	out.zi[q] = zi - base;
	// the next emitted flubble is this one's child iff it lies deeper (k_pvst_emit: parent = nearest earlier flubble
	// with a smaller level)
	const bool leaf = !(j + 1 < in.NE && in.comp_of(in.e_i[j + 1]) == c && in.lev[j + 1] > in.lev[j]);
	out.fam[q] = leaf_label(in, ai, zi, base, N, leaf);
}
__global__ void k_leaf_roots(uint32_t C, const uint32_t *__restrict__ c_ntree, const uint32_t *__restrict__ doff, LeafOut out)
{
	uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= C || c_ntree[c] == 0)
		return;
	const uint32_t q = doff[c];
	out.ai[q] = out.zi[q] = NIL;
	out.fam[q] = FAM_DUMMY;
}

// ---- components whose add_flubbles went through the sequential redo: their PVST sits in the per-component layout of the
// one-lane kernels (component c owns the slots from voff[c] + c; seq_pvst also left ai / zi there)
__global__ void k_leaf_seq_children(uint32_t P, const CompSpans comp, const uint32_t *__restrict__ comp_bad,
				    const uint32_t *__restrict__ c_npvst, const uint32_t *__restrict__ p_parent,
				    uint8_t *__restrict__ has_child)
{
	uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
	if (slot >= P)
		return;
	const uint32_t c = comp.of_slot(slot), pb = comp.voff[c] + c, k = slot - pb;
	if (!comp_bad[c] || k == 0 || k >= c_npvst[c])
		return;
	has_child[pb + p_parent[slot]] = 1;
}
__global__ void k_leaf_seq_eval(uint32_t P, const LeafIn in, const CompSpans comp, const uint32_t *__restrict__ comp_bad,
				const uint32_t *__restrict__ c_npvst, const uint32_t *__restrict__ p_ai,
				const uint32_t *__restrict__ p_zi, const uint8_t *__restrict__ has_child, uint8_t *__restrict__ p_fam)
{
	uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
	if (slot >= P)
		return;
	const uint32_t c = comp.of_slot(slot), pb = comp.voff[c] + c, k = slot - pb;
	if (!comp_bad[c] || k >= c_npvst[c])
		return;
	if (k == 0) {
		p_fam[slot] = FAM_DUMMY;
		return;
	}
	const uint32_t base = 2 * in.voff[c] + c;
	p_fam[slot] = leaf_label(in, base + p_ai[slot], base + p_zi[slot], base, in.c_ntree[c], has_child[slot] == 0);
}

namespace
{
// what leaf_prepare computes per tree vertex (the redo's arrays and the dense output live in LeafState)
struct LeafTmp {
	uint32_t *gp, *nchild, *out_ord, *in_ord, *nself, *in_ext, *Ps, *O, *X, *w, *tail, *B;
	uint8_t *capf, *simp, *hit1, *hit3, *nx;
	void *scan;
	size_t scan_bytes;
};
void leaf_spans(LeafTmp &t, LeafState &ls, size_t V, size_t C, size_t total, Spans &take)
{
	const size_t T = 2 * V + C, P = V + C;
	take(T + 4, t.gp, t.nchild, t.out_ord, t.in_ord, t.nself, t.in_ext, t.Ps, t.O, t.X, t.w, t.tail, t.B);
	take(T + 64, t.capf, t.simp, t.hit1, t.hit3, t.nx);
	take(total + 16, ls.dense.ai, ls.dense.zi);
	take(total + 64, ls.dense.fam);
	take(P + 4, ls.p_ai, ls.p_zi);
	take(P + 64, ls.p_fam, ls.p_has_child);
	t.scan_bytes = scan_tmp_bytes(T + 4);
	take(t.scan_bytes, t.scan);
}
} // namespace
size_t leaf_workspace_bytes(size_t V, size_t C, size_t total)
{
	LeafTmp t{};
	LeafState ls{};
	return measure([&](Spans &take) { leaf_spans(t, ls, V, C, total, take); }) + (1 << 16);
}

void leaf_prepare(const CompState &cs, const SeqWs &sw, const ParWs &pw, const TreeWs &tw, uint32_t C, Arena &ar, LeafState &ls,
		  hipStream_t s)
{
	const uint32_t V = sw.V, T = 2 * V + C;
	const size_t total = pw.d_total;
	ar.reserve(leaf_workspace_bytes(V, C, total));
	LeafTmp t{};
	Spans take{&ar};
	leaf_spans(t, ls, V, C, total, take);
	ls.P = (size_t)V + C;

	for (uint32_t *p : {t.nchild, t.out_ord, t.in_ord, t.nself, t.in_ext, t.w, t.tail})
		HIP_CHECK(hipMemsetAsync(p, 0, ((size_t)T + 4) * 4, s));
	for (uint8_t *p : {t.capf, t.simp, t.hit1, t.hit3})
		HIP_CHECK(hipMemsetAsync(p, 0, (size_t)T + 64, s));
	const CompSpans comp{cs.voff, C};
	LAUNCH(k_leaf_tree, T, s, T, sw.t_size, sw.t_par, comp, t.gp, t.nchild);
	const uint32_t NB = pw.nb0 + pw.ncap + pw.nsimp;
	LAUNCH(k_leaf_edges, NB, s, NB, pw.nb0, pw.ncap, pw.b_src, pw.b_tgt, sw.t_size, sw.t_flags, t.gp, t.out_ord, t.in_ord, t.nself, t.in_ext,
	       t.capf, t.simp, t.hit1, t.hit3);
	LAUNCH(k_leaf_extra_counts, (size_t)T + 1, s, T, t.capf, t.simp, t.nx);
	scan_exclusive_diff_u32(t.out_ord, t.in_ord, t.Ps, (size_t)T + 1, t.scan, t.scan_bytes, s);
	scan_exclusive_u32(t.out_ord, t.O, (size_t)T + 1, t.scan, t.scan_bytes, s);
	scan_exclusive_u8(t.nx, t.X, (size_t)T + 1, nullptr, nullptr, 0, t.scan, t.scan_bytes, s);
	edge_id_weights(cs, sw, tw, t.w, t.tail, s);
	LAUNCH(k_leaf_closed, T, s, T, sw.t_size, t.tail, comp, sw.c_ntree, t.w);
	scan_exclusive_u32(t.w, t.B, (size_t)T + 2, t.scan, t.scan_bytes, s);

	LeafIn &in = ls.in;
	in = LeafIn{};
	in.NE = pw.n_emitted;
	in.C = C;
	in.voff = cs.voff;
	in.c_ntree = sw.c_ntree;
	in.cproc_ps = pw.cproc_ps;
	in.e_i = pw.e_i;
	in.lev = pw.lev;
	in.comp_of = pw.stack_comp();
	in.s_vtx = pw.s_vtx;
	in.ns = pw.ns;
	in.t_size = sw.t_size;
	in.gp = t.gp;
	in.nchild = t.nchild;
	in.t_flags = sw.t_flags;
	in.out_ord = t.out_ord;
	in.in_ord = t.in_ord;
	in.nself = t.nself;
	in.in_ext = t.in_ext;
	in.capf = t.capf;
	in.simp = t.simp;
	in.hit1 = t.hit1;
	in.hit3 = t.hit3;
	in.P = t.Ps;
	in.O = t.O;
	in.X = t.X;
	in.B = t.B;
}

void leaf_dense(const LeafState &ls, const SeqWs &sw, const ParWs &pw, uint32_t C, hipStream_t s)
{
	LAUNCH(k_leaf_roots, C, s, C, sw.c_ntree, pw.doff, ls.dense);
	LAUNCH(k_leaf_flubbles, ls.in.NE, s, ls.in, ls.dense);
}

void leaf_seq(const LeafState &ls, const CompState &cs, const SeqWs &sw, const uint32_t *comp_bad, uint32_t C, hipStream_t s)
{
	const uint32_t P = (uint32_t)ls.P;
	const CompSpans comp{cs.voff, C};
	HIP_CHECK(hipMemsetAsync(ls.p_has_child, 0, ls.P + 64, s));
	LAUNCH(k_leaf_seq_children, P, s, P, comp, comp_bad, sw.c_npvst, sw.p_parent, ls.p_has_child);
	LAUNCH(k_leaf_seq_eval, P, s, P, ls.in, comp, comp_bad, sw.c_npvst, ls.p_ai, ls.p_zi, ls.p_has_child, ls.p_fam);
}

} // namespace povu_hip
