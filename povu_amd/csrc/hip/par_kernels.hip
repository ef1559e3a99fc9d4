// par_kernels.hip -- rows D-G as data-parallel kernels over ALL components at once.
//
// The reference computes these stages with sequential sweeps (reverse pre-order bracket lists,
// a list-splicing tree walk, a hash-map sweep and a stack machine).  Because the tree vertex idx
// IS the DFS pre-order number, every one of them has an exact closed form over pre-order
// intervals [v, v+size(v)); the kernels below evaluate those closed forms with scans, radix
// sorts and min-segment-tree descents.  DESIGN.md ("Parallel formulations") derives each one;
// tests/ differential-test them against the oracle (and the sequential kernels) bit for bit.
//
//   D  cycle classes      flubbles.cpp:503-719 (handle_vertex), bracket_list.cpp:61-100
//   E  candidate stack    tree_utils.cpp:19-155, flubbles.cpp:412-501
//   F  next_seen          flubbles.cpp:375-410
//   G  PVST               flubbles.cpp:295-367
//
// Index spaces: T-space = global tree vertex idx (component c starts at 2*voff[c]+c, holes are
// marked gsize == 0); bracket space (dense, all components); stack space (one entry per black
// tree edge, component-major); emitted-flubble space.
#include "par_kernels.hpp"
#include "segtree.hpp"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace povu_hip
{

#define NIL POVU_NIL
static constexpr size_t PVST_STAGE_MIN = size_t(1) << 20; // PVST vertices from which the result goes through a device block

// ------------------------------------------------------------- T-space setup
// component c owns the tree-vertex slots [2 voff[c] + c, 2 voff[c+1] + c]: two per segment and one more
// (the dummy root, when it exists, shifts the sides up by one); t_comp[T] = NIL closes the array
__global__ void k_tcomp_vertices(uint32_t V, uint32_t T, const uint32_t *__restrict__ ckey, const uint32_t *__restrict__ voff,
				 uint32_t *__restrict__ t_comp)
{
	uint32_t i = BIDX * blockDim.x + threadIdx.x;
	if (i >= V)
		return;
	uint32_t c = ckey[i];
	t_comp[2 * i + c] = c;
	t_comp[2 * i + 1 + c] = c;
	if (i + 1 == voff[c + 1])
		t_comp[2 * i + 2 + c] = c;
	if (i == V - 1)
		t_comp[T] = NIL;
}
__global__ void k_globalize(uint32_t T, const uint32_t *__restrict__ t_comp, const uint32_t *__restrict__ voff,
			    const uint32_t *__restrict__ c_ntree, const uint32_t *__restrict__ t_par,
			    const uint32_t *__restrict__ t_size, uint32_t *__restrict__ gpar, uint32_t *__restrict__ gsize,
			    uint32_t *__restrict__ t_root, uint32_t *__restrict__ hi0, uint32_t *__restrict__ cov,
			    const uint32_t *__restrict__ depth, uint32_t *__restrict__ mpre, uint32_t *__restrict__ incnt,
			    uint32_t *__restrict__ srccnt, uint8_t *__restrict__ t_flags)
{
	uint32_t t = BIDX * blockDim.x + threadIdx.x;
	if (t >= T)
		return;
	if (srccnt) { // (null: the tree stage keeps the counts as bytes and has cleared the slots without a vertex)
		srccnt[t] = 0; // brackets per source, [T+2]
		if (t == T - 1)
			srccnt[T] = srccnt[T + 1] = 0;
	}
	if (cov) { // (not on the dense path: the tree stage left hi0 and the count of bracket ends, and needs no coverage array)
		hi0[t] = NIL; // k_hi0 takes minima into it
		cov[t] = 0;   // ... and counts back-edge ends here
		incnt[t] = 0; // brackets that end at a vertex, [T+2]
		if (t == T - 1) {
			hi0[T] = NIL;
			cov[T] = 0;
			incnt[T] = incnt[T + 1] = 0;
		}
	} else if (t == T - 1) {
		hi0[T] = NIL;
	}
	uint32_t c = t_comp[t];
	uint32_t base = 2 * voff[c] + c, l = t - base, n = c_ntree[c];
	t_root[t] = base;
	if (l < n) {
		uint32_t p = t_par[t], sz = t_size[t];
		gpar[t] = p == NIL ? NIL : base + p;
		if (p == NIL)
			t_flags[t] |= TF_ROOT; // (k_tree_emit has set it already; a one-lane tree stage writes the two low fields only)
		gsize[t] = sz;
		// mirror pre-order (children visited in DESCENDING idx): the order brackets sit in a bracket list, because each
		// child's list is spliced in front of its earlier siblings' (flubbles.cpp:586-588).  With q(v) = mpre(v) + v + size(v)
		// one gets q(child) = q(parent) + 1, hence mpre(v) = depth(v) + N - v - size(v) (local indices, N = tree vertices
		// of the component)
		mpre[t] = base + depth[t] + n - l - sz;
	} else {
		gpar[t] = NIL;
		gsize[t] = 0;
		mpre[t] = NIL;
	}
}
__global__ void k_dense_be(uint32_t NB0, uint32_t C, const uint32_t *__restrict__ dbo, const uint32_t *__restrict__ voff,
			   const uint32_t *__restrict__ eoff, const uint32_t *__restrict__ be_src,
			   const uint32_t *__restrict__ be_tgt, uint32_t *__restrict__ b_src, uint32_t *__restrict__ b_tgt)
{
	uint32_t j = BIDX * blockDim.x + threadIdx.x;
	if (j >= NB0)
		return;
	uint32_t c = span_of(dbo, C, j), b = j - dbo[c];
	uint64_t tb = 2ull * voff[c] + c, bb = (uint64_t)eoff[c] + voff[c] + 2 * tb;
	b_src[j] = (uint32_t)tb + be_src[bb + b];
	b_tgt[j] = (uint32_t)tb + be_tgt[bb + b];
}

// ------------------------------------------------------------- row D
// hi0(v) = min target of v's own back edges; cov(v) = back edges leaving v minus back edges arriving at v.  A back
// edge runs from a descendant to an ancestor, so the sum of cov over subtree(v) counts exactly the back edges that
// leave subtree(v) upwards past v.
// (incnt, when given: brackets that end at a vertex -- the ordinary ones are counted here, while their ends are in hand)
__global__ void k_hi0(uint32_t NB0, const uint32_t *__restrict__ b_src, const uint32_t *__restrict__ b_tgt,
		      uint32_t *__restrict__ hi0, uint32_t *__restrict__ cov, uint32_t *__restrict__ incnt)
{
	uint32_t j = BIDX * blockDim.x + threadIdx.x;
	if (j >= NB0)
		return;
	const uint32_t sv = b_src[j], tv = b_tgt[j];
	atomicMin(&hi0[sv], tv);
	if (incnt) { // (dense path: cov = edges leaving - edges arriving is read off the two counts, see run_parallel_dg)
		atomicAdd(&incnt[tv], 1u);
	} else if (sv != tv) {
		atomicAdd(&cov[sv], 1u);
		atomicSub(&cov[tv], 1u);
	}
}
// bridge(v): no ordinary back edge out of subtree(v) reaches a proper ancestor of v (the bracket list of v would be
// empty but for simplifying edges): the subtree sum of cov is zero
// (four vertices a lane, 16-byte loads: see k_entry_list)
__global__ void __launch_bounds__(TPB) k_bridge_flags(uint32_t T, const uint32_t *__restrict__ gsize, const uint8_t *__restrict__ t_flags,
						       const uint32_t *__restrict__ pscov, uint4 *__restrict__ brec)
{
	// the flags go out as BITS, 64 to a record of the bit-rank directory (common.hpp): "how many bridge vertices in front of x"
	// is then one 16-byte look-up into a 50 MB table -- until round 5 a byte per vertex, scanned into a 4-byte prefix per vertex
	// ("has a parent" is the root bit of the tree stage's flag bytes, four of them in one word: the parents themselves are not read)
	const uint32_t t0 = (BIDX * blockDim.x + threadIdx.x) * 4u;
	uint32_t f = 0;
	if (t0 + 4 <= T) {
		const uint4 sz = *reinterpret_cast<const uint4 *>(gsize + t0);
		const uint32_t tf = *reinterpret_cast<const uint32_t *>(t_flags + t0);
		const uint4 pc = *reinterpret_cast<const uint4 *>(pscov + t0);
		f = ((sz.x && !(tf & TF_ROOT) && pscov[t0 + sz.x] == pc.x) ? 1u : 0u) |
		    ((sz.y && !(tf & (TF_ROOT << 8)) && pscov[t0 + 1 + sz.y] == pc.y) ? 2u : 0u) |
		    ((sz.z && !(tf & (TF_ROOT << 16)) && pscov[t0 + 2 + sz.z] == pc.z) ? 4u : 0u) |
		    ((sz.w && !(tf & (TF_ROOT << 24)) && pscov[t0 + 3 + sz.w] == pc.w) ? 8u : 0u);
	} else {
		for (uint32_t t = t0; t < T; t++) {
			const uint32_t sz = gsize[t];
			f |= ((sz && !(t_flags[t] & TF_ROOT) && pscov[t + sz] == pscov[t]) ? 1u : 0u) << (t - t0);
		}
	}
	const uint32_t w0 = (BIDX * blockDim.x + (threadIdx.x & ~63u)) / 16u; // first record of this wave's 256 vertices
	bitrank_store_wave(brec + w0, f, w0 + (threadIdx.x & 63u) <= T / 64u);
}
// capping back edge v -> hi_2 when hi_2 < hi_0 (flubbles.cpp:555-574, 613-619).  Children of v in
// ascending idx are v+1, then each next sibling at c + size(c).  hi(c) = min target of the back edges leaving
// subtree(c) -- the root as soon as subtree(c) holds a simplifying edge -- is only ever compared between siblings,
// so it is evaluated on demand, for the children of branching vertices alone (range-min over hi0).
// Root of the tree that holds tree vertex t.  The all-parallel pass keeps no per-vertex table of it (it is needed at
// few vertices): component c owns [2 voff[c] + c, 2 voff[c+1] + c], so the component is found by bisection over voff.
struct RootOf {
	const uint32_t *t_root; // per-vertex table, or null: bisect
	const uint32_t *voff;
	uint32_t C;
	__device__ __forceinline__ uint32_t operator()(uint32_t t) const
	{
		if (t_root)
			return t_root[t];
		const uint32_t c = CompSpans{voff, C}.of_tree(t);
		return 2 * voff[c] + c;
	}
};
// rank(x) out of the record that holds x (bitrank, common.hpp)
__device__ __forceinline__ uint32_t bitrank_in(const uint4 &r, uint32_t x)
{
	const unsigned long long bits = (unsigned long long)r.x | ((unsigned long long)r.y << 32);
	return r.z + (uint32_t)__popcll(bits & ((1ull << (x & 63u)) - 1ull));
}
// the smallest of the first n (1 .. 8) of eight words
__device__ __forceinline__ uint32_t min_of_first(const uint4 &a, const uint4 &b, uint32_t n)
{
	uint32_t m = a.x;
	m = min(m, n > 1 ? a.y : NIL), m = min(m, n > 2 ? a.z : NIL), m = min(m, n > 3 ? a.w : NIL);
	m = min(m, n > 4 ? b.x : NIL), m = min(m, n > 5 ? b.y : NIL), m = min(m, n > 6 ? b.z : NIL), m = min(m, n > 7 ? b.w : NIL);
	return m;
}
__device__ __forceinline__ void capping_of(uint32_t v, const uint32_t *__restrict__ gsize, const uint32_t *__restrict__ hi0,
					   const uint4 *__restrict__ brec, const RootOf &root_of,
					   const SegTree &segA, uint32_t *__restrict__ cap_tgt,
					   uint8_t *__restrict__ capf, uint32_t *__restrict__ literal_rule_seen, uint32_t hi0_words)
{
	uint32_t root = NIL; // of v's tree, looked up at most once
	auto root_once = [&]() __attribute__((always_inline)) {
		if (root == NIL)
			root = root_of(v);
		return root;
	};
	auto hi_of = [&](uint32_t c) {
		const uint32_t cs = max(gsize[c], 1u);
		if (bitrank(brec, c + cs) != bitrank(brec, c)) // a bridge vertex in subtree(c): a simplifying edge sits at or below it
			return root_once();
		if (cs <= 8) { // a small branch: its hi0 values share a cache line or two
			uint32_t m = NIL;
			for (uint32_t k = c; k < c + cs; k++)
				m = min(m, hi0[k]);
			return m;
		}
		return seg_min(segA, c, c + cs);
	};
	// one sweep over the children: the first child that attains the minimum (hi_child), and the first two children
	// whose hi lies above v in the tree -- hi_2 belongs to the first of them that is not hi_child
	uint32_t hi_1 = NIL, hi_child = NIL, lt_c0 = NIL, lt_c1 = NIL, lt_h0 = NIL, lt_h1 = NIL;
	uint32_t second = NIL; // the second smallest hi over the children, with multiplicity: what hi_2 "should" be
	auto take = [&](uint32_t c, uint32_t h) __attribute__((always_inline)) { // (three call sites: kept in registers only when inlined)
		if (h < hi_1 || hi_child == NIL) {
			second = hi_1;
			hi_1 = h;
			hi_child = c;
		} else {
			second = min(second, h);
		}
		// (as selects: written as branches, the four words ended up in scratch memory behind a selected address)
		const bool f0 = h < v && lt_c0 == NIL, f1 = h < v && !f0 && lt_c1 == NIL;
		lt_c0 = f0 ? c : lt_c0, lt_h0 = f0 ? h : lt_h0;
		lt_c1 = f1 ? c : lt_c1, lt_h1 = f1 ? h : lt_h1;
	};
	// The first two children -- a branching vertex has them, and mostly no more -- without the chain child -> its size ->
	// the records behind its subtree -> its hi0 words -> next child: ONE run of loads takes everything at v and at the
	// first child that does not depend on the child's size (both sizes, hi0[v], the bit-rank record at the child, the eight
	// hi0 words from the child on: a subtree of up to eight vertices needs no more), a second run the same at the second
	// child, whose record is also the one the first child's subtree ends in.  The eight words are read whatever the
	// subtree's size: they must lie inside hi0's hi0_words words, or the vertex goes through the loop below as a whole
	// (the last few vertices of the tree space).  Further children: the loop, as before.
	uint32_t c = v + 1, end, hv;
	if (c + 8 <= hi0_words) {
		uint32_t szv = gsize[v], g1 = gsize[c];
		hv = hi0[v];
		uint4 r1 = brec[c >> 6], a1 = load4_unaligned(hi0 + c), b1 = load4_unaligned(hi0 + c + 4);
		landed(szv, hv, g1, r1, a1, b1);
		end = v + szv;
		const uint32_t cs1 = max(g1, 1u), c2 = c + cs1; // c2 < end <= T: the list holds vertices with a second child only (k_hi_simp)
		if (c2 + 8 <= hi0_words) {
			uint32_t g2 = gsize[c2];
			uint4 r2 = brec[c2 >> 6], a2 = load4_unaligned(hi0 + c2), b2 = load4_unaligned(hi0 + c2 + 4);
			landed(g2, r2, a2, b2);
			const uint32_t cs2 = max(g2, 1u), c3 = c2 + cs2; // c3 <= end: its record exists (rank(T) is asked for)
			// (mostly the record in hand.  Tied to registers first: the plain select became a flat load from a selected
			// address, with the record in hand stored to scratch memory for it)
			uint4 r3 = r2;
			landed(r3);
			if ((c3 >> 6) != (c2 >> 6))
				r3 = brec[c3 >> 6];
			const uint32_t k1 = bitrank_in(r1, c), k2 = bitrank_in(r2, c2), k3 = bitrank_in(r3, c3);
			take(c, k2 != k1 ? root_once() : cs1 <= 8 ? min_of_first(a1, b1, cs1) : seg_min(segA, c, c2));
			take(c2, k3 != k2 ? root_once() : cs2 <= 8 ? min_of_first(a2, b2, cs2) : seg_min(segA, c2, c3));
			c = c3;
		}
	} else {
		end = v + gsize[v];
		hv = hi0[v];
	}
	for (; c < end; c += max(gsize[c], 1u))
		take(c, hi_of(c));
	const uint32_t hi_2 = lt_c0 != hi_child ? lt_h0 : lt_h1;
	// The literal rule (first other child in idx order with hi < v, not the one reaching highest) can leave a capping
	// edge that ends too early; only then can a bracket come back on top with MORE brackets under it than before.
	// The black-edge-only class pass relies on that never happening (see run_parallel_dg), so say when it might.
	if (hi_2 != (second < v ? second : NIL))
		*literal_rule_seen = 1u;
	if (hi_2 < hv) {
		cap_tgt[v] = hi_2;
		capf[v] = 1;
	}
}
// simplifying(v): bridge(v) and no bridge vertex below it (the deepest ones get the back edge to
// the root, flubbles.cpp:621-643)
// ... and which vertices BRANCH (two or more children): only they can get a capping edge, about one vertex in nine.
// The sweep over a branching vertex's children is a chain of dependent gathers (child, its size, the flags behind its
// subtree, the next child ...): it runs in a kernel of its own over the compacted list of branching vertices, every lane
// busy with one of them -- inside this kernel the few lanes that had work left the rest of their workgroup waiting.
static constexpr uint32_t HS_ITER = LIST_ITER, HS_VERTS = LIST_SPAN; // vertices a workgroup of k_hi_simp takes: one atomic add for 16 384 of them
static_assert(TPB == (int)LIST_TPB, "append_in_order is written for workgroups of 256");
__global__ void __launch_bounds__(TPB) k_hi_simp(uint32_t T, const uint32_t *__restrict__ gsize, const uint4 *__restrict__ brec,
						  uint8_t *__restrict__ simp, uint8_t *__restrict__ hpf,
						  uint8_t *__restrict__ capf, uint32_t *__restrict__ br_list, uint32_t *__restrict__ n_br)
{
	const uint32_t B0 = BIDX * HS_VERTS;
	// p0 = bridge vertices in front of t: simplifying iff t is the only one of its subtree
	auto one = [&](uint32_t t, uint32_t sz, uint32_t br, uint32_t p0, uint32_t sz_next, uint32_t &sm, uint32_t &bch) {
		sm = (sz && br && bitrank(brec, t + sz) - p0 == 1) ? 1u : 0u;
		bch = (sz > 2 && t + 1 + max(sz_next, 1u) < t + sz) ? 1u : 0u; // the first child does not fill the subtree
	};
	unsigned long long bw = 0; // bit 4 it + j: vertex B0 + it * 1024 + 4 tid + j branches
#pragma unroll 4
	for (uint32_t it = 0; it < HS_ITER; it++) {
		const uint32_t t0 = B0 + it * (TPB * 4u) + threadIdx.x * 4u; // (four vertices a lane, 16-byte loads: see k_entry_list)
		uint32_t b4 = 0;
		if (t0 + 4 < T) { // (strictly: the last of the four looks at its successor's size)
			const uint4 sz = *reinterpret_cast<const uint4 *>(gsize + t0);
			const uint32_t sz4 = gsize[t0 + 4];
			// the four flags and the count in front of them out of one record (t0 is a multiple of four: one record holds all four)
			const uint4 r = brec[t0 >> 6];
			const unsigned long long bits = (unsigned long long)r.x | ((unsigned long long)r.y << 32);
			const uint32_t br = (uint32_t)(bits >> (t0 & 63u)) & 15u;
			const uint32_t p0 = r.z + (uint32_t)__popcll(bits & ((1ull << (t0 & 63u)) - 1ull));
			const uint32_t p1 = p0 + (br & 1u), p2 = p1 + ((br >> 1) & 1u), p3 = p2 + ((br >> 2) & 1u);
			uint32_t s0, s1, s2, s3, c0, c1, c2, c3;
			one(t0, sz.x, br & 1u, p0, sz.y, s0, c0);
			one(t0 + 1, sz.y, br & 2u, p1, sz.z, s1, c1);
			one(t0 + 2, sz.z, br & 4u, p2, sz.w, s2, c2);
			one(t0 + 3, sz.w, br & 8u, p3, sz4, s3, c3);
			const uint32_t sw = s0 | (s1 << 8) | (s2 << 16) | (s3 << 24);
			*reinterpret_cast<uint32_t *>(simp + t0) = sw;
			if (hpf)
				*reinterpret_cast<uint32_t *>(hpf + t0) = sw;
			*reinterpret_cast<uint32_t *>(capf + t0) = 0u; // (cap_tgt is only read where capf says so)
			b4 = c0 | (c1 << 1) | (c2 << 2) | (c3 << 3);
		} else {
			for (uint32_t t = t0; t < T; t++) {
				uint32_t sm, bch;
				one(t, gsize[t], bitrank_test(brec, t) ? 1u : 0u, bitrank(brec, t), gsize[t + 1], sm, bch);
				simp[t] = (uint8_t)sm;
				if (t == T - 1)
					simp[T] = 0;
				if (hpf)
					hpf[t] = (uint8_t)sm;
				capf[t] = 0;
				b4 |= bch << (t - t0);
			}
		}
		bw |= (unsigned long long)b4 << (4 * it);
	}
	// the branching vertices go straight onto the list k_capping works through, in vertex order (append_in_order, common.hpp)
	append_in_order(bw, B0, br_list, n_br);
}
__global__ void k_capping(const uint32_t *__restrict__ n_list, const uint32_t *__restrict__ list, const uint32_t *__restrict__ gsize,
			  const uint32_t *__restrict__ hi0, const uint4 *__restrict__ brec, const RootOf root_of, const SegTree segA,
			  uint32_t *__restrict__ cap_tgt, uint8_t *__restrict__ capf, uint32_t *__restrict__ literal_rule_seen,
			  uint32_t hi0_words)
{
	const uint32_t n = *n_list; // (the count only exists on the device: grid-stride)
	for (uint32_t i = BIDX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
		capping_of(list[i], gsize, hi0, brec, root_of, segA, cap_tgt, capf, literal_rule_seen, hi0_words);
}
// Bracket list order = (mirror pre-order of the source) and, inside one source, the later pushed
// first: simplifying, capping, ordinary edges by descending creation idx (flubbles.cpp:608-643).
// The brackets are laid out in an initial order that already satisfies the second criterion
// (simplifying | capping | ordinary by DESCENDING dense idx), so ONE stable 32-bit radix sort by the
// source's mirror pre-order yields the list order.
// Where a capping / simplifying bracket goes needs the rank of its vertex among the flagged ones.  No prefix arrays: the
// flags are counted per workgroup of k_bracket_extra (k_flag_tile_counts, 256 vertices a tile), the two count arrays
// scanned, and k_bracket_extra ranks its own 256 flags again with ballots.
static constexpr uint32_t BX_TILE = TPB;
__global__ void __launch_bounds__(TPB) k_flag_tile_counts(uint32_t T, const uint8_t *__restrict__ capf, const uint8_t *__restrict__ simp,
							   uint32_t *__restrict__ tcap, uint32_t *__restrict__ tsimp, uint32_t ntiles)
{
	// a workgroup counts 16 tiles: every lane takes 16 consecutive vertices (one 16-byte load per flag array), sixteen
	// consecutive lanes make a tile
	const uint32_t e0 = (blockIdx.x * TPB + threadIdx.x) * 16u;
	uint32_t nc = 0, ns = 0;
	if (e0 + 16 <= T) {
		const uint4 a = *reinterpret_cast<const uint4 *>(capf + e0), b = *reinterpret_cast<const uint4 *>(simp + e0);
		const uint32_t wa[4] = {a.x, a.y, a.z, a.w}, wb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
		for (int k = 0; k < 4; k++)
#pragma unroll
			for (int q = 0; q < 4; q++) {
				nc += ((wa[k] >> (8 * q)) & 0xFFu) ? 1u : 0u;
				ns += ((wb[k] >> (8 * q)) & 0xFFu) ? 1u : 0u;
			}
	} else {
		for (uint32_t k = e0; k < T; k++) {
			nc += capf[k] ? 1u : 0u;
			ns += simp[k] ? 1u : 0u;
		}
	}
	for (int off = 8; off; off >>= 1) {
		nc += __shfl_down(nc, off, 16);
		ns += __shfl_down(ns, off, 16);
	}
	const uint32_t tile = (blockIdx.x * TPB + threadIdx.x) / 16u;
	if ((threadIdx.x & 15u) == 0 && tile <= ntiles) { // (tile == ntiles closes the arrays: the scan leaves the totals there)
		tcap[tile] = tile < ntiles ? nc : 0u;
		tsimp[tile] = tile < ntiles ? ns : 0u;
	}
}
// Four vertices a lane (16-byte loads: a kernel of a few loads per element is bound by its memory INSTRUCTIONS), so a
// wave covers exactly one tile of 256 vertices and ranks its flags with eight ballots; no LDS, no barrier.
// (the counts it places by -- ordinary back edges, capping vertices -- are read from the device: the kernel is launched
// before the host has them, see the driver)
// OC / SC / IC: the width of the three bracket counts (ParWs::narrow_*).  With incnt as bytes a bracket that ends at a root is
// not counted (every simplifying bracket; a capping bracket whose target carries the root bit), and a capping target whose
// byte stands at 255 raises *ovf instead of counting (see ParWs::incnt8): nothing here is indexed by the counts.
template <typename OC, typename SC, typename IC>
__global__ void __launch_bounds__(TPB) k_bracket_extra(uint32_t T, uint32_t NB0_host, const uint32_t *__restrict__ nb0_dev, uint32_t ntiles,
							uint32_t nb_cap, const uint8_t *__restrict__ capf,
							const uint32_t *__restrict__ tcap, const uint8_t *__restrict__ simp,
							const uint32_t *__restrict__ tsimp, const uint32_t *__restrict__ cap_tgt,
							const RootOf root_of, uint32_t *__restrict__ b_src, uint32_t *__restrict__ b_tgt,
							const OC *__restrict__ ordcnt, const uint32_t *__restrict__ gsize,
							const uint32_t *__restrict__ mpre, IC *__restrict__ incnt,
							SC *__restrict__ srccnt, const uint8_t *__restrict__ t_flags,
							uint32_t *__restrict__ ovf)
{
	const uint32_t NB0 = nb0_dev ? *nb0_dev : NB0_host, ncap = tcap[ntiles];
	if ((uint64_t)NB0 + ncap + tsimp[ntiles] > nb_cap)
		return; // (an internal sizing bug: the host throws when it reads the counts; nothing is written out of bounds)
	const uint32_t v0 = (BIDX * blockDim.x + threadIdx.x) * 4u, lane = threadIdx.x & 63u, tile = v0 / BX_TILE;
	uint32_t cw = 0, sw = 0; // the four flag bytes of this lane
	if (v0 + 4 <= T) {
		cw = *reinterpret_cast<const uint32_t *>(capf + v0);
		sw = *reinterpret_cast<const uint32_t *>(simp + v0);
	} else {
		for (uint32_t j = 0; v0 + j < T && j < 4; j++) {
			cw |= (capf[v0 + j] ? 1u : 0u) << (8 * j);
			sw |= (simp[v0 + j] ? 1u : 0u) << (8 * j);
		}
	}
	// rank among the flagged vertices: the tiles before (scanned counts) + the lanes before + this lane's own earlier ones
	const unsigned long long lt = (1ull << lane) - 1ull;
	uint32_t rc = 0, rs = 0;
#pragma unroll
	for (int j = 0; j < 4; j++) {
		rc += (uint32_t)__popcll(__ballot(((cw >> (8 * j)) & 0xFFu) != 0) & lt);
		rs += (uint32_t)__popcll(__ballot(((sw >> (8 * j)) & 0xFFu) != 0) & lt);
	}
	if (v0 >= T)
		return;
	if (cw)
		rc += tcap[tile];
	if (sw)
		rs += tsimp[tile];
	uint4 oc = make_uint4(0u, 0u, 0u, 0u), gs = oc, mp = oc;
	if (ordcnt) {
		if (v0 + 4 <= T) {
			if constexpr (sizeof(OC) == 1) { // the lane's four counts in one word
				const uint32_t w = *reinterpret_cast<const uint32_t *>(ordcnt + v0);
				oc = make_uint4(w & 0xFFu, (w >> 8) & 0xFFu, (w >> 16) & 0xFFu, w >> 24);
			} else {
				oc = *reinterpret_cast<const uint4 *>(ordcnt + v0);
			}
			gs = *reinterpret_cast<const uint4 *>(gsize + v0);
			mp = *reinterpret_cast<const uint4 *>(mpre + v0);
		} else {
			uint32_t *o = &oc.x, *g = &gs.x, *m = &mp.x;
			for (uint32_t j = 0; v0 + j < T && j < 4; j++)
				o[j] = ordcnt[v0 + j], g[j] = gsize[v0 + j], m[j] = mpre[v0 + j];
		}
	}
	const uint32_t ocv[4] = {oc.x, oc.y, oc.z, oc.w}, gsv[4] = {gs.x, gs.y, gs.z, gs.w}, mpv[4] = {mp.x, mp.y, mp.z, mp.w};
#pragma unroll
	for (uint32_t j = 0; j < 4; j++) {
		const uint32_t v = v0 + j;
		if (v >= T)
			break;
		const uint32_t c = (cw >> (8 * j)) & 0xFFu, sm = (sw >> (8 * j)) & 0xFFu;
		if (c) {
			const uint32_t q = NB0 + rc++;
			const uint32_t tg = cap_tgt[v];
			b_src[q] = v;
			b_tgt[q] = tg;
			if constexpr (sizeof(IC) == 1) {
				if (!(t_flags[tg] & TF_ROOT) && incnt_add(incnt, tg) == 255u) {
					incnt_take_back(incnt, tg);
					atomicOr(ovf, 1u);
				}
			} else if (ordcnt) {
				incnt_add(incnt, tg);
			}
		}
		if (sm) {
			const uint32_t q = NB0 + ncap + rs++;
			const uint32_t root = root_of(v);
			b_src[q] = v;
			b_tgt[q] = root;
			if (sizeof(IC) == 4 && ordcnt)
				incnt_add(incnt, root);
		}
		// (dense path) brackets per source, at its place in the list order: known per vertex, no counting pass over the brackets
		if (ordcnt && gsv[j])
			srccnt[mpv[j]] = (SC)(ocv[j] + (c ? 1u : 0u) + (sm ? 1u : 0u)); // (a byte only when ordcnt + 2 < 256 everywhere)
	}
}
__global__ void k_bracket_order(uint32_t NB, uint32_t NB0, uint32_t ncap, uint32_t nsimp, const uint32_t *__restrict__ b_src,
				const uint32_t *__restrict__ b_tgt, const uint32_t *__restrict__ mpre,
				uint32_t *__restrict__ key, uint32_t *__restrict__ val, uint32_t *__restrict__ incnt,
				uint32_t *__restrict__ srccnt)
{
	uint32_t q = BIDX * blockDim.x + threadIdx.x;
	if (q >= NB)
		return;
	uint32_t j;
	if (q < nsimp)
		j = NB0 + ncap + q;
	else if (q < nsimp + ncap)
		j = NB0 + (q - nsimp);
	else
		j = NB0 - 1 - (q - nsimp - ncap);
	uint32_t m = mpre[b_src[j]];
	key[q] = m;
	val[q] = j;
	atomicAdd(&incnt[b_tgt[j]], 1u);
	atomicAdd(&srccnt[m], 1u); // brackets per mirror pre-order position -> range starts
}
// With the per-source rank of every ordinary edge known (parallel tree stage), the list order needs no
// sort: a bracket's position = (first bracket of its source's mirror pre-order position) + its rank
// inside the source (simplifying, capping, ordinary edges top first).
// BS: how the range starts are read (PrefixWords / PrefixRecords, common.hpp)
template <class BS>
__global__ void k_bracket_place(uint32_t NB, uint32_t NB0, uint32_t ncap, const uint32_t *__restrict__ b_src,
				const uint32_t *__restrict__ b_tgt, const uint32_t *__restrict__ b_ord,
				const uint32_t *__restrict__ mpre, const BS bstart,
				const uint8_t *__restrict__ capf, const uint8_t *__restrict__ simp,
				uint32_t *__restrict__ tgtR, uint32_t *__restrict__ rid)
{
	uint32_t j = BIDX * blockDim.x + threadIdx.x;
	if (j >= NB)
		return;
	const uint32_t v = b_src[j], m = mpre[v];
	uint32_t rank;
	if (j < NB0) // b_ord counts from the bottom of the source's ordinary edges; the list has the later pushed on top
		rank = bstart.count(m) - 1 - b_ord[j];
	else if (j < NB0 + ncap)
		rank = simp[v];
	else
		rank = 0;
	const uint32_t pos = bstart.at(m) + rank;
	tgtR[pos] = b_tgt[j];
	if (rid) // (which bracket sits at a list position: only the hairpin report asks, k_top_bracket)
		rid[pos] = j;
}
__global__ void k_gather_u32(uint32_t n, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ src,
			     uint32_t *__restrict__ dst)
{
	uint32_t i = BIDX * blockDim.x + threadIdx.x;
	if (i < n)
		dst[i] = src[idx[i]];
}
// top bracket and bracket-list size at v when the class of tree edge (parent(v), v) is decided
// (flubbles.cpp:664-686): the live brackets are those with source in subtree(v) and target a
// proper ancestor of v; in list order they are the contiguous range [bstart[mpre(v)],
// bstart[mpre(v)+size(v)]), the top is the first live one.  Output in DESCENDING v order so that a
// stable sort by top bracket leaves every group ordered from the deepest vertex up.
// where the candidate-stack entry of a black vertex goes (row E worked out before the class pass)
struct StackPlace {
	const uint32_t *voff, *soff, *shift; // shift: the INCLUSIVE sums of row E's differences (one stream, not the exclusive sums and the differences)
	uint32_t *s_vtx;
};
// BLACK: only the child ends of black tree edges take part (n = V of them: segment slot g of component c is tree
// vertex 2g + c + [dummy root] + 1, the opposite side follows the entered side in pre-order) -- the candidate stack
// holds no other edge, see run_parallel_dg for when that is enough.
// PS / BS: how psin and the range starts are read, each on its own (PrefixWords / PrefixRecords, common.hpp).
template <bool BLACK, class PS, class BS>
__global__ void k_top_bracket(uint32_t n, const uint32_t *__restrict__ gsize, const uint32_t *__restrict__ gpar,
			      const uint32_t *__restrict__ mpre, const BS bstart,
			      const SegTree segB, const uint32_t *__restrict__ tgtR,
			      const PS psin, uint32_t *__restrict__ ckey, uint32_t *__restrict__ cval,
			      uint32_t *__restrict__ lsz, uint32_t *__restrict__ err, const uint32_t *__restrict__ rid,
			      uint32_t first_simp_id, uint8_t *__restrict__ hpf, const uint32_t *__restrict__ seg_comp,
			      const uint32_t *__restrict__ c_ntree, const StackPlace sp, const LszField lf)
{
	const uint32_t q = BIDX * blockDim.x + threadIdx.x;
	if (q >= n)
		return;
	uint32_t v = n - 1 - q, c = 0;
	const uint32_t g = v;
	if (BLACK) {
		c = seg_comp[g];
		v = 2 * g + c + (c_ntree[c] & 1u) + 1;
	}
	uint32_t sz = gsize[v];
	if (sz == 0 || (!BLACK && gpar[v] == NIL)) { // (the far end of a black edge always has a parent: the entered side)
		cval[q] = v;
		ckey[q] = NIL;
		if (!BLACK)
			lsz[v] = 0;
		return;
	}
	// BLACK: everything downstream lives in candidate-stack order, so the sort carries the entry's stack index and the
	// entry itself (its tree vertex) is written here; lsz is indexed by stack position too -- and written only where the
	// size does not fit the field the payload has for it (LszField, par_kernels.hpp)
	uint32_t at = v;
	if (BLACK) {
		at = sp.soff[c] + (g - sp.voff[c]) + sp.shift[g];
		sp.s_vtx[at] = v; // (its component is looked up where it is needed: StackComp)
	}
	uint32_t m = mpre[v];
	uint32_t lo = bstart.at(m), hi = bstart.at(m + sz);
	// (The look-ups above and below were also tried as two batches ahead of the branch on the size -- mpre with gsize, then
	// the four sums, from indices an empty slot may read too: 1.160 against 1.178 ms, below what two runs of one build
	// differ by, and taken out again; profiles/class_payload_summary.md.)
	// Number of live brackets first (two prefix sums): in a chain of bubbles the brackets of everything below v are closed
	// inside their bubbles and the few live ones -- a simplifying edge, a tip's edge to the root -- come from the
	// deepest sources, i.e. sit at the END of the range.  When the last `live` entries are all live they are THE live
	// ones, and the top bracket is the first of them: no search at all.
	const uint32_t live = (hi - lo) - (psin.at(v + sz) - psin.at(v));
	uint32_t i = NIL;
	if (live >= 1 && live <= 4) { // (the four words in one 16-byte load; the array carries slack behind its last entry)
		const uint4 a = load4_unaligned(tgtR + (hi - live));
		const bool all = a.x < v && (live < 2 || a.y < v) && (live < 3 || a.z < v) && (live < 4 || a.w < v);
		if (all)
			i = hi - live;
	}
	// otherwise the top bracket often is one of the first few of the range: probe them (one load)
	// before falling back to the O(log n) descent
	if (i == NIL) {
		const uint32_t np = min(hi - lo, 4u);
		const uint4 a = load4_unaligned(tgtR + lo);
		if (np > 0 && a.x < v)
			i = lo;
		else if (np > 1 && a.y < v)
			i = lo + 1;
		else if (np > 2 && a.z < v)
			i = lo + 2;
		else if (np > 3 && a.w < v)
			i = lo + 3;
		if (i == NIL && lo + np < hi)
			i = seg_first_less(segB, lo + np, hi, v);
	}
	if (i == NIL) {
		atomicAdd(&err[PW_NO_BRACKET], 1u); // cannot happen: every list holds at least a simplifying bracket
		ckey[q] = NIL;
		cval[q] = at; // (nobody reads a payload or a list size behind a NIL key)
		if (!BLACK)
			lsz[at] = 0;
		return;
	}
	if (BLACK) {
		cval[q] = lf.pack(at, live);
		if (live >= lf.lmax)
			lsz[at] = live;
		// (Saturated entries are NOT counted here.  One atomic add per wave that has any, on one word, was measured: with
		// every entry saturated -- no field, 10^8 entries -- this kernel took 17.8 ms instead of 1.4.  Who wants the number
		// counts it from the sorted payload afterwards: count_saturated.)
	} else {
		cval[q] = at;
		lsz[at] = live;
	}
	ckey[q] = i;
	if (hpf && rid[i] >= first_simp_id) // the top bracket is a simplifying edge (flubbles.cpp:644-656)
		hpf[v] |= 2;
}
// (Tried in round 5 and dropped: the black-edge-only form with FOUR segment slots a lane -- component, shift, size and list
// position words in 16-byte loads, keys and stack indices in 16-byte stores.  3.43 ms against 1.86: the look-ups into the
// bracket list are chains of dependent gathers, and four of them one after the other in a lane cost more than the narrow
// loads of four lanes did; the wide form only pays in kernels that stream, gpurun_out r5l.)
// a bracket hands out a new class whenever the list size differs from the size it saw last
// (recent_size / recent_class, flubbles.cpp:668-676)
// (also row F's marks: q + 1 where the vertex at sorted position q ends a black edge, see k_next_from_runs)
// BLACK: n = V sorted entries, all of them black edges (no marks).
template <bool BLACK>
__global__ void k_class_flags(uint32_t n, uint32_t V, const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sval,
			      const uint32_t *__restrict__ lsz, const uint8_t *__restrict__ tf, uint8_t *__restrict__ flag,
			      uint32_t *__restrict__ dlt, uint32_t *__restrict__ mark)
{
	uint32_t q = BIDX * blockDim.x + threadIdx.x;
	if (!BLACK && q < V + 2)
		dlt[q] = 0; // row E's difference array, [V+2] (launched with max(n, V + 2) threads; BLACK: row E ran already)
	if (q >= n)
		return;
	uint32_t k = skey[q];
	if (k == NIL) {
		flag[q] = 0;
		if (!BLACK)
			mark[q] = 0;
		return;
	}
	const uint32_t v = sval[q];
	bool fresh = q == 0 || skey[q - 1] != k || lsz[sval[q - 1]] != lsz[v];
	flag[q] = fresh ? 1 : 0;
	if (!BLACK)
		mark[q] = (tf[v] & TF_BLACK) ? q + 1 : 0;
}
__global__ void k_class_scatter(uint32_t n, const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sval,
				const uint8_t *__restrict__ flag, const uint32_t *__restrict__ ps,
				uint32_t *__restrict__ gcls)
{
	uint32_t q = BIDX * blockDim.x + threadIdx.x;
	if (q >= n)
		return;
	const uint32_t cls = skey[q] == NIL ? NIL : ps[q] + flag[q] - 1; // inclusive scan - 1
	gcls[sval[q]] = cls; // (T-space = the per-component layout the debug hook reads)
}

// ------------------------------------------------------------- row E
// candidate-stack order = pre-order, except that under a branching entered side `a` the black
// child's subtree comes after the gray children's (tree_utils.cpp:47-76, flubbles.cpp:446-457).
// Only black edges enter the stack, and pre-order puts exactly one black vertex on every other position (segment slot
// g of component c <-> black vertex b = 2g + c + [dummy root] + 1, its parent a = b - 1): the whole permutation is
// worked out in units of black vertices, over the V segment slots.  subtree(b) holds (size + 1) / 2 black vertices,
// the gray children of a (size(a) - 1 - size(b)) / 2.
__global__ void k_shift_delta(uint32_t V, const uint32_t *__restrict__ seg_comp, const uint32_t *__restrict__ c_ntree,
			      const uint32_t *__restrict__ gsize, uint32_t *__restrict__ dlt)
{
	uint32_t g = BIDX * blockDim.x + threadIdx.x;
	if (g >= V)
		return;
	const uint32_t c = seg_comp[g], b = 2 * g + c + (c_ntree[c] & 1u) + 1, sb = gsize[b];
	if (sb == 0)
		return;
	const uint32_t sa = gsize[b - 1], gray = (sa - 1 - sb) / 2, black = (sb + 1) / 2;
	if (gray == 0)
		return;
	atomicAdd(&dlt[g], gray);		       // the black subtree moves behind the gray ones
	atomicAdd(&dlt[g + black], 0u - gray - black); // the gray subtrees move forward by the black one's entries
	atomicAdd(&dlt[g + sa / 2], black);
}
// the entry of every black edge, straight at its stack position (no flags, no compaction: a processed component's
// entries start at soff[c], a host-built table)
__global__ void k_stack_emit(uint32_t V, const uint32_t *__restrict__ seg_comp, const uint32_t *__restrict__ c_ntree,
			     const uint32_t *__restrict__ voff, const uint32_t *__restrict__ soff,
			     const uint32_t *__restrict__ dlt, const uint32_t *__restrict__ dlt_ps,
			     const uint32_t *__restrict__ gsize, const uint32_t *__restrict__ gcls,
			     uint32_t *__restrict__ s_vtx, uint32_t *__restrict__ s_cls,
			     uint32_t *__restrict__ sidx, uint32_t *__restrict__ ns, uint32_t *__restrict__ prev)
{
	uint32_t g = BIDX * blockDim.x + threadIdx.x;
	if (g >= V)
		return;
	const uint32_t c = seg_comp[g], b = 2 * g + c + (c_ntree[c] & 1u) + 1;
	if (gsize[b] == 0)
		return;
	const uint32_t i = soff[c] + (g - voff[c]) + dlt_ps[g] + dlt[g];
	s_vtx[i] = b;
	s_cls[i] = gcls[b];
	sidx[b] = i;
	ns[i] = i; // "no later occurrence" until k_next_from_runs says otherwise (flubbles.cpp:391-399)
	prev[i] = NIL;
}
// ------------------------------------------------------------- row F
// next_seen without another sort.  The class stage already grouped the tree vertices by top bracket
// with every group ordered from the deepest vertex up, and a class is a run inside a group.  The
// members of a class lie on one root-to-leaf path, so their order in the candidate stack is their
// order by depth: for consecutive BLACK members (deeper d, shallower u) of a run, next_seen[u] = d.
__global__ void k_next_from_runs(uint32_t T, const uint32_t *__restrict__ mark, const uint32_t *__restrict__ lastb,
				 const uint32_t *__restrict__ sval, const uint32_t *__restrict__ gcls,
				 const uint32_t *__restrict__ sidx, uint32_t *__restrict__ ns, uint32_t *__restrict__ prev)
{
	uint32_t q = BIDX * blockDim.x + threadIdx.x;
	if (q >= T || !mark[q])
		return;
	const uint32_t p = lastb[q]; // 1 + position of the previous black entry of the sorted order
	if (!p)
		return;
	const uint32_t u = sval[q], d = sval[p - 1];
	if (gcls[u] != gcls[d])
		return;
	const uint32_t iu = sidx[u], id = sidx[d];
	ns[iu] = id;
	prev[id] = iu;
}

// The flag byte of a candidate-stack entry: bit 0 = it opens a flubble (D), bit 1 = its class occurred before (U).
static constexpr uint32_t DF_OPENS = 1u, DF_SEEN = 2u;
// BLACK pass, all in one: next_seen / prev and the "opens a flubble" flag of the entry at sorted position q, written at
// its stack index (the sort's payload).  Consecutive entries of a run are consecutive members of a class (deeper
// first), so next_seen[u] = the entry before it in the run, prev[u] = the entry after it.  Nothing downstream needs the
// classes as numbers; the debug hooks number them on demand (k_class_ids_black).
__global__ void k_class_finish_black(uint32_t n, uint32_t S, const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sval,
				     const uint32_t *__restrict__ lsz, uint8_t *__restrict__ flag, uint32_t *__restrict__ ns,
				     uint32_t *__restrict__ prev, bool write_prev, uint8_t *__restrict__ dflag, const LszField lf)
{
	// prev is a word per entry at scattered addresses, and with exact classes all the walk asks of it is "is there one":
	// that goes into bit 1 (DF_SEEN) of the flag byte written anyway.  Only the laminarity check reads the word itself.
	// Four sorted positions a lane (the sorted keys, the stack indices and the flags move in 16-byte words), and the
	// "opens a new class" flags (k_class_flags<true>: a bracket hands out a new class whenever the list size differs from
	// the one it saw last, flubbles.cpp:668-676) are worked out right here, for the four and the one behind them.
	const uint32_t q0 = (BIDX * blockDim.x + threadIdx.x) * 4u;
	if (q0 == 0)
		dflag[S] = 0;
	if (q0 >= n)
		return;
	uint32_t K[6], U[6], L[6]; // positions q0 - 1 .. q0 + 4
	// (the neighbours' words leave with the lane's own: unconditional loads from clamped indices -- 0 <= q0 - 1 or 0, and
	// q0 + 4 or n - 1, all below n -- selected behind landed())
	const uint32_t qa = q0 ? q0 - 1 : 0u, qz = min(q0 + 4, n - 1);
	uint32_t ka = skey[qa], ua = sval[qa], kz = skey[qz], uz = sval[qz];
	if (q0 + 4 <= n) {
		const uint4 k4 = *reinterpret_cast<const uint4 *>(skey + q0), u4 = *reinterpret_cast<const uint4 *>(sval + q0);
		K[1] = k4.x, K[2] = k4.y, K[3] = k4.z, K[4] = k4.w;
		U[1] = u4.x, U[2] = u4.y, U[3] = u4.z, U[4] = u4.w;
	} else {
		for (uint32_t j = 1; j <= 4; j++) {
			K[j] = q0 + j - 1 < n ? skey[q0 + j - 1] : NIL;
			U[j] = q0 + j - 1 < n ? sval[q0 + j - 1] : 0u;
		}
	}
	landed(ka, ua, kz, uz);
	K[0] = q0 ? ka : NIL, U[0] = q0 ? ua : 0u;
	K[5] = q0 + 4 < n ? kz : NIL, U[5] = q0 + 4 < n ? uz : 0u;
	// The payload is the stack index under the list size (LszField); an invalid entry's payload is anything, and nothing
	// of it is used.  A size that filled its field is looked up: all six of a lane in one batch, behind one test the whole
	// wave agrees on -- in a chain of bubbles hardly a wave has one.  Two saturated neighbours compare their true sizes,
	// and a saturated size (>= lmax) differs from every unsaturated one by itself.
	bool sat[6], any_sat = false;
#pragma unroll
	for (int j = 0; j < 6; j++) {
		L[j] = K[j] != NIL ? lf.size(U[j]) : 0u;
		U[j] = lf.index(U[j]);
		sat[j] = K[j] != NIL && L[j] == lf.lmax;
		any_sat |= sat[j];
	}
	if (__any(any_sat)) {
		uint32_t t[6];
		// (gather_if, common.hpp; safe: lsz[q0], next to nothing in particular but the lane's own and always there -- q0 <
		// n <= V, and lsz has T + 2 > V words)
#pragma unroll
		for (int j = 0; j < 6; j++)
			t[j] = gather_if(sat[j], lsz, U[j], q0);
		landed(t[0], t[1], t[2], t[3], t[4], t[5]);
#pragma unroll
		for (int j = 0; j < 6; j++)
			L[j] = sat[j] ? t[j] : L[j];
	}
	bool fresh[6];
	fresh[0] = true;
#pragma unroll
	for (int j = 1; j < 6; j++)
		fresh[j] = (q0 + j - 1 == 0) || K[j - 1] != K[j] || L[j - 1] != L[j];
	uint32_t fw = 0;
#pragma unroll
	for (int j = 1; j <= 4; j++) {
		const uint32_t q = q0 + j - 1;
		if (q >= n || K[j] == NIL)
			continue; // (invalid entries carry NIL and sit behind every valid key: flag 0)
		const uint32_t u = U[j];
		fw |= (fresh[j] ? 1u : 0u) << (8 * (j - 1));
		const uint32_t nx = fresh[j] ? u : U[j - 1];
		ns[u] = nx;
		const bool seen = K[j + 1] != NIL && !fresh[j + 1];
		if (write_prev)
			prev[u] = seen ? U[j + 1] : NIL;
		// entry u opens a flubble iff its class comes back later than at the next entry
		dflag[u] = (uint8_t)(((u + 1 < nx) ? DF_OPENS : 0u) | (seen ? DF_SEEN : 0u));
	}
	if (q0 + 4 <= n) {
		*reinterpret_cast<uint32_t *>(flag + q0) = fw;
	} else {
		for (uint32_t j = 0; q0 + j < n; j++)
			flag[q0 + j] = (uint8_t)((fw >> (8 * j)) & 0xFFu);
	}
}
__global__ void k_class_ids_black(uint32_t n, const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sval,
				  const uint8_t *__restrict__ fresh, const uint32_t *__restrict__ ps, uint32_t *__restrict__ s_cls,
				  const LszField lf)
{
	uint32_t q = BIDX * blockDim.x + threadIdx.x;
	if (q < n && skey[q] != NIL)
		s_cls[lf.index(sval[q])] = ps[q] + fresh[q] - 1; // inclusive scan - 1 (the payload: the stack index under the list size)
}
// Entries of the sorted order whose list size filled its field (debug hook after a BLACK pass).  One atomic add per wave from a
// ballot, none when the wave has none; every lane of the workgroup gets here.
__global__ void k_count_saturated(uint32_t n, const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sval, const LszField lf,
				  uint32_t *__restrict__ count)
{
	const uint32_t q = BIDX * blockDim.x + threadIdx.x;
	const bool sat = q < n && skey[q] != NIL && lf.size(sval[q]) == lf.lmax;
	const unsigned long long sm = __ballot(sat);
	if (sm && (threadIdx.x & 63u) == 0)
		atomicAdd(count, (uint32_t)__popcll(sm));
}
// classes of the black tree vertices back in T-space (debug hook after a BLACK pass)
__global__ void k_cls_from_stack(uint32_t S, const uint32_t *__restrict__ s_vtx, const uint32_t *__restrict__ s_cls,
				 uint32_t *__restrict__ gcls)
{
	uint32_t i = BIDX * blockDim.x + threadIdx.x;
	if (i < S)
		gcls[s_vtx[i]] = s_cls[i];
}
// ------------------------------------------------------------- row G
// add_flubbles as a stack machine: at entry i, "class already open" pops through it and moves the
// PVST parent one level up (U, saturating at the root); a non-adjacent next occurrence emits a
// flubble and descends (D).  When the (prev, i) intervals are laminar the class is open iff it
// occurred before, so U/D are known per entry; a crossing pair sends the component to the
// sequential kernel instead.
// one kernel: the laminarity check of the (prev, i) intervals and the +-1 walk of the stack machine.
// Entry i takes two steps: U (-1 if its class was seen before) and then D (+1 if it opens a flubble).  The level of a
// new flubble is the walk's value after its D less the running minimum, and as D never goes down the minimum is
// always attained right after a U: the walk is kept at those points only, one word per entry, step(i) = D(i-1) + U(i).
// The walks of all components sit back to back in one array.  So that ONE unsegmented running minimum serves every
// component, the first step of component c also drops by B_c = 2 * (entries of the component before it) + 2: further
// than that component's walk can have climbed or fallen, so nothing in front of c ever is the minimum again (and the
// zero of component c is simply the walk's value at its first entry, whose own U is 0).
//
// CROSSING intervals (only possible when the literal hi_2 rule made the classes inexact, DESIGN.md section 4 "Row G").  The
// machine's U at entry i is "class(i) is on its stack", i.e. the entry pushed at p = prev[i] is still there: no entry k in
// (p, i) popped through a class that was pushed before p -- no k in (p, i) with prev[k] < p whose own class was open at k.
// With laminar intervals no such k exists and U = "has a previous occurrence".  Otherwise the entries whose interval holds
// a smaller prev are FLAGGED here (the range-min test), and k_resolve_crossings decides them, in stack order, one lane per
// component: U(i) = has-prev and not crossed(i), crossed(i) = some k in (p, i) with prev[k] < p that is not itself crossed
// (an unflagged entry with a previous occurrence is always open).  The U / D events are then the machine's own -- and they
// are all the PVST depends on --, so such a component needs no sequential redo (until round 4 it took one: 0.66 s per
// 10^6 segments).  tests/test_laminar_fuzz.py checks the rule against the machine on arbitrary label sequences.
__device__ __forceinline__ void laminar_check_one(uint32_t i, uint32_t p, const uint32_t *__restrict__ prev, const SegTree &segP,
						   uint8_t *__restrict__ xflag)
{
	if (p == NIL || p + 1 >= i)
		return;
	uint32_t lowest;
	if (i - p <= 9) { // a class that comes back within a few entries: its neighbours' words sit next to prev[i]
		lowest = NIL;
		for (uint32_t k = p + 1; k < i; k++)
			lowest = min(lowest, prev[k]);
	} else {
		lowest = seg_min(segP, p + 1, i);
	}
	if (lowest < p)
		xflag[i] = 1; // (cleared by the caller)
}
__global__ void k_laminar_walk(uint32_t S, const uint32_t *__restrict__ prev, const SegTree segP, bool check, const StackComp comp_of,
			       const uint32_t *__restrict__ soff, uint8_t *__restrict__ xflag, const uint8_t *__restrict__ dflag,
			       uint32_t *__restrict__ walk)
{
	// four entries a lane (one 4-byte load of their flag bytes and one 16-byte store: a kernel of a few loads per element is
	// bound by the memory instructions it issues).  U and D are bits of the flag bytes; where a component starts is a bit of
	// the component directory, and only there (a few thousand entries) the component in front is looked up.  prev is read
	// by the laminarity check alone.
	const uint32_t i0 = (BIDX * blockDim.x + threadIdx.x) * 4u;
	if (i0 >= S)
		return;
	// the drop in front of a component's first entry: further than the walk of the component before it can have moved
	auto drop = [&](uint32_t i) { return 2 * (i - soff[comp_of(i - 1)]) + 2; };
	if (i0 + 4 <= S) {
		const uint32_t d4 = *reinterpret_cast<const uint32_t *>(dflag + i0); // flags of the entries i0 .. i0 + 3
		const uint32_t dm = i0 ? dflag[i0 - 1] : 0u;
		const uint4 r = comp_of.rec[i0 >> 6]; // (i0 is a multiple of four: one record holds the four bits)
		const uint32_t starts = (((i0 & 32u) ? r.y : r.x) >> (i0 & 31u)) & 15u;
		const uint32_t dprev = (dm & DF_OPENS) | ((d4 & 0x00010101u) << 8); // byte j: D of the entry before entry i0 + j
		uint32_t w[4];
#pragma unroll
		for (uint32_t j = 0; j < 4; j++) {
			const uint32_t i = i0 + j;
			uint32_t step = ((d4 >> (8 * j)) & DF_SEEN) ? 0xFFFFFFFFu : 0u; // U: -1
			if (i > 0) {
				step += (dprev >> (8 * j)) & 1u; // D of the entry before
				if ((starts >> j) & 1u)
					step -= drop(i);
			}
			w[j] = step;
		}
		*reinterpret_cast<uint4 *>(walk + i0) = make_uint4(w[0], w[1], w[2], w[3]);
		if (check) { // (!check: the class stage was exact, the intervals are laminar by construction)
			const uint4 p4 = *reinterpret_cast<const uint4 *>(prev + i0);
			laminar_check_one(i0, p4.x, prev, segP, xflag);
			laminar_check_one(i0 + 1, p4.y, prev, segP, xflag);
			laminar_check_one(i0 + 2, p4.z, prev, segP, xflag);
			laminar_check_one(i0 + 3, p4.w, prev, segP, xflag);
		}
		return;
	}
	for (uint32_t i = i0; i < S; i++) {
		uint32_t step = (dflag[i] & DF_SEEN) ? 0xFFFFFFFFu : 0u; // U: -1
		if (i > 0) {
			step += dflag[i - 1] & DF_OPENS; // D of the entry before
			if (bitrank_test(comp_of.rec, i))
				step -= drop(i);
		}
		walk[i] = step;
		if (check)
			laminar_check_one(i, prev[i], prev, segP, xflag);
	}
}
// the flagged entries of every component, in stack order (xlist is ascending): crossed ones get xflag 2 and their U undone
__global__ void k_resolve_crossings(uint32_t C, const uint32_t *__restrict__ soff, const uint32_t *__restrict__ n_x,
				    const uint32_t *__restrict__ xlist, const uint32_t *__restrict__ prev, const SegTree segP,
				    uint8_t *xflag, uint32_t *__restrict__ walk, uint32_t *__restrict__ n_crossed)
{
	const uint32_t nx = *n_x;
	for (uint32_t c = BIDX * blockDim.x + threadIdx.x; c < C; c += gridDim.x * blockDim.x) {
		// this component's stretch of the list
		const uint32_t b = soff[c], e = soff[c + 1], lo = lower_bound(xlist, 0u, nx, b);
		uint32_t crossed = 0;
		for (uint32_t t = lo; t < nx; t++) {
			const uint32_t i = xlist[t];
			if (i >= e)
				break;
			const uint32_t p = prev[i];
			for (uint32_t k = p + 1;;) {
				k = seg_first_less(segP, k, i, p); // next entry inside (p, i) that reaches back beyond p
				if (k == NIL)
					break;
				if (xflag[k] != 2) { // it was open at k (prev[k] < p: it has a previous occurrence): it popped p's entry
					xflag[i] = 2;
					walk[i] += 1u; // the U of entry i does not happen
					crossed++;
					break;
				}
				k++;
			}
		}
		if (crossed)
			atomicAdd(n_crossed, crossed);
	}
}
// inclusive prefix sums of the walk, biased so that u32 order = int order; neg = their complement (a running
// maximum of the complement is the running minimum of the walk)
__global__ void k_walk_bias(uint32_t n, const uint32_t *walk, const uint32_t *ps, uint32_t *out, uint32_t *neg)
{
	const uint32_t k0 = (BIDX * blockDim.x + threadIdx.x) * 4u; // (in place on both arrays: a lane reads its four, then writes them)
	if (k0 >= n)
		return;
	if (k0 + 4 <= n) {
		const uint4 a = *reinterpret_cast<const uint4 *>(ps + k0), b = *reinterpret_cast<const uint4 *>(walk + k0);
		const uint4 w = make_uint4(a.x + b.x + 0x80000000u, a.y + b.y + 0x80000000u, a.z + b.z + 0x80000000u, a.w + b.w + 0x80000000u);
		*reinterpret_cast<uint4 *>(out + k0) = w;
		*reinterpret_cast<uint4 *>(neg + k0) = make_uint4(~w.x, ~w.y, ~w.z, ~w.w);
		return;
	}
	for (uint32_t k = k0; k < n; k++) {
		const uint32_t w = ps[k] + walk[k] + 0x80000000u;
		out[k] = w;
		neg[k] = ~w;
	}
}
// entry i opens a flubble iff its class comes back later than at the next entry (flubbles.cpp:344)
// (all-vertex class pass: next_seen and prev were scattered by k_next_from_runs; the flag byte takes both bits here)
__global__ void k_dflag(uint32_t S, const uint32_t *__restrict__ ns, const uint32_t *__restrict__ prev, uint8_t *__restrict__ dflag)
{
	uint32_t i = BIDX * blockDim.x + threadIdx.x;
	if (i < S)
		dflag[i] = (uint8_t)(((i + 1 < ns[i]) ? DF_OPENS : 0u) | (prev[i] != NIL ? DF_SEEN : 0u));
	if (i == S)
		dflag[S] = 0;
}
// The "opens a flubble" bits of the flag bytes as a bit-rank directory (common.hpp): "flubbles emitted in front of entry i"
// is then one 16-byte look-up into S / 4 bytes, where a 4-byte prefix per entry was written once and gathered by four
// kernels.  Four entries a lane, whole waves; positions from S on (stale bytes of an earlier, larger pass) read as 0.
__global__ void __launch_bounds__(TPB) k_pack_opens(uint32_t S, const uint8_t *__restrict__ dflag, uint4 *__restrict__ erec)
{
	const uint32_t i0 = (BIDX * blockDim.x + threadIdx.x) * 4u;
	uint32_t f = 0;
	if (i0 + 4 <= S) {
		const uint32_t d4 = *reinterpret_cast<const uint32_t *>(dflag + i0);
		f = (d4 & 1u) | ((d4 >> 7) & 2u) | ((d4 >> 14) & 4u) | ((d4 >> 21) & 8u);
	} else {
		for (uint32_t i = i0; i < S; i++)
			f |= (dflag[i] & DF_OPENS) << (i - i0);
	}
	const uint32_t w0 = (BIDX * blockDim.x + (threadIdx.x & ~63u)) / 16u; // first record of this wave's 256 entries
	bitrank_store_wave(erec + w0, f, w0 + (threadIdx.x & 63u) <= S / 64u);
}
// The component directory (StackComp, common.hpp): a bit where a non-empty component's entries start (the records were
// cleared), and, once the bits are ranked, the list of those components.  soff is the host's table; components that are not
// decomposed have empty ranges and leave no trace.
__global__ void k_comp_starts(uint32_t C, const uint32_t *__restrict__ soff, uint4 *__restrict__ crec)
{
	const uint32_t c = BIDX * blockDim.x + threadIdx.x;
	if (c >= C)
		return;
	const uint32_t i = soff[c];
	if (i < soff[c + 1])
		atomicOr(reinterpret_cast<uint32_t *>(crec + (i >> 6)) + ((i >> 5) & 1u), 1u << (i & 31u));
}
__global__ void k_comp_list(uint32_t C, const uint32_t *__restrict__ soff, const uint4 *__restrict__ crec, uint32_t *__restrict__ clist)
{
	const uint32_t c = BIDX * blockDim.x + threadIdx.x;
	if (c < C && soff[c] < soff[c + 1])
		clist[bitrank(crec, soff[c])] = c;
}
// Endpoints and orientations of every flubble straight into the (page-locked host) PVST arrays.  They only depend on
// the candidate stack and next_seen, so this kernel runs on the context's side stream while the main stream still
// computes levels and parents: the PCIe writes (10 of the 14 bytes per PVST vertex) hide behind that work.  A small
// grid-stride launch: a few ten thousand lanes keep the link busy and leave the CUs to the main stream.
__global__ void __launch_bounds__(TPB) k_emit_endpoints(uint32_t S, const uint4 *__restrict__ erec, const StackComp comp_of,
							 const uint32_t *__restrict__ ns,
							 const uint32_t *__restrict__ s_vtx, const uint8_t *__restrict__ tf,
							 const uint32_t *__restrict__ t_gid, const uint32_t *__restrict__ cproc_ps,
							 uint32_t *__restrict__ p_a, uint32_t *__restrict__ p_z, uint8_t *__restrict__ p_aor,
							 uint8_t *__restrict__ p_zor)
{
	// Only one entry in four or five opens a flubble.  A wave reads the flags of 256 entries (four bits a lane, out of their record),
	// lists the ones that do in LDS, and then every lane takes one of THOSE: the ten gathers behind an emitted flubble run
	// with full waves instead of waves that are four fifths idle.
	__shared__ uint32_t list[TPB / 64][256];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (uint32_t b0 = blockIdx.x * (4u * TPB); b0 < S; b0 += gridDim.x * (4u * TPB)) { // (uniform per workgroup: the barriers below are safe)
		const uint32_t i0 = b0 + wave * 256u + lane * 4u;
		uint32_t fl = 0; // (the directory holds no bits from S on, but its records end at S / 64)
		if (i0 < S) {
			const uint4 r = erec[i0 >> 6];
			fl = (((i0 & 32u) ? r.y : r.x) >> (i0 & 31u)) & 15u;
		}
		const uint32_t cnt = (uint32_t)__popc(fl);
		const uint32_t inc = wave_inclusive_sum(cnt);
		const uint32_t total = __shfl(inc, 63);
		uint32_t at = inc - cnt;
#pragma unroll
		for (uint32_t k = 0; k < 4; k++)
			if ((fl >> k) & 1u)
				list[wave][at++] = i0 + k;
		__syncthreads();
		for (uint32_t k = lane; k < total; k += 64) {
			const uint32_t i = list[wave][k];
			// dense output slot: flubbles emitted before + one root per earlier component, + 1 for this component's root
			const uint64_t q = (uint64_t)bitrank(erec, i) + cproc_ps[comp_of(i)] + 1;
			uint32_t va = s_vtx[i], vz = s_vtx[ns[i]];
			uint32_t ra = ((tf[va] & TF_TYPE_MASK) == 1) ? 0u : 1u, rz = ((tf[vz] & TF_TYPE_MASK) == 1) ? 0u : 1u;
			if (ra && rz) { // normalize_endpoints, flubbles.cpp:233-244
				p_a[q] = t_gid[vz];
				p_z[q] = t_gid[va];
				p_aor[q] = 0;
				p_zor[q] = 0;
			} else {
				p_a[q] = t_gid[va];
				p_z[q] = t_gid[vz];
				p_aor[q] = (uint8_t)ra;
				p_zor[q] = (uint8_t)rz;
			}
		}
		__syncthreads();
	}
}
// level of every emitted flubble
__global__ void k_levels(uint32_t S, const uint4 *__restrict__ erec, const StackComp comp_of, const uint32_t *__restrict__ soff,
			 const uint32_t *__restrict__ wb, const uint32_t *__restrict__ negmax,
			 uint32_t *__restrict__ lev, uint32_t *__restrict__ e_i)
{
	// four entries a lane: their record says which of them open a flubble (one in four or five does) and how many did
	// in front of them (the directory holds no bits from S on)
	const uint32_t i0 = (BIDX * blockDim.x + threadIdx.x) * 4u;
	if (i0 >= S)
		return;
	const uint4 r = erec[i0 >> 6];
	const unsigned long long bits = (unsigned long long)r.x | ((unsigned long long)r.y << 32);
	const uint32_t fl = (uint32_t)(bits >> (i0 & 63u)) & 15u;
	if (!fl)
		return;
	uint32_t j = r.z + (uint32_t)__popcll(bits & ((1ull << (i0 & 63u)) - 1ull));
#pragma unroll
	for (uint32_t k = 0; k < 4; k++) {
		if (!((fl >> k) & 1u))
			continue;
		const uint32_t i = i0 + k, c = comp_of(i), f0 = soff[c];
		// zero of this component's walk = its value at the component's first entry (after the drop B_c, before any U or D)
		const uint32_t zero = wb[f0];
		// running minimum up to i (negmax = exclusive running maximum of ~wb): everything in front of f0 lies above `zero`
		const uint32_t cur = wb[i], run = min(cur, ~negmax[i]);
		lev[j] = cur + 1 - min(zero, run); // depth of the new flubble (>= 1): the walk after this entry's own D
		e_i[j] = i;
		j++;
	}
}
// PVST parent of every flubble = nearest earlier flubble of its component with a smaller level
__global__ void k_pvst_emit(uint32_t NE, const uint32_t *__restrict__ lev, const uint32_t *__restrict__ e_i,
			    const SegTree segL, const StackComp comp_of, const uint32_t *__restrict__ doff,
			    const uint32_t *__restrict__ cproc_ps, uint32_t *__restrict__ p_parent)
{
	uint32_t j = BIDX * blockDim.x + threadIdx.x;
	if (j >= NE)
		return;
	// dense slot of the component's root (k_pvst_counts): flubbles emitted before + one root per earlier component
	const uint32_t i = e_i[j], c = comp_of(i);
	const uint64_t pb = doff[c];
	const uint32_t jb = (uint32_t)pb - cproc_ps[c]; // first flubble of the component
	uint32_t jp = seg_last_less(segL, jb, j, lev[j]);
	p_parent[pb + 1 + (j - jb)] = jp == NIL ? 0u : 1 + (jp - jb);
}
// per component: where its PVST starts in the dense output, its size, its stack entries -- everything the host needs for
// the forest's tree table, known as soon as the "opens a flubble" flags are ranked (before the result block exists)
__global__ void k_pvst_counts(uint32_t C, const uint32_t *__restrict__ c_ntree, const uint32_t *__restrict__ soff,
			      const uint4 *__restrict__ erec, const uint32_t *__restrict__ cproc_ps, uint32_t *__restrict__ doff,
			      uint32_t *__restrict__ c_npvst, uint32_t *__restrict__ c_nstack)
{
	uint32_t c = BIDX * blockDim.x + threadIdx.x;
	if (c > C)
		return;
	doff[c] = bitrank(erec, soff[c]) + cproc_ps[c];
	if (c == C)
		return;
	if (c_ntree[c] == 0) {
		c_npvst[c] = 0;
		return;
	}
	c_npvst[c] = 1 + (bitrank(erec, soff[c + 1]) - bitrank(erec, soff[c]));
	c_nstack[c] = soff[c + 1] - soff[c];
}
// the root vertex of every PVST (flubbles.cpp:736-741)
__global__ void k_pvst_roots(uint32_t C, const uint32_t *__restrict__ c_ntree, const uint32_t *__restrict__ doff,
			     uint32_t *__restrict__ p_parent, uint32_t *__restrict__ p_a, uint32_t *__restrict__ p_z,
			     uint8_t *__restrict__ p_aor, uint8_t *__restrict__ p_zor)
{
	uint32_t c = BIDX * blockDim.x + threadIdx.x;
	if (c >= C || c_ntree[c] == 0)
		return;
	const uint64_t pb = doff[c];
	p_parent[pb] = NIL;
	p_a[pb] = p_z[pb] = NIL;
	p_aor[pb] = p_zor[pb] = 0;
}
// copies of the parallel results into the per-component layout the debug hooks read
__global__ void k_export_stack(uint32_t S, const StackComp comp_of, const uint32_t *__restrict__ soff,
			       const uint32_t *__restrict__ voff, const uint32_t *__restrict__ s_vtx,
			       const uint32_t *__restrict__ s_cls, const uint32_t *__restrict__ ns,
			       uint32_t *__restrict__ o_vtx, uint32_t *__restrict__ o_cls, uint32_t *__restrict__ o_ns)
{
	uint32_t i = BIDX * blockDim.x + threadIdx.x;
	if (i >= S)
		return;
	uint32_t c = comp_of(i), l = i - soff[c], base = 2 * voff[c] + c;
	o_vtx[voff[c] + l] = s_vtx[i] - base;
	o_cls[voff[c] + l] = s_cls[i];
	o_ns[voff[c] + l] = ns[i] - soff[c];
}
// ------------------------------------------------------------- hairpin boundaries
// The reverse pre-order sweep opens a hairpin at every simplifying vertex (b1 = its segment), extends
// b2 while the top bracket is a simplifying edge, and closes it at the next leaf (or the root)
// (flubbles.cpp:531-535, 621-656).  Per closing vertex c the window of vertices processed since the
// previous closer is (c, prev closer]; everything is a "nearest flagged vertex" query.
__global__ void k_hp_inputs(uint32_t T, const uint32_t *__restrict__ gsize, const uint32_t *__restrict__ gpar,
			    const uint8_t *__restrict__ hpf, uint32_t *__restrict__ a_simp, uint32_t *__restrict__ a_q,
			    uint32_t *__restrict__ a_close)
{
	uint32_t v = BIDX * blockDim.x + threadIdx.x;
	if (v >= T)
		return;
	const uint32_t sz = gsize[v];
	const uint8_t f = sz ? hpf[v] : 0;
	const bool root = sz && gpar[v] == NIL;
	a_simp[v] = (sz && !root && (f & 1)) ? 0u : 1u;
	a_q[v] = (sz && !root && !(f & 1) && (f & 2)) ? 0u : 1u;
	a_close[v] = (sz && (root || sz == 1)) ? 0u : 1u;
}
__global__ void k_hp_close(uint32_t T, const uint32_t *__restrict__ gsize, const uint32_t *__restrict__ t_root,
			   const uint32_t *__restrict__ t_comp, const uint32_t *__restrict__ c_ntree,
			   const uint32_t *__restrict__ t_gid, const uint32_t *__restrict__ a_close,
			   const SegTree s1, const SegTree s2, const SegTree s3, uint8_t *__restrict__ push,
			   unsigned long long *__restrict__ b12)
{
	uint32_t c = BIDX * blockDim.x + threadIdx.x;
	if (c >= T)
		return;
	push[c] = 0;
	if (a_close[c])
		return;
	const uint32_t base = t_root[c], end = base + c_ntree[t_comp[c]];
	// previous closer in processing order = nearest closer with a larger idx
	const uint32_t cp = seg_first_less(s3, c + 1, end, 1u);
	const uint32_t hi = cp == NIL ? end : cp + 1; // window (c, hi)
	const uint32_t smin = seg_first_less(s1, c + 1, hi, 1u);
	if (smin == NIL)
		return; // no simplifying vertex since the previous closer: not in a hairpin
	const uint32_t smax = seg_last_less(s1, c + 1, hi, 1u);
	const uint32_t q = seg_first_less(s2, c + 1, smax, 1u);
	push[c] = 1;
	b12[2 * (size_t)c] = t_gid[smin];
	b12[2 * (size_t)c + 1] = q == NIL ? (unsigned long long)NIL : (unsigned long long)t_gid[q];
	(void)gsize;
}
// boundaries are reported in processing order: closers by descending idx inside a component
__global__ void k_hp_emit(uint32_t T, const uint8_t *__restrict__ push, const uint32_t *__restrict__ ps,
			  const uint32_t *__restrict__ t_root, const uint32_t *__restrict__ t_comp,
			  const uint32_t *__restrict__ c_ntree, const uint32_t *__restrict__ voff,
			  const unsigned long long *__restrict__ b12, unsigned long long *__restrict__ out,
			  uint32_t *__restrict__ c_nbry)
{
	uint32_t c = BIDX * blockDim.x + threadIdx.x;
	if (c >= T)
		return;
	const uint32_t ci = t_comp[c];
	if (ci == NIL)
		return;
	const uint32_t base = t_root[c], end = base + c_ntree[ci];
	if (c == base && c_ntree[ci])
		c_nbry[ci] = ps[end] - ps[base];
	if (!push[c])
		return;
	const uint32_t after = ps[end] - ps[c + 1]; // pushes of this component with a larger idx come first
	const uint64_t pb = (uint64_t)voff[ci] + ci;
	out[2 * (pb + after)] = b12[2 * (size_t)c];
	out[2 * (pb + after) + 1] = b12[2 * (size_t)c + 1];
}

void run_parallel_hairpins(const CompState &cs, SeqWs &sw, ParWs &pw, uint32_t C, StageTimer &tm, hipStream_t s)
{
	const uint32_t T = 2 * sw.V + C;
	tm.begin("par_hairpins");
	LAUNCH(k_hp_inputs, T, s, T, pw.gsize, pw.gpar, pw.hpf, pw.hp1, pw.hp2, pw.hp3);
	seg_build(pw.segH1, pw.hp1, T, s);
	seg_build(pw.segH2, pw.hp2, T, s);
	seg_build(pw.segH3, pw.hp3, T, s);
	uint8_t *push = pw.f8a;
	uint32_t *pps = pw.psA;
	unsigned long long *b12 = pw.hp_b12; // [2T] boundary pairs
	if (!b12 || !pw.hpf || !pw.t_comp)
		throw HipError("hairpin report: its arrays were not carved (internal)");
	LAUNCH(k_hp_close, T, s, T, pw.gsize, pw.t_root, pw.t_comp, sw.c_ntree, sw.t_gid, pw.hp3, pw.segH1, pw.segH2, pw.segH3, push,
	       b12);
	scan_exclusive_u8(push, pps, (size_t)T + 1, nullptr, nullptr, 0, pw.scan_tmp, pw.scan_tmp_bytes, s);
	LAUNCH(k_hp_emit, T, s, T, push, pps, pw.t_root, pw.t_comp, sw.c_ntree, cs.voff, b12, (unsigned long long *)sw.hairpins,
	       sw.c_nbry);
	tm.end(10);
}

// ------------------------------------------------------------- workspace
static void for_each_span(ParWs &pw, size_t V, size_t E, size_t Cmax, int groups, const StageWsOpts &o, Spans &spans)
{
	// Group 1: what the TREE stage already writes (its tree arrays in the layout the class stage reads, the back edges, the
	// scratch of the primitives).  Group 2: everything first written by the class stage and later -- by then the tree
	// stage's own workspace is dead but for a few arrays (tree_spans, group 1), and group 2 lies over the rest of it
	// (stage_workspace_carve).
	auto take1 = [&](size_t n, auto *&...p) {
		if (groups & 1)
			spans(n, p...);
	};
	auto take = [&](size_t n, auto *&...p) {
		if (groups & 2)
			spans(n, p...);
	};
	// brackets: the back edges of from_bd (links outside the tree, one per side without links) and, per tree vertex, at most
	// ONE edge of the class stage -- a capping edge needs a non-empty bracket list, a simplifying edge an empty one
	const size_t T = 2 * V + Cmax, NB = o.nb_cap ? std::min(o.nb_cap, E + V + T) : E + V + T, S = V + 1;
	pw.nb_cap = NB;
	auto skip = [](auto **p) { *p = nullptr; };
	take1(T + 2, pw.hi0, pw.mpre, pw.dlt, pw.incnt, pw.lsz);
	if (groups & 1) { // the byte forms of the three bracket counts, inside the word arrays they stand in for (see ParWs)
		pw.ordcnt8 = reinterpret_cast<uint8_t *>(pw.lsz);
		pw.srccnt8 = reinterpret_cast<uint8_t *>(pw.dlt);
		pw.incnt8 = reinterpret_cast<uint8_t *>(pw.incnt);
	}
	take1(NB + 2, pw.b_src, pw.b_tgt, pw.b_ord);
	take1(V + 4, pw.sdl);
	take1(PASS_WORDS, pw.err);
	take1(Cmax + 2, pw.comp_bad); // (zeroed when the pass starts, ahead of the tree stage)
	pw.scan_tmp_bytes = std::max(scan_tmp_bytes(std::max(T, NB) + 4), 2 * compact_tmp_bytes(std::max(T, NB) + 4));
	pw.sort_tmp_bytes = sort_tmp_bytes(std::max(std::max(T, NB), std::max(4 * V, 2 * E) + 8) + 4);
	take1(pw.scan_tmp_bytes, pw.scan_tmp);
	take1(pw.sort_tmp_bytes, pw.sort_tmp);
	for (uint32_t **p : {&pw.t_comp, &pw.t_root, &pw.gpar, &pw.gsize, &pw.cov}) {
		if (o.full_t)
			take(T + 2, *p);
		else if (groups & 2)
			skip(p);
	}
	take(T + 2, pw.psA, pw.psB, pw.flagC, pw.psC, pw.cap_tgt, pw.dlt_ps, pw.psin, pw.topi, pw.gcls, pw.vals_t, pw.vals_t2);
	take(T + 32, pw.f8a, pw.f8b, pw.f8c, pw.f8d);
	take(T + 2, pw.keys_t, pw.keys_t2);
	take(Cmax + 2, pw.dbo);
	take(NB + 2, pw.b_val2, pw.tgtR);
	for (uint32_t **p : {&pw.b_val, &pw.b_key, &pw.b_key2}) { // (the bracket sort: only behind a sequential tree stage)
		if (o.sorted_brackets)
			take(NB + 2, *p);
		else if (groups & 2)
			skip(p);
	}
	take(S + 2, pw.s_vtx, pw.s_cls, pw.ns, pw.prev, pw.lev, pw.e_i);
	// the two directories over the stack positions [0, S]: S / 64 + 1 records and the closing one (+ one of slack)
	take(S / 64 + 3, pw.erec, pw.crec);
	take(S / 64 + 3, pw.rk_cnt);
	take(Cmax + 2, pw.clist);
	take(S + 4, pw.walk, pw.walk_ps, pw.wrun);
	take(Cmax + 2, pw.cproc_ps, pw.doff);
	take(SegTree::tree_words(T + 1), pw.segA.tree);
	take(SegTree::tree_words(NB + 1), pw.segB.tree);
	take(SegTree::tree_words(S + 1), pw.segP.tree, pw.segL.tree);
	take(forest_wire::PvstArrays::bound(S + Cmax + 2) + 256, pw.stage); // (a PVST block of every stack entry and one root per component)
	if (o.hairpins) {
		take(2 * T + 4, pw.hp_b12);
		take(T + 2, pw.hpf);
		take(T + 2, pw.hp1, pw.hp2, pw.hp3);
		take(SegTree::tree_words(T + 1), pw.segH1.tree, pw.segH2.tree, pw.segH3.tree);
	} else if (groups & 2) {
		pw.hpf = nullptr;
		pw.hp_b12 = nullptr;
		pw.hp1 = pw.hp2 = pw.hp3 = nullptr;
		pw.segH1.tree = pw.segH2.tree = pw.segH3.tree = nullptr;
	}
}

size_t par_workspace_bytes(size_t V, size_t E, size_t Cmax, int groups, const StageWsOpts &o)
{
	ParWs tmp{};
	return measure([&](Spans &take) { for_each_span(tmp, V, E, Cmax, groups, o, take); }) + (1 << 20);
}

void par_carve(Arena &ar, ParWs &pw, size_t V, size_t E, size_t Cmax, int groups, const StageWsOpts &o)
{
	Spans take{&ar};
	for_each_span(pw, V, E, Cmax, groups, o, take);
}

// ------------------------------------------------------------- overlays
// Every array of ParWs that the class stage uses under another type or meaning than the one it is declared with, named
// once.  Next to each view: the array under it, and from which kernel to which the view is live (the array's earlier or
// later tenant in brackets).  The steps below address these arrays through the views only.
struct ClassViews {
	// ---- row D, up to the placing of the brackets
	uint4 *brec;	      // psA: bridge flags as a bit-rank directory over T + 1 positions ((T / 64 + 2) records = T / 4 + 32 bytes); k_bridge_flags -> k_capping [then cps]
	uint32_t *brec_cnt;   // f8a: the counts its build scans ((T / 64 + 2) words); inside bitrank_build only [then cflag]
	uint32_t *pscov;      // psB: scan of the coverage differences; the difference scan -> k_bridge_flags [then tsimp]
	uint8_t *simp, *capf; // f8b, f8c: [T+1] simplifying / capping vertex; k_hi_simp, k_capping -> k_bracket_place [capf: then dflag]
	uint32_t *br_list;    // vals_t: the bridge vertices, listed; k_hi_simp -> k_capping [then the class sort's values, k_top_bracket]
	uint32_t *tsimp, *tcap; // psB, psC: simplifying / capping vertices per tile of k_bracket_extra, scanned in place [ntiles + 1], totals in the last word; k_flag_tile_counts -> k_bracket_extra [psC: then lastb]
	uint32_t *srccnt;     // dlt: brackets per mirror pre-order position, as words; k_globalize / k_tree_emit -> the scan of the range starts [then row E's differences]
	uint32_t *bstart;     // dlt_ps: first bracket of every position, as words or (byte counts) as count records in the same span; that scan -> k_top_bracket [all vertices: then the scan of row E's differences]
	// ---- classes and rows E, F
	uint32_t *ck, *ck2;   // keys_t, keys_t2: keys of the class sort; k_top_bracket -> the class kernels (and stack_class_ids after a black-only pass)
	uint8_t *cflag;	      // f8a: "opens a class" per sorted entry; the class kernels -> k_class_scatter / stack_class_ids [before: brec_cnt]
	uint32_t *cps;	      // psA: its scan [before: brec]
	uint8_t *dflag;	      // f8c: [S+1] <= [T+1] opens / seen flags of the stack entries; k_class_finish_black / k_dflag -> k_laminar_walk [before: capf]
	uint32_t *shift_ps;   // topi: black only: INCLUSIVE scan of row E's differences (dlt_ps still holds the bracket range starts; nobody needs vertex -> stack index there) [all vertices: topi itself, k_stack_emit]
	uint32_t *mark, *lastb; // flagC, psC: all vertices: run marks (written with the class flags) and their running maximum; k_class_flags -> k_next_from_runs [psC before: tcap]
	// ---- row G
	uint8_t *xflag;	      // f8d: [T + 32] >= S entries whose interval is crossed; the memset -> k_resolve_crossings [the branching flags are long compacted]
	uint32_t *xlist;      // wrun: those entries, listed; compact_flagged_u8 -> k_resolve_crossings [then wrun itself]
	uint32_t *wb;	      // walk_ps: in place, exclusive -> biased inclusive; k_walk_bias -> k_levels
	uint32_t *wneg;	      // walk: the steps are dead once k_walk_bias has read them; k_walk_bias -> the max scan
	uint32_t *wrun;	      // wrun: running minimum (complemented); the max scan -> k_levels
};
static ClassViews class_views(const ParWs &pw)
{
	ClassViews v;
	v.brec = reinterpret_cast<uint4 *>(pw.psA);
	v.brec_cnt = reinterpret_cast<uint32_t *>(pw.f8a);
	v.pscov = pw.psB;
	v.simp = pw.f8b, v.capf = pw.f8c;
	v.br_list = pw.vals_t;
	v.tsimp = pw.psB, v.tcap = pw.psC;
	v.srccnt = pw.dlt, v.bstart = pw.dlt_ps;
	v.ck = pw.keys_t, v.ck2 = pw.keys_t2;
	v.cflag = pw.f8a, v.cps = pw.psA;
	v.dflag = pw.f8c;
	v.shift_ps = pw.topi;
	v.mark = pw.flagC, v.lastb = pw.psC;
	v.xflag = pw.f8d;
	v.xlist = pw.wrun;
	v.wb = pw.walk_ps, v.wneg = pw.walk, v.wrun = pw.wrun;
	return v;
}

// ------------------------------------------------------------- driver
// Everything the host needs to know about a finished pass, written straight into page-locked host
// memory (PassSummary).
__global__ void k_summary(uint32_t C, const uint32_t *__restrict__ err, const uint32_t *__restrict__ bad,
			  const uint32_t *__restrict__ status, const uint32_t *__restrict__ npvst,
			  const uint32_t *__restrict__ nbry, const uint32_t *__restrict__ doff, uint32_t *__restrict__ out)
{
	uint32_t i = BIDX * blockDim.x + threadIdx.x;
	if (i > C)
		return;
	const PassSummary o(C, out);
	if (i == 0) {
		o.err(PassSummary::NO_BRACKET) = err ? err[PW_NO_BRACKET] : 0;
		o.err(PassSummary::WALK_POOL) = err ? err[PW_WALK_POOL] : 0;
		o.err(PassSummary::FOREST_SIZE) = err ? err[PW_FOREST_SIZE] : 0;
		o.err(PassSummary::SPARE) = 0;
	}
	if (i < C) {
		o.bad(i) = bad ? bad[i] : 0;
		o.status(i) = status[i];
		o.npvst(i) = npvst[i];
		o.nbry(i) = nbry[i];
	}
	o.doff(i) = doff ? doff[i] : 0;
}

void pass_summary(const SeqWs &sw, const ParWs *pw, uint32_t C, uint32_t *host_out, hipStream_t s)
{
	uint32_t *dev_out = nullptr;
	HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void **>(&dev_out), host_out, 0));
	LAUNCH(k_summary, (size_t)C + 1, s, C, pw ? pw->err : nullptr, pw ? pw->comp_bad : nullptr, sw.c_status, sw.c_npvst,
	       sw.c_nbry, pw ? pw->doff : nullptr, dev_out);
}

// One pass of rows D-G: what run_parallel_dg's steps share.  The steps run in the order they stand in, each between the
// stage timer's marks it names; the routes are decided once, at the top.
struct ClassPass {
	const CompState &cs;
	SeqWs &sw;
	ParWs &pw;
	StageTimer &tm;
	hipStream_t s;
	const SideStream &side;
	PassTail &tail;
	const std::function<void *(size_t)> &alloc_result_block;
	const ClassViews v;
	const uint32_t C, V, T, S, n_processed; // components, segments, tree-vertex slots, candidate-stack entries, processed components
	const int64_t dense_nb0;
	// ---- the routes
	const bool dense;     // the parallel tree stage left the back edges in b_src / b_tgt (else: a sequential tree stage, densified here)
	const bool want_hp;   // the hairpin report follows
	// All-parallel pass: the tree stage wrote sizes (0 = no vertex in this slot), parents (only ever tested against NIL), the
	// mirror pre-order and the cleared bracket counts in T-space itself; the root of a vertex's tree is looked up where it
	// is needed.  A sequential tree stage works per component: its arrays are brought into that form here, and the
	// hairpin report wants the per-vertex tables too.
	const bool lean;
	const bool narrow_oc, narrow_sc, narrow_ic; // the bracket counts of the parallel tree stage as bytes (it wrote them in the form the caller chose, see ParWs)
	// psin / the range starts as count records (the spans of psin / dlt_ps hold them): exactly where the scan's input is a byte
	// array, unless PassHooks::word_prefix (POVU_HIP_WORD_PREFIX, an A/B hook) says words: 1 = both, 2 = psin, 3 = the range starts
	const int word_prefix;
	const bool rec_ps, rec_bs;
	// bits of the class sort's payload that carry the list size in a black-only pass (LszField, par_kernels.hpp), at most:
	// PassHooks::lsz_field (POVU_HIP_LSZ_FIELD, an A/B hook) lowers the cap, 0 = the bare stack index and every size looked up
	const unsigned lsz_cap;
	bool black_only = false;	 // classes of the black tree edges only (place_brackets decides)
	const RootOf root_of;
	// ---- counts: ordinary / capping / simplifying back edges, all brackets, vertices that get a class
	uint32_t NB0 = 0, ncap = 0, nsimp = 0, NB = 0, NC = 0;
	const uint32_t ntiles; // tiles of k_bracket_extra
	// ---- words on their way to the host
	uint32_t *extra = nullptr; // [5] capping count | simplifying count | literal-rule flag | back edges of the tree stage | a byte of incnt8 overflowed
	HostScratch::Token extra_ready = 0;
	uint32_t *early = nullptr; // pass_summary's words as of the PVST count
	HostScratch::Token early_ready = 0;
	bool use_side = false; // the endpoints and the copies go to the side stream

	ClassPass(const CompState &cs_, SeqWs &sw_, ParWs &pw_, uint32_t C_, uint32_t n_processed_, uint32_t n_stack, int64_t dense_nb0_,
		  const PassHooks &hooks, const std::function<void *(size_t)> &alloc, StageTimer &tm_, hipStream_t s_, const SideStream &side_, PassTail &tail_)
		: cs(cs_), sw(sw_), pw(pw_), tm(tm_), s(s_), side(side_), tail(tail_), alloc_result_block(alloc), v(class_views(pw_)), C(C_),
		  V(sw_.V), T(2 * sw_.V + C_), S(n_stack), n_processed(n_processed_), dense_nb0(dense_nb0_), dense(dense_nb0_ >= 0),
		  want_hp(sw_.hairpins != nullptr), lean(dense && !want_hp), narrow_oc(dense && pw_.narrow_ordcnt),
		  narrow_sc(narrow_oc && pw_.narrow_srccnt), narrow_ic(narrow_sc && pw_.narrow_incnt),
		  word_prefix(hooks.word_prefix), rec_ps(narrow_ic && word_prefix != 1 && word_prefix != 2),
		  rec_bs(narrow_sc && word_prefix != 1 && word_prefix != 3),
		  lsz_cap(hooks.lsz_field), root_of{lean ? nullptr : pw_.t_root, cs_.voff, C_},
		  ntiles((T + BX_TILE - 1) / BX_TILE)
	{
	}
	void scan(const uint32_t *in, uint32_t *out, size_t n) const { scan_exclusive_u32(in, out, n, pw.scan_tmp, pw.scan_tmp_bytes, s); }
	void scan8(const uint8_t *in, uint32_t *out, size_t n) const
	{
		scan_exclusive_u8(in, out, n, nullptr, nullptr, 0, pw.scan_tmp, pw.scan_tmp_bytes, s);
	}
	void scan8pair(const uint8_t *in0, uint32_t *out0, size_t n0, const uint8_t *in1, uint32_t *out1, size_t n1) const
	{
		scan_exclusive_u8(in0, out0, n0, in1, out1, n1, pw.scan_tmp, pw.scan_tmp_bytes, s);
	}
	uint4 *psin_rec() const { return reinterpret_cast<uint4 *>(pw.psin); }
	uint4 *bstart_rec() const { return reinterpret_cast<uint4 *>(v.bstart); }
	// f(psin's view, the range starts' view): the four forms of the kernels that read them
	template <class F>
	void with_prefix_views(F &&f) const
	{
		if (rec_ps && rec_bs)
			f(PrefixRecords{psin_rec()}, PrefixRecords{bstart_rec()});
		else if (rec_ps)
			f(PrefixRecords{psin_rec()}, PrefixWords{v.bstart});
		else if (rec_bs)
			f(PrefixWords{pw.psin}, PrefixRecords{bstart_rec()});
		else
			f(PrefixWords{pw.psin}, PrefixWords{v.bstart});
	}
	void scan2(const uint32_t *in0, uint32_t *out0, size_t n0, const uint32_t *in1, uint32_t *out1, size_t n1) const
	{
		scan_exclusive_u32_pair(in0, out0, n0, in1, out1, n1, pw.scan_tmp, pw.scan_tmp_bytes, s);
	}
};

// ---- T-space + dense back edges.  Reads the tree stage's arrays in sw (lean: in place); writes gpar / gsize / t_root /
// hi0 / mpre and the cleared counts when not lean, b_src / b_tgt behind a sequential tree stage.
static void t_space_setup(ClassPass &P)
{
	ParWs &pw = P.pw;
	const SeqWs &sw = P.sw;
	const CompState &cs = P.cs;
	hipStream_t s = P.s;
	const uint32_t V = P.V, T = P.T, C = P.C;
	P.tm.begin("par_setup");
	if (P.lean) {
		pw.gsize = sw.t_size;
		pw.gpar = sw.t_par;
	} else {
		LAUNCH(k_tcomp_vertices, V, s, V, T, cs.ckey, cs.voff, pw.t_comp);
		LAUNCH(k_globalize, T, s, T, pw.t_comp, cs.voff, sw.c_ntree, sw.t_par, sw.t_size, pw.gpar, pw.gsize, pw.t_root, pw.hi0,
		       P.dense ? nullptr : pw.cov, sw.t_depth, pw.mpre, pw.incnt, P.narrow_sc ? nullptr : pw.dlt, sw.t_flags);
	}
	// pw.comp_bad and pw.err are zeroed by the caller (zero_component_counters)
	if (P.dense) { // the parallel tree stage already left the back edges in b_src / b_tgt
		P.NB0 = P.dense_nb0 == NB0_ON_DEVICE ? 0u : (uint32_t)P.dense_nb0; // (on the device: read in place_brackets, nothing before that needs it)
	} else {
		P.scan(sw.c_nbe0, pw.dbo, (size_t)C + 1);
		P.NB0 = pw.host->read_u32(pw.dbo + C, s);
		LAUNCH(k_dense_be, P.NB0, s, P.NB0, C, pw.dbo, cs.voff, cs.eoff, sw.be_src, sw.be_tgt, pw.b_src, pw.b_tgt);
	}
	P.tm.end(7);
}

// the five words of ClassPass::extra on their way to the host, in one launch
static void publish_extra(ClassPass &P)
{
	ParWs &pw = P.pw;
	P.extra = pw.host->take<uint32_t>(5);
	publish_words(P.extra, WordSrc{{P.v.tcap + P.ntiles, P.v.tsimp + P.ntiles, pw.err + PW_LITERAL_RULE, pw.err + PW_NB0, pw.err + PW_INCNT_OVF}}, 5, P.s);
	P.extra_ready = pw.host->mark(P.s);
}

// ---- row D, first half: bridge flags, simplifying and capping vertices, and their counts on the way to the host.  Reads
// hi0, the coverage counts (ordcnt8 / lsz and incnt, or cov), gsize, the root bits of t_flags; writes segA, brec, simp, capf, cap_tgt, br_list,
// tsimp, tcap and the words PW_N_BRIDGE, PW_LITERAL_RULE.
static void bridge_and_capping(ClassPass &P)
{
	ParWs &pw = P.pw;
	const ClassViews &v = P.v;
	hipStream_t s = P.s;
	const uint32_t T = P.T, ntiles = P.ntiles;
	P.tm.begin("par_classes");
	if (!P.dense)
		LAUNCH(k_hi0, P.NB0, s, P.NB0, pw.b_src, pw.b_tgt, pw.hi0, pw.cov, nullptr);
	seg_build(pw.segA, pw.hi0, T, s);
	if (P.narrow_ic) // back edges leaving a vertex minus those arriving (both counted by the tree stage; as bytes: not those that arrive at a root)
		scan_exclusive_diff_u8_u8(pw.ordcnt8, pw.incnt8, v.pscov, (size_t)T + 1, pw.scan_tmp, pw.scan_tmp_bytes, s);
	else if (P.narrow_oc)
		scan_exclusive_diff_u8_u32(pw.ordcnt8, pw.incnt, v.pscov, (size_t)T + 1, pw.scan_tmp, pw.scan_tmp_bytes, s);
	else if (P.dense)
		scan_exclusive_diff_u32(pw.lsz, pw.incnt, v.pscov, (size_t)T + 1, pw.scan_tmp, pw.scan_tmp_bytes, s);
	else
		P.scan(pw.cov, v.pscov, (size_t)T + 1);
	KLAUNCH(k_bridge_flags, dim3(nblk(((size_t)T / 256 + 1) * 64)), dim3(TPB), 0, s, T, pw.gsize, P.sw.t_flags, v.pscov, v.brec); // (whole waves: every record of [0, T] is written)
	bitrank_build(v.brec, (size_t)T / 64 + 1, v.brec_cnt, pw.scan_tmp, pw.scan_tmp_bytes, s);
	uint32_t *n_br = pw.err + PW_N_BRIDGE;
	KLAUNCH(k_hi_simp, dim3((unsigned)(((size_t)T + HS_VERTS - 1) / HS_VERTS)), dim3(TPB), 0, s, T, pw.gsize, v.brec, v.simp, P.want_hp ? pw.hpf : nullptr, v.capf, v.br_list,
		n_br);
	KLAUNCH(k_capping, dim3(std::min<unsigned>(nblk(T / 8 + 1), 16384)), dim3(TPB), 0, s, n_br, v.br_list, pw.gsize, pw.hi0, v.brec, P.root_of,
		pw.segA, pw.cap_tgt, v.capf, pw.err + PW_LITERAL_RULE, T + 2); // (hi0 is carved with T + 2 words: for_each_span)
	// capping / simplifying vertices per tile of k_bracket_extra, scanned: [ntiles + 1] each, the totals in the last word
	KLAUNCH(k_flag_tile_counts, dim3((ntiles + 1 + 15) / 16 + 1), dim3(TPB), 0, s, T, v.capf, v.simp, v.tcap, v.tsimp, ntiles);
	scan_exclusive_u32_pair(v.tsimp, v.tsimp, (size_t)ntiles + 1, v.tcap, v.tcap, (size_t)ntiles + 1, pw.scan_tmp, pw.scan_tmp_bytes, s);
	// The stream is not left idle while the host reads them (HostScratch::mark): the kernel that places the capping and
	// simplifying brackets takes the counts from the device, and the scan behind it does not need them at all.
	// (byte in-counts: the words go out behind that kernel, which may raise the last of them; the scan still covers the read)
	if (!P.narrow_ic)
		publish_extra(P);
}

// ---- row D, second half: the capping and simplifying brackets join the ordinary ones (b_src / b_tgt, the two counts),
// then, with the counts on the host, every bracket goes to its place in the bracket lists (tgtR, segB; b_val2 for the
// hairpin report).  Decides black_only.  False: the byte in-counts overflowed, the pass must be repeated with words.
static bool place_brackets(ClassPass &P)
{
	ParWs &pw = P.pw;
	const ClassViews &v = P.v;
	hipStream_t s = P.s;
	const uint32_t T = P.T;
	auto bracket_extra = [&](auto *ordcnt, auto *sc, auto *ic) {
		using OC = std::remove_const_t<std::remove_pointer_t<decltype(ordcnt)>>;
		using SC = std::remove_pointer_t<decltype(sc)>;
		using IC = std::remove_pointer_t<decltype(ic)>;
		LAUNCH((k_bracket_extra<OC, SC, IC>), ((size_t)T + 3) / 4, s, T, P.NB0, P.dense_nb0 == NB0_ON_DEVICE ? pw.err + PW_NB0 : nullptr, P.ntiles,
		       (uint32_t)std::min<size_t>(pw.nb_cap, 0xFFFFFFFFu), v.capf, v.tcap, v.simp, v.tsimp, pw.cap_tgt, P.root_of, pw.b_src, pw.b_tgt,
		       ordcnt, pw.gsize, pw.mpre, ic, sc, P.sw.t_flags, pw.err + PW_INCNT_OVF);
	};
	if (P.narrow_ic)
		bracket_extra((const uint8_t *)pw.ordcnt8, pw.srccnt8, pw.incnt8);
	else if (P.narrow_sc)
		bracket_extra((const uint8_t *)pw.ordcnt8, pw.srccnt8, pw.incnt);
	else if (P.narrow_oc)
		bracket_extra((const uint8_t *)pw.ordcnt8, v.srccnt, pw.incnt);
	else
		bracket_extra(P.dense ? (const uint32_t *)pw.lsz : nullptr, v.srccnt, pw.incnt);
	if (P.narrow_ic)
		publish_extra(P);
	// ranks inside every source and the counts per source are known: place directly
	// (byte counts: as count records, a third of the words' size, in the words' spans -- each array on its own under the A/B hook)
	const size_t n1 = (size_t)T + 1;
	if (P.rec_ps && P.rec_bs) {
		scan_count_records_u8(pw.incnt8, P.psin_rec(), n1, pw.srccnt8, P.bstart_rec(), n1, pw.scan_tmp, pw.scan_tmp_bytes, s);
	} else if (P.rec_ps) {
		scan_count_records_u8(pw.incnt8, P.psin_rec(), n1, nullptr, nullptr, 0, pw.scan_tmp, pw.scan_tmp_bytes, s);
		P.scan8(pw.srccnt8, v.bstart, n1);
	} else if (P.rec_bs) {
		if (P.narrow_ic)
			P.scan8(pw.incnt8, pw.psin, n1);
		else
			P.scan(pw.incnt, pw.psin, n1);
		scan_count_records_u8(pw.srccnt8, P.bstart_rec(), n1, nullptr, nullptr, 0, pw.scan_tmp, pw.scan_tmp_bytes, s);
	} else if (P.narrow_ic)
		P.scan8pair(pw.incnt8, pw.psin, (size_t)T + 1, pw.srccnt8, v.bstart, (size_t)T + 1);
	else if (P.narrow_sc)
		scan_exclusive_u32_u8_pair(pw.incnt, pw.psin, (size_t)T + 1, pw.srccnt8, v.bstart, (size_t)T + 1, pw.scan_tmp, pw.scan_tmp_bytes, s);
	else if (P.dense)
		P.scan2(pw.incnt, pw.psin, (size_t)T + 1, v.srccnt, v.bstart, (size_t)T + 1);
	pw.host->wait(P.extra_ready);
	// A byte of incnt8 would have passed 255 (capping brackets that share a target, which no gate bounds): psin is not the scan
	// of the true counts, and nothing that indexes with it has been launched.  The caller repeats the pass with words.
	if (P.extra[4]) {
		P.tm.end(30);
		return false;
	}
	pw.prefix_records = (P.rec_ps ? 1 : 0) | (P.rec_bs ? 2 : 0);
	if (P.dense_nb0 == NB0_ON_DEVICE) {
		P.NB0 = P.extra[3];
		if (P.NB0 > pw.nb_cap)
			throw HipError("spanning tree: more back edges than links outside the tree and sides without links (internal sizing bug)");
	}
	const uint32_t NB0 = P.NB0, ncap = P.extra[0], nsimp = P.extra[1], NB = NB0 + ncap + nsimp;
	P.ncap = pw.ncap = ncap;
	P.nsimp = pw.nsimp = nsimp;
	P.NB = NB;
	pw.nb0 = NB0;
	if ((size_t)NB > pw.nb_cap) // (the bracket arrays are carved for that many entries, see for_each_span)
		throw HipError("class stage: more brackets than the workspace was sized for (internal sizing bug)");
	if (!P.dense && !pw.b_key)
		throw HipError("class stage: the bracket sort's buffers were not carved for a sequential tree stage (internal)");
	if (!P.lean && !pw.t_comp)
		throw HipError("class stage: the per-vertex tables were not carved (internal)");
	// Classes of the black tree edges only (the candidate stack holds no others: half the vertices to look up, sort and
	// number).  Per top bracket the reference walks ALL vertices that have it on top, deepest first, and opens a class
	// whenever the list size differs from the one before (recent_size, flubbles.cpp:668-676); leaving the gray edges'
	// vertices out of that walk gives the same classes on the black ones as long as the sizes seen by one bracket never
	// grow again on the way up -- which is what capping edges are for (a bracket only resurfaces once every list spliced
	// under it has ended).  The literal hi_2 rule (flubbles.cpp:566-574) can cap too low; k_capping reports when it
	// picked another target than the second-highest reach, and hairpin reports want the top bracket of every vertex:
	// both take the all-vertices pass.
	P.black_only = !P.want_hp && !pw.all_vertex_classes && P.extra[2] == 0;
	pw.black_only_used = P.black_only;
	if (P.dense) {
		auto place = [&](auto bs) {
			LAUNCH(k_bracket_place<decltype(bs)>, NB, s, NB, NB0, ncap, pw.b_src, pw.b_tgt, pw.b_ord, pw.mpre, bs, v.capf, v.simp, pw.tgtR,
			       P.want_hp ? pw.b_val2 : nullptr);
		};
		if (P.rec_bs)
			place(PrefixRecords{P.bstart_rec()});
		else
			place(PrefixWords{v.bstart});
	} else {
		uint32_t *bk = pw.b_key, *bk2 = pw.b_key2;
		LAUNCH(k_bracket_order, NB, s, NB, NB0, ncap, nsimp, pw.b_src, pw.b_tgt, pw.mpre, bk, pw.b_val, pw.incnt, v.srccnt);
		P.scan2(pw.incnt, pw.psin, (size_t)T + 1, v.srccnt, v.bstart, (size_t)T + 1);
		sort_pairs_u32(bk, bk2, pw.b_val, pw.b_val2, NB, bits_for(T), pw.sort_tmp, pw.sort_tmp_bytes, s);
		LAUNCH(k_gather_u32, NB, s, NB, pw.b_val2, pw.b_tgt, pw.tgtR);
	}
	seg_build(pw.segB, pw.tgtR, NB, s);
	P.NC = P.black_only ? P.V : T;
	return true;
}

// ---- classes of the black tree vertices, in stack order, with rows E and F folded in.  Row E goes first (it only needs
// the tree): the stack index of every black vertex, so that the class pass can work in stack order from the start -- the
// sort carries stack indices, and classes, next_seen and prev are written where rows F/G read them.  Writes s_vtx, ns,
// prev (on request), cflag, dflag; the sorted keys and their stack indices stay where they are for stack_class_ids.
static void classes_black_only(ClassPass &P)
{
	ParWs &pw = P.pw;
	const ClassViews &v = P.v;
	const CompState &cs = P.cs;
	hipStream_t s = P.s;
	const uint32_t V = P.V, NC = P.NC;
	uint32_t *sdl = pw.dlt;
	if (pw.sdl_filled && P.dense) {
		sdl = pw.sdl; // the tree stage's emit kernel had both sizes of every segment in hand and left the differences there
	} else {
		HIP_CHECK(hipMemsetAsync(pw.dlt, 0, ((size_t)V + 2) * 4, s)); // (the bracket counts that lived here are dead)
		LAUNCH(k_shift_delta, V, s, V, cs.ckey, P.sw.c_ntree, pw.gsize, pw.dlt);
	}
	scan_inclusive_u32(sdl, v.shift_ps, (size_t)V + 1, pw.scan_tmp, pw.scan_tmp_bytes, s);
	const StackPlace sp{cs.voff, pw.soff, v.shift_ps, pw.s_vtx};
	// (a stack index is below S, the total of pw.soff, which the host had before the launch)
	const LszField lf = pw.lsz_field = lsz_field(P.S, P.lsz_cap);
	P.with_prefix_views([&](auto ps, auto bs) {
		LAUNCH((k_top_bracket<true, decltype(ps), decltype(bs)>), NC, s, NC, pw.gsize, pw.gpar, pw.mpre, bs, pw.segB, pw.tgtR, ps, v.ck,
		       pw.vals_t, pw.lsz, pw.err, pw.b_val2, P.NB0 + P.ncap, nullptr, cs.ckey, P.sw.c_ntree, sp, lf);
	});
	sort_pairs_u32(v.ck, v.ck2, pw.vals_t, pw.vals_t2, NC, bits_for((uint64_t)P.NB + 1), pw.sort_tmp, pw.sort_tmp_bytes, s);
	// invalid entries carry NIL; after the sort on the low bits they sit behind every valid key
	P.tm.end(30 + 2 * 22);
	P.tm.begin("par_stack");
	// (the class flags are worked out by the same kernel: invalid entries carry NIL and sort behind every valid key)
	// (black_only: the literal hi_2 rule did not fire, so the laminarity check -- prev's one reader -- runs only on request)
	LAUNCH(k_class_finish_black, std::max<size_t>(((size_t)NC + 3) / 4, 1), s, NC, P.S, v.ck2, pw.vals_t2, pw.lsz, v.cflag, pw.ns, pw.prev,
	       pw.check_laminar, v.dflag, lf);
	P.tm.end(1);
	P.tm.begin("par_next_seen"); // (folded into the kernel above)
	P.tm.end(0);
	pw.gcls_valid = false;
	pw.s_cls_valid = false;
}

// ---- classes of every tree vertex (gcls), then row E (the candidate stack: s_vtx, s_cls, topi) and row F (ns, prev, dflag)
static void classes_all_vertices(ClassPass &P)
{
	ParWs &pw = P.pw;
	const ClassViews &v = P.v;
	const CompState &cs = P.cs;
	const SeqWs &sw = P.sw;
	hipStream_t s = P.s;
	const uint32_t V = P.V, T = P.T, NC = P.NC;
	const StackPlace none{nullptr, nullptr, nullptr, nullptr};
	pw.lsz_field = LszField{0, 32, 0}; // (no field: the size of every vertex's list goes through lsz)
	P.with_prefix_views([&](auto ps, auto bs) {
		LAUNCH((k_top_bracket<false, decltype(ps), decltype(bs)>), NC, s, NC, pw.gsize, pw.gpar, pw.mpre, bs, pw.segB, pw.tgtR, ps, v.ck,
		       pw.vals_t, pw.lsz, pw.err, pw.b_val2, P.NB0 + P.ncap, P.want_hp ? pw.hpf : nullptr, nullptr, nullptr, none, pw.lsz_field);
	});
	sort_pairs_u32(v.ck, v.ck2, pw.vals_t, pw.vals_t2, NC, bits_for((uint64_t)P.NB + 1), pw.sort_tmp, pw.sort_tmp_bytes, s);
	LAUNCH(k_class_flags<false>, std::max<size_t>(NC, (size_t)V + 2), s, NC, V, v.ck2, pw.vals_t2, pw.lsz, sw.t_flags, v.cflag, pw.dlt,
	       v.mark);
	P.scan8(v.cflag, v.cps, (size_t)NC + 1);
	LAUNCH(k_class_scatter, NC, s, NC, v.ck2, pw.vals_t2, v.cflag, v.cps, pw.gcls);
	pw.gcls_valid = true;
	pw.s_cls_valid = true;
	P.tm.end(30 + 2 * 22);

	// ---- row E
	P.tm.begin("par_stack");
	LAUNCH(k_shift_delta, V, s, V, cs.ckey, sw.c_ntree, pw.gsize, pw.dlt);
	P.scan(pw.dlt, pw.dlt_ps, (size_t)V + 1);
	// one candidate-stack entry per black tree edge = per segment of a processed component: the host knows where
	// every component's entries start (pw.soff) and the total
	LAUNCH(k_stack_emit, V, s, V, cs.ckey, sw.c_ntree, cs.voff, pw.soff, pw.dlt, pw.dlt_ps, pw.gsize, pw.gcls, pw.s_vtx, pw.s_cls,
	       pw.topi, pw.ns, pw.prev);
	P.tm.end(9);

	// ---- row F
	P.tm.begin("par_next_seen");
	scan_exclusive_max_u32(v.mark, v.lastb, T, pw.scan_tmp, pw.scan_tmp_bytes, s);
	LAUNCH(k_next_from_runs, T, s, T, v.mark, v.lastb, pw.vals_t2, pw.gcls, pw.topi, pw.ns, pw.prev);
	P.tm.end(4);
	LAUNCH(k_dflag, (size_t)P.S + 1, s, P.S, pw.ns, pw.prev, v.dflag);
}

// ---- row G, first part: the two directories over the stack positions (erec: flubbles opened in front of an entry; crec /
// clist: the entry's component), the PVST size of every component, and the summary on its way to the host
static void stack_directories(ClassPass &P)
{
	ParWs &pw = P.pw;
	SeqWs &sw = P.sw;
	hipStream_t s = P.s;
	const uint32_t C = P.C, S = P.S;
	P.tm.begin("par_pvst");
	const size_t n_rec = (size_t)S / 64 + 1;
	KLAUNCH(k_pack_opens, dim3(nblk(((size_t)S / 256 + 1) * 64)), dim3(TPB), 0, s, S, P.v.dflag, pw.erec); // (whole waves: every record of [0, S] is written)
	bitrank_build(pw.erec, n_rec, pw.rk_cnt, pw.scan_tmp, pw.scan_tmp_bytes, s);
	HIP_CHECK(hipMemsetAsync(pw.crec, 0, n_rec * 16, s));
	LAUNCH(k_comp_starts, (size_t)C, s, C, pw.soff, pw.crec);
	bitrank_build(pw.crec, n_rec, pw.rk_cnt, pw.scan_tmp, pw.scan_tmp_bytes, s);
	LAUNCH(k_comp_list, (size_t)C, s, C, pw.soff, pw.crec, pw.clist);
	// What the host needs to lay out the forest -- PVST size and offset of every component, the error words -- goes back in
	// ONE read together with the PVST count: after this synchronisation only the PVST arrays themselves are still to come.
	LAUNCH(k_pvst_counts, (size_t)C + 1, s, C, sw.c_ntree, pw.soff, pw.erec, pw.cproc_ps, pw.doff, sw.c_npvst, sw.c_nstack);
	P.early = pw.host->take<uint32_t>(PassSummary::words(C));
	count_kernel_d2h(PassSummary::words(C) * 4);
	pass_summary(sw, &pw, C, P.early, s);
	P.use_side = S && P.side.stream;
	if (P.use_side) // (everything the endpoints need is computed: the side stream starts from here)
		HIP_CHECK(hipEventRecord(P.side.fork, s));
	// The stream is not left idle while the host reads the PVST count (HostScratch::mark): levels and parents of the
	// flubbles need the stack only, their kernels go out first.
	P.early_ready = pw.host->mark(s);
}

// ---- row G, second part: the laminarity check (when the classes may not be exact, or on request), crossings resolved in
// place, and the level and stack index of every emitted flubble (lev, e_i)
static void laminar_and_levels(ClassPass &P)
{
	ParWs &pw = P.pw;
	const ClassViews &v = P.v;
	hipStream_t s = P.s;
	const uint32_t C = P.C, S = P.S;
	const StackComp comp_of = pw.stack_comp();
	// The (prev, i) intervals of exact cycle-equivalence classes never cross ("Row G"): the laminarity
	// check is only needed when the literal hi_2 rule capped differently from the second-highest reach (extra[2]), i.e. when
	// the classes may not be the exact ones -- or when a caller asks for it.  Without it nothing that follows can flag a
	// component: the summary the host is about to read is the final one.
	pw.laminar_checked = pw.check_laminar || P.extra[2] != 0;
	if (pw.laminar_checked) {
		seg_build(pw.segP, pw.prev, S, s); // NIL (= +inf) where a class has no earlier occurrence
		HIP_CHECK(hipMemsetAsync(v.xflag, 0, (size_t)S + 1, s));
	}
	LAUNCH(k_laminar_walk, ((size_t)S + 3) / 4, s, S, pw.prev, pw.segP, pw.laminar_checked, comp_of, pw.soff, v.xflag, v.dflag, pw.walk);
	if (pw.laminar_checked && S) { // the entries whose interval is crossed: decided in stack order, U undone where the class was popped
		uint32_t *n_x = pw.err + PW_N_X, *n_crossed = pw.err + PW_N_CROSSED;
		compact_flagged_u8(v.xflag, S, v.xlist, n_x, pw.scan_tmp, pw.scan_tmp_bytes, s);
		KLAUNCH(k_resolve_crossings, dim3(std::min<unsigned>(nblk(C), 1024)), dim3(TPB), 0, s, C, pw.soff, n_x, v.xlist, pw.prev, pw.segP, v.xflag,
			pw.walk, n_crossed);
	}
	P.scan(pw.walk, pw.walk_ps, (size_t)S);
	LAUNCH(k_walk_bias, ((size_t)S + 3) / 4, s, S, pw.walk, pw.walk_ps, v.wb, v.wneg);
	scan_exclusive_max_u32(v.wneg, v.wrun, (size_t)S, pw.scan_tmp, pw.scan_tmp_bytes, s);
	LAUNCH(k_levels, ((size_t)S + 3) / 4, s, S, pw.erec, comp_of, pw.soff, v.wb, v.wrun, pw.lev, pw.e_i);
}

// ---- row G, last part: with the PVST count on the host, the result block, the emit kernels and the copies.  Small
// results are written by the emit kernels straight into the forest's page-locked host block (no copy, no extra launch).
// Large ones go through a device block of the same layout (forest_wire::PvstArrays): the scattered 4- and 1-byte stores
// of the emit kernels make poor PCIe packets (~25 GB/s measured), the copy engine moves the finished arrays at link
// speed -- all copies on the side stream: endpoints and orientations while this one still works out levels and parents,
// the parents behind them.
static void emit_and_copy(ClassPass &P)
{
	using Pvst = forest_wire::PvstArrays;
	ParWs &pw = P.pw;
	const SeqWs &sw = P.sw;
	const SideStream &side = P.side;
	PassTail &tail = P.tail;
	hipStream_t s = P.s;
	const uint32_t C = P.C, S = P.S;
	const bool use_side = P.use_side;
	const StackComp comp_of = pw.stack_comp();
	pw.host->wait(P.early_ready);
	const size_t total = PassSummary(C, P.early).total(); // flubbles + one root per processed component
	if (total < P.n_processed || total - P.n_processed > S)
		throw HipError("internal error: PVST size out of range");
	const uint32_t NE = (uint32_t)(total - P.n_processed);
	pw.n_emitted = NE;
	tail.early_summary = P.early;
	tail.summary_final = true; // (nothing after the count flags a component any more: crossings are resolved in place)
	tail.overlapped = tail.want_overlap && tail.summary_final;
	Pvst host, dev; // the forest's block (its device view), and where the emit kernels write
	Pvst::layout(P.alloc_result_block(total), total, &host);
	const bool staged = total >= PVST_STAGE_MIN && side.stream != nullptr;
	if (!staged)
		count_kernel_d2h(total * 14); // (the emit kernels write the five arrays straight into the page-locked block)
	if (staged)
		Pvst::layout(pw.stage, total, &dev);
	else
		dev = host;
	pw.d_a = dev.a, pw.d_z = dev.z, pw.d_parent = dev.parent, pw.d_aor = dev.aor, pw.d_zor = dev.zor;
	pw.d_total = total;
	auto copy_parents = [&](hipStream_t on) {
		HIP_CHECK(copy_async(host.parent, dev.parent, Pvst::word_bytes(total), hipMemcpyDeviceToHost, on));
	};
	if (use_side) {
		// (the roots' slots with the endpoints: the copies behind them take whole arrays)
		HIP_CHECK(hipStreamWaitEvent(side.stream, side.fork, 0));
		KLAUNCH(k_pvst_roots, dim3(nblk((size_t)C)), dim3(TPB), 0, side.stream, C, sw.c_ntree, pw.doff, pw.d_parent, pw.d_a, pw.d_z, pw.d_aor, pw.d_zor);
		KLAUNCH(k_emit_endpoints, dim3(staged ? nblk((S + 3) / 4) : std::min<unsigned>(nblk((S + 3) / 4), 160)), dim3(TPB), 0, side.stream, S, pw.erec,
			comp_of, pw.ns, pw.s_vtx, sw.t_flags, sw.t_gid, pw.cproc_ps, pw.d_a, pw.d_z, pw.d_aor, pw.d_zor);
		if (staged) { // the arrays a..z, then the two orientation arrays
			HIP_CHECK(copy_async(host.a, dev.a, 2 * Pvst::word_bytes(total), hipMemcpyDeviceToHost, side.stream));
			HIP_CHECK(copy_async(host.aor, dev.aor, 2 * Pvst::flag_bytes(total), hipMemcpyDeviceToHost, side.stream));
		}
	} else {
		LAUNCH(k_pvst_roots, (size_t)C, s, C, sw.c_ntree, pw.doff, pw.d_parent, pw.d_a, pw.d_z, pw.d_aor, pw.d_zor);
		if (S)
			KLAUNCH(k_emit_endpoints, dim3(nblk((S + 3) / 4)), dim3(TPB), 0, s, S, pw.erec, comp_of, pw.ns, pw.s_vtx, sw.t_flags,
				sw.t_gid, pw.cproc_ps, pw.d_a, pw.d_z, pw.d_aor, pw.d_zor);
	}
	seg_build(pw.segL, pw.lev, NE, s);
	LAUNCH(k_pvst_emit, NE, s, NE, pw.lev, pw.e_i, pw.segL, comp_of, pw.doff, pw.cproc_ps,
	       pw.d_parent);
	// the parents follow the endpoints on the side stream (the copy engine takes one array after the other anyway): the main
	// stream ends with its last kernel
	hipStream_t last = s;
	if (use_side) {
		if (staged) {
			HIP_CHECK(hipEventRecord(side.fork2, s));
			HIP_CHECK(hipStreamWaitEvent(side.stream, side.fork2, 0));
			copy_parents(side.stream);
		}
		HIP_CHECK(hipEventRecord(side.join, side.stream));
		if (!tail.overlapped)
			HIP_CHECK(hipStreamWaitEvent(s, side.join, 0)); // the pass is complete when both streams are
		else
			last = side.stream; // (the side stream's last work waited for the main stream's last kernel when the result is staged;
					    //  when it is not, `done` below is recorded on both -- see the caller)
	} else if (staged) {
		copy_parents(s);
	}
	if (tail.done) {
		if (tail.overlapped && !staged && use_side) { // both streams carry kernels that write the host block: join them on the side
			HIP_CHECK(hipEventRecord(side.fork2, s));
			HIP_CHECK(hipStreamWaitEvent(side.stream, side.fork2, 0));
		}
		HIP_CHECK(hipEventRecord(tail.done, last));
		if (tail.done2)
			HIP_CHECK(hipEventRecord(tail.done2, last));
	}
	pw.n_stack = S; // export_parallel_stack copies the stack into the per-component layout when a debug hook asks
	P.tm.end(12 + 3 * 22);
}

bool run_parallel_dg(const CompState &cs, SeqWs &sw, ParWs &pw, uint32_t C, uint32_t n_processed, uint32_t n_stack,
		     int64_t dense_nb0, const PassHooks &hooks, const std::function<void *(size_t)> &alloc_result_block, StageTimer &tm,
		     hipStream_t s, const SideStream &side, PassTail &tail)
{
	ClassPass P(cs, sw, pw, C, n_processed, n_stack, dense_nb0, hooks, alloc_result_block, tm, s, side, tail);
	pw.V = P.V;
	pw.E = sw.E;
	pw.C = C;
	pw.T = P.T;
	pw.prefix_records = 0;
	t_space_setup(P);
	bridge_and_capping(P);
	if (!place_brackets(P))
		return false;
	if (P.black_only)
		classes_black_only(P);
	else
		classes_all_vertices(P);
	stack_directories(P);
	laminar_and_levels(P);
	emit_and_copy(P);
	return true;
}

// class ids of the stack entries after a black-only pass (debug hooks): the runs of the sorted order, numbered
static void stack_class_ids(ParWs &pw, hipStream_t s)
{
	if (pw.s_cls_valid)
		return;
	const uint32_t V = pw.V;
	const ClassViews v = class_views(pw);
	scan_exclusive_u8(v.cflag, v.cps, (size_t)V + 1, nullptr, nullptr, 0, pw.scan_tmp, pw.scan_tmp_bytes, s);
	LAUNCH(k_class_ids_black, V, s, V, v.ck2, pw.vals_t2, v.cflag, v.cps, pw.s_cls, pw.lsz_field);
	pw.s_cls_valid = true;
}
uint32_t count_saturated(ParWs &pw, hipStream_t s)
{
	if (!pw.black_only_used)
		return 0;
	const ClassViews v = class_views(pw);
	HIP_CHECK(hipMemsetAsync(pw.err + PW_LSZ_SAT, 0, 4, s));
	LAUNCH(k_count_saturated, pw.V, s, pw.V, v.ck2, pw.vals_t2, pw.lsz_field, pw.err + PW_LSZ_SAT);
	return pw.host->read_u32(pw.err + PW_LSZ_SAT, s);
}
void classes_to_tree_space(ParWs &pw, hipStream_t s)
{
	if (pw.gcls_valid)
		return;
	stack_class_ids(pw, s);
	HIP_CHECK(hipMemsetAsync(pw.gcls, 0xFF, (size_t)pw.T * 4, s));
	if (pw.n_stack)
		LAUNCH(k_cls_from_stack, pw.n_stack, s, pw.n_stack, pw.s_vtx, pw.s_cls, pw.gcls);
	pw.gcls_valid = true;
}

void export_parallel_stack(const CompState &cs, SeqWs &sw, ParWs &pw, hipStream_t s)
{
	stack_class_ids(pw, s);
	const uint32_t S = pw.n_stack;
	LAUNCH(k_export_stack, S, s, S, pw.stack_comp(), pw.soff, cs.voff, pw.s_vtx, pw.s_cls, pw.ns, sw.s_vtx, sw.s_cls,
	       sw.next_seen);
}

} // namespace povu_hip
