// call_kernels.hip -- the variant calls of a set of PVST vertices by reference paths (povu_hip_segments_upload,
// povu_hip_call; include/povu_hip.h).
//
// The definition is this project's own ("Variant calls"; restated in tests/vcf_ref.py).  A call runs the
// traversal pipeline (trav_kernels.hip) on the sites given and keeps its arrays on the device, then:
//   reference offsets  the segment lengths of the reference paths' steps, one exclusive u64 scan (a path's offsets are the
//                      scan minus its value at the path's first step);
//   callability        a CSR over the segments lists (site, boundary) pairs; a pass over the reference steps marks the
//                      (site, reference, boundary) bits it meets; presence per (tree, reference) is the OR over the tree's
//                      sites; a site is callable when no subflubble lies on its way to the root, some reference is present
//                      and every present reference has both bits; a callable site clears its parent's "called" flag;
//   slot table         per called site of two alleles or more and per genotype slot, the min and max allele (atomics);
//   records            the reference traversals of those sites, compacted, radix-sorted by (reference, POS) (stable, so
//                      ties keep (site, first step) order); per record one wave, a lane per sample: GT codes, AC, AN, NS,
//                      TANGLED;
//   spelling           per (site, orientation) a record needs, every allele: lengths, u64 scans, then one wave per allele
//                      copies the bases (reverse-complemented on '<' steps, lanes across a segment's bytes) and writes the
//                      AT step string (lanes across steps, a wave prefix sum of their decimal widths).
// With POVU_HIP_T_NESTED (INTEGRATION.md "Nested calls"; nest_kernels.hip) the steps from the kept sites on read classes where
// they read alleles: `aoff`, `oa` and `afirst` below are then the class offsets of a site, the class of a traversal and the
// first traversal of a class's representative.  What differs per record is kept per record (rstate): whether it is anchored
// (REF is the reference's own exact allele, the ALTs the representatives), whether REF has no inner base, whether REF is
// spelled on its own (an "extra" one-allele block behind the class blocks).  A block is a (site, anchored, orientation).
// With POVU_HIP_T_OFFREF (INTEGRATION.md "Off-reference calls"; offref_kernels.hip) the sites called off-reference join `called`
// behind callability, and from surrogate_offsets on the view's "reference paths" are the calling paths: the references and the
// surrogates, ascending.  Which traversals of a kept site are records is asked of is_record_path (call_common.hpp).
// With POVU_HIP_T_UNTANGLE (INTEGRATION.md "Untangled calls"; untangle_kernels.hip) one step behind the spelling rewrites the GT
// rows and counts of the sites a path laps; without the flag it is not run and nothing of it is allocated.
// With regions (povu_hip_call_restricted; INTEGRATION.md "Region calls"; region_kernels.hip) the front end marks the segments
// the regions meet and the sites that pass; where the call is not nested the other sites lose their entered sides there, so
// the traversal pipeline never scans them; flubble_records selects the records of the passing sites in front of the sort
// (under the mask it drops nothing) and the inversion records are reported against the marks.  The region arrays live in the
// front end's arena (tr_ws), which nothing carves again before both have read them.
// With a threshold (povu_hip_call_clustered; INTEGRATION.md "Clustered calls"; cluster_kernels.hip) the classes are the clusters of
// a site's exact alleles: the same four arrays from another producer, the own-REF path and the extra blocks as in a nested call.
// What stays a nested call's alone: PS, levels, parents and TANGLED on a collapse.  Per record the call then also says whether
// its site lost alleles, the site's lowest similarity and the exact alleles behind every written allele (k_cl_provenance).
#include "call_common.hpp"
#include "call_modes.hpp"
#include "cluster_kernels.hpp"
#include "cluster_rules.hpp"
#include "merge_kernels.hpp"
#include "nest_kernels.hpp"
#include "norm_kernels.hpp"
#include "offref_kernels.hpp"
#include "prim_kernels.hpp"
#include "region_kernels.hpp"
#include "untangle_kernels.hpp"

namespace povu_hip
{

static constexpr uint32_t MAX_ALLELES = 65534;

// ---- reference offsets: length of every reference step (ref_base: first step of every reference in the concatenation)
__global__ void k_cl_ref_len(RefView R, PathsView P, uint64_t *__restrict__ len)
{
	for (uint64_t i = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; i < R.NR; i += (uint64_t)gridDim.x * Q_TPB) {
		const uint32_t r = span_of(R.ref_base, R.nR, i);
		const uint32_t x = P.steps[P.path_off[R.ref_path[r]] + (i - R.ref_base[r])];
		len[i] = P.seq_off[(x >> 1) + 1] - P.seq_off[x >> 1];
	}
}
void launch_ref_len(const RefView &R, const PathsView &P, uint64_t *len, hipStream_t s)
{
	KLAUNCH(k_cl_ref_len, dim3(stride_blocks(R.NR)), dim3(Q_TPB), 0, s, R, P, len);
}

// ---- segment -> (site, boundary) CSR
__global__ void k_cl_seg_count(uint32_t n, const uint32_t *__restrict__ qa, const uint32_t *__restrict__ qz, const uint32_t *__restrict__ vid,
			       uint32_t V, uint32_t *__restrict__ cnt, uint32_t *__restrict__ qv)
{
	for (uint32_t q = blockIdx.x * Q_TPB + threadIdx.x; q < n; q += gridDim.x * Q_TPB) {
		const uint32_t a = find_vertex(vid, V, qa[q]), z = find_vertex(vid, V, qz[q]);
		qv[2 * (size_t)q] = a;
		qv[2 * (size_t)q + 1] = z;
		if (a != NO_QUERY)
			atomicAdd(cnt + a, 1u);
		if (z != NO_QUERY)
			atomicAdd(cnt + z, 1u);
	}
}
__global__ void k_cl_seg_fill(uint32_t n, const uint32_t *__restrict__ qv, const uint32_t *__restrict__ off, uint32_t *__restrict__ cur,
			      uint32_t *__restrict__ val)
{
	for (uint64_t e = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; e < 2 * (uint64_t)n; e += (uint64_t)gridDim.x * Q_TPB) {
		const uint32_t v = qv[e];
		if (v != NO_QUERY)
			val[off[v] + atomicAdd(cur + v, 1u)] = (uint32_t)e; // (site << 1 | boundary)
	}
}

// ---- (site, reference, boundary) bits met by the reference steps
__global__ void k_cl_hits(RefView R, PathsView P, const uint32_t *__restrict__ off, const uint32_t *__restrict__ val, uint32_t *__restrict__ hit)
{
	for (uint64_t i = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; i < R.NR; i += (uint64_t)gridDim.x * Q_TPB) {
		const uint32_t r = span_of(R.ref_base, R.nR, i);
		const uint32_t v = P.steps[P.path_off[R.ref_path[r]] + (i - R.ref_base[r])] >> 1;
		for (uint32_t e = off[v]; e < off[v + 1]; e++) {
			const uint32_t qr = val[e];
			const uint64_t bit = ((uint64_t)(qr >> 1) * R.nR + r) * 2 + (qr & 1u);
			atomicOr(hit + (bit >> 5), 1u << (bit & 31));
		}
	}
}
__device__ __forceinline__ uint32_t hits_of(const uint32_t *__restrict__ hit, uint64_t q, uint32_t nR, uint32_t r)
{
	const uint64_t bit = (q * nR + r) * 2;
	return (hit[bit >> 5] >> (bit & 31)) & 3u;
}
__device__ __forceinline__ bool bit_of(const uint32_t *__restrict__ w, uint64_t b) { return (w[b >> 5] >> (b & 31)) & 1u; }

__global__ void k_cl_present(uint64_t nq, uint32_t nR, const uint32_t *__restrict__ hit, const uint32_t *__restrict__ tree,
			     uint32_t *__restrict__ present)
{
	for (uint64_t i = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; i < nq * nR; i += (uint64_t)gridDim.x * Q_TPB) {
		const uint64_t q = i / nR;
		const uint32_t r = (uint32_t)(i % nR);
		if (hits_of(hit, q, nR, r)) {
			const uint64_t b = (uint64_t)tree[q] * nR + r;
			atomicOr(present + (b >> 5), 1u << (b & 31));
		}
	}
}

__device__ __forceinline__ bool is_sub(uint8_t f) { return f == 'T' || f == 'O' || f == 'C' || f == 'M' || f == 'S'; }

__global__ void k_cl_callable(uint32_t n, uint32_t nR, const uint32_t *__restrict__ hit, const uint32_t *__restrict__ present,
			      const uint32_t *__restrict__ tree, const uint32_t *__restrict__ parent, const uint8_t *__restrict__ fam,
			      uint8_t *__restrict__ callable, uint8_t *__restrict__ called)
{
	for (uint32_t q = blockIdx.x * Q_TPB + threadIdx.x; q < n; q += gridDim.x * Q_TPB) {
		bool skip = false;
		for (uint32_t v = q, k = 0; v != NO_QUERY && k <= n; v = parent[v], k++)
			skip |= is_sub(fam[v]);
		bool any = false, ok = true;
		for (uint32_t r = 0; r < nR && !skip; r++) {
			if (bit_of(present, (uint64_t)tree[q] * nR + r)) {
				any = true;
				ok &= hits_of(hit, q, nR, r) == 3u;
			}
		}
		callable[q] = called[q] = !skip && any && ok;
	}
}
__global__ void k_cl_unparent(uint32_t n, const uint8_t *__restrict__ callable, const uint32_t *__restrict__ parent, uint8_t *__restrict__ called)
{
	for (uint32_t q = blockIdx.x * Q_TPB + threadIdx.x; q < n; q += gridDim.x * Q_TPB)
		if (callable[q] && parent[q] != NO_QUERY)
			called[parent[q]] = 0;
}
// kept sites: called, two alleles or more
__global__ void k_cl_keep(uint32_t n, const uint8_t *__restrict__ called, const uint32_t *__restrict__ aoff, uint32_t *__restrict__ keep,
			  uint32_t *__restrict__ maxal)
{
	for (uint32_t q = blockIdx.x * Q_TPB + threadIdx.x; q <= n; q += gridDim.x * Q_TPB) {
		const uint32_t nal = q < n ? aoff[q + 1] - aoff[q] : 0;
		keep[q] = q < n && called[q] && nal >= 2;
		if (keep[q])
			atomicMax(maxal, nal);
	}
}

// inner bases and AT width of every allele (of a kept site), S -> Z
__global__ void k_cl_inner(uint32_t n_al, CallView V, uint64_t *__restrict__ ilen, uint64_t *__restrict__ atl)
{
	for (uint32_t a = blockIdx.x * Q_TPB + threadIdx.x; a < n_al; a += gridDim.x * Q_TPB) {
		const uint32_t t = V.afirst[a];
		InnerSize n{0, 0};
		if (V.keep[V.trav.rq[t]])
			n = span_inner_size(trav_span(V.trav.rpos, V.trav.rlen, t), V.paths);
		ilen[a] = n.bases;
		atl[a] = n.at;
	}
}
// alleles without an inner base, per kept site (a record is anchored when REF or one of its ALTs is such an allele)
__global__ void k_cl_zero_len(uint32_t n, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ aoff, const uint64_t *__restrict__ ilen,
			      uint32_t *__restrict__ zc)
{
	for (uint32_t q = blockIdx.x * Q_TPB + threadIdx.x; q < n; q += gridDim.x * Q_TPB) {
		uint32_t e = 0;
		if (keep[q])
			for (uint32_t a = aoff[q]; a < aoff[q + 1]; a++)
				e += ilen[a] == 0;
		zc[q] = e;
	}
}
// a call with classes: the kept sites with fewer classes than exact alleles; vanished: the called sites of two exact alleles or
// more left with one class
__global__ void k_cl_collapsed(uint32_t n, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ exact_off, const uint32_t *__restrict__ aoff,
			       const uint8_t *__restrict__ called, uint8_t *__restrict__ collapsed, uint32_t *__restrict__ count,
			       uint32_t *__restrict__ vanished)
{
	for (uint32_t q = blockIdx.x * Q_TPB + threadIdx.x; q < n; q += gridDim.x * Q_TPB) {
		const bool c = keep[q] && aoff[q + 1] - aoff[q] < exact_off[q + 1] - exact_off[q];
		collapsed[q] = c;
		if (c)
			atomicAdd(count, 1u);
		if (called[q] && exact_off[q + 1] - exact_off[q] >= 2 && aoff[q + 1] - aoff[q] == 1)
			atomicAdd(vanished, 1u);
	}
}
// clustered calls, per record (row dst[i], or i): its site lost alleles, the site's lowest similarity, and per written allele
// (REF's cluster first, the others in order) the exact alleles behind it, at ac_off[row] + row + allele
__global__ void k_cl_provenance(uint32_t nrec, const uint32_t *__restrict__ perm, CallView V, const uint32_t *__restrict__ dst,
				const uint8_t *__restrict__ collapsed, const uint32_t *__restrict__ minsim, const uint32_t *__restrict__ csize,
				const uint64_t *__restrict__ ac_off, uint8_t *__restrict__ rec_clustered, uint32_t *__restrict__ cl_minsim,
				uint32_t *__restrict__ cl_nx)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < nrec; i += gridDim.x * Q_TPB) {
		const uint32_t t = V.rlist[perm[i]], q = V.trav.rq[t], d = dst ? dst[i] : i, rc = V.oa[t], c0 = V.aoff[q], nc = V.aoff[q + 1] - c0;
		rec_clustered[d] = collapsed[q];
		cl_minsim[d] = minsim[q];
		uint32_t *__restrict__ nx = cl_nx + ac_off[d] + d;
		nx[0] = csize[c0 + rc];
		for (uint32_t c = 0, k = 1; c < nc; c++)
			if (c != rc)
				nx[k++] = csize[c0 + c];
	}
}
// per flubble record j (before the sort): rstate; the inner bases and AT width of its REF (xilen, xatl: the reference's own
// exact allele); with want_len the written lengths of REF and of its longest allele.  V.crep == NULL: not nested (alleles, REF
// always the block's).
__global__ void k_cl_rec_state(CallView V, uint32_t want_len, uint8_t *__restrict__ rstate, uint64_t *__restrict__ xilen, uint64_t *__restrict__ xatl,
			       uint64_t *__restrict__ ref_len, uint64_t *__restrict__ max_len)
{
	for (uint32_t j = blockIdx.x * Q_TPB + threadIdx.x; j < V.nfl; j += gridDim.x * Q_TPB) {
		const uint32_t t = V.rlist[j], q = V.trav.rq[t], ec = V.aoff[q] + V.oa[t];
		const bool own = V.crep && V.crep[ec] != V.trav.aoff[q] + V.trav.oa[t];
		InnerSize n{V.ilen[ec], V.atl[ec]};
		if (own)
			n = span_inner_size(trav_span(V.trav.rpos, V.trav.rlen, t), V.paths);
		const bool anch = n.bases == 0 || V.zc[q] - (V.ilen[ec] == 0 ? 1u : 0u) > 0;
		rstate[j] = (anch ? RS_ANCHORED : 0) | (n.bases == 0 ? RS_REF_EMPTY : 0) | (own ? RS_OWN_REF : 0);
		xilen[j] = n.bases;
		xatl[j] = n.at;
		if (want_len) {
			// the anchor step is the site's boundary the reference enters by, whatever the allele
			const WrittenAllele ref = written_allele(V, t, V.trav.orv[t] != 0, anch, n.bases, n.at);
			uint64_t mx = n.bases;
			for (uint32_t a = V.aoff[q]; a < V.aoff[q + 1]; a++)
				if (a != ec)
					mx = max(mx, V.ilen[a]);
			ref_len[j] = ref.text_len();
			max_len[j] = mx + (ref.anchor_base ? 1 : 0);
		}
	}
}

// min / max allele of every (kept site, slot)
__global__ void k_cl_slots(uint32_t R, const uint32_t *__restrict__ rq, const uint32_t *__restrict__ op, const uint32_t *__restrict__ oa,
			   const uint32_t *__restrict__ keep, const uint32_t *__restrict__ qidx, const uint32_t *__restrict__ slot_of_path,
			   uint32_t S, uint32_t *__restrict__ smin, uint32_t *__restrict__ smax)
{
	for (uint32_t t = blockIdx.x * Q_TPB + threadIdx.x; t < R; t += gridDim.x * Q_TPB) {
		const uint32_t q = rq[t];
		if (!keep[q])
			continue;
		const uint64_t i = (uint64_t)qidx[q] * S + slot_of_path[op[t]];
		atomicMin(smin + i, oa[t]);
		atomicMax(smax + i, oa[t]);
	}
}
__global__ void k_cl_rec_flag(CallView V, uint8_t *__restrict__ flag)
{
	for (uint32_t t = blockIdx.x * Q_TPB + threadIdx.x; t < V.trav.R; t += gridDim.x * Q_TPB)
		flag[t] = V.keep[V.trav.rq[t]] && is_record_path(V, V.trav.rq[t], V.trav.op[t]);
}
// reference number of flubble record j
__device__ __forceinline__ uint32_t ref_of_record(const CallView &V, uint32_t j) { return V.ref.ref_of_path[V.trav.op[V.rlist[j]]]; }
__global__ void k_cl_pos(CallView V, uint64_t *__restrict__ pos)
{
	for (uint32_t j = blockIdx.x * Q_TPB + threadIdx.x; j < V.nfl; j += gridDim.x * Q_TPB) {
		const uint64_t b = V.ref.ref_base[ref_of_record(V, j)];
		pos[j] = V.ref.roff[b + V.trav.of[V.rlist[j]] + 1] - V.ref.roff[b] + ((V.rstate[j] & RS_ANCHORED) ? 0 : 1);
	}
}
// sort key of record perm[i]: 0 = POS low word, 1 = POS high word, 2 = reference
__global__ void k_cl_key(uint32_t nrec, int which, const uint32_t *__restrict__ perm, CallView V, uint32_t *__restrict__ key)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < nrec; i += gridDim.x * Q_TPB) {
		const uint32_t j = perm[i];
		key[i] = which == 0 ? (uint32_t)V.pos[j] : which == 1 ? (uint32_t)(V.pos[j] >> 32) : ref_of_record(V, j);
	}
}

// per record (sorted; row dst[i] of the record list when inversion records are merged in, else row i): its fields, the ALT count for the AC offsets, the (site, orientation) it needs spelled
__global__ void k_cl_rec_fields(uint32_t nrec, const uint32_t *__restrict__ perm, CallView V, InvRows o, uint32_t *__restrict__ need,
				const uint32_t *__restrict__ dst, const uint32_t *__restrict__ n_level, const uint32_t *__restrict__ n_parent,
				uint32_t *__restrict__ o_level, uint32_t *__restrict__ o_parent, uint32_t *__restrict__ xneed,
				const uint8_t *__restrict__ star, uint8_t *__restrict__ o_star)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < nrec; i += gridDim.x * Q_TPB) {
		const uint32_t j = perm[i], t = V.rlist[j], q = V.trav.rq[t], d = dst ? dst[i] : i;
		// (what is read, then what is written: the rows' pointers come in a struct and promise the compiler nothing)
		const uint32_t level = n_level ? n_level[j] : V.height[q] - 1, parent = n_parent ? n_parent[j] : NO_QUERY;
		// ("Spanning alleles": a record with a spanned entry writes one ALT more, `*`, behind its classes)
		const bool has_star = star && star[j];
		const uint32_t path = V.trav.op[t], first = V.trav.of[t], ref = V.oa[t], nal = span_n_alleles(V.aoff[q + 1] - V.aoff[q], has_star);
		const uint64_t pos = V.pos[j];
		const uint8_t st = V.rstate[j], orv = V.trav.orv[t];
		o_level[d] = level;
		o_parent[d] = parent;
		xneed[i] = (st & RS_OWN_REF) ? 1 : 0;
		o.o_q[d] = q;
		o.o_path[d] = path;
		o.o_first[d] = first;
		o.o_ref[d] = ref;
		o.o_nal[d] = nal;
		o.o_pos[d] = pos;
		o.nalt[d] = nal - 1;
		if (o_star)
			o_star[d] = has_star;
		need[4 * (size_t)q + ((st & RS_ANCHORED) ? 2 : 0) + orv] = 1;
	}
}
// reference number and POS of the sorted records (the inversion records are merged in by them)
__global__ void k_cl_sorted_keys(uint32_t nrec, const uint32_t *__restrict__ perm, CallView V, uint32_t *__restrict__ f_ref, uint64_t *__restrict__ f_pos)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < nrec; i += gridDim.x * Q_TPB) {
		f_ref[i] = ref_of_record(V, perm[i]);
		f_pos[i] = V.pos[perm[i]];
	}
}

// GT codes, AC, AN, NS and flags: one wave per record, a lane per sample (its slots are consecutive).  SPAN ("Spanning
// alleles"): an empty slot whose bit of span_bits is set takes the `*` code; without it the kernel is the one it was
template <bool SPAN>
__global__ __launch_bounds__(Q_TPB) void k_cl_records(uint32_t nrec, CallView V, SlotsView SL, InvRows o, const uint32_t *__restrict__ qidx,
						      const uint32_t *__restrict__ smin, const uint32_t *__restrict__ smax,
						      const uint64_t *__restrict__ ac_off, const uint32_t *__restrict__ perm,
						      const uint8_t *__restrict__ collapsed, const uint8_t *__restrict__ rescued,
						      uint32_t *__restrict__ ac, const uint32_t *__restrict__ dst,
							      const unsigned long long *__restrict__ span_bits, uint32_t span_words)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	// what the loop over the slots reads and writes, out of the structs
	const uint32_t *__restrict__ slot_first = SL.slot_first;
	uint16_t *__restrict__ gt = o.gt;
	const uint32_t n_samples = SL.NS, S = SL.S;
	for (uint32_t i0 = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); i0 < nrec; i0 += waves) {
		const uint32_t i = dst ? dst[i0] : i0;
		const uint32_t q = o.o_q[i], ra = o.o_ref[i], own = SL.slot_of_path[o.o_path[i]];
		const uint64_t base = (uint64_t)qidx[q] * S;
		// "Spanning alleles": the words of the record's spanned entries (k_ns_span, by the record before the sort), its classes
		const unsigned long long *__restrict__ spanned = SPAN ? span_bits + (uint64_t)perm[i0] * span_words : nullptr;
		const uint32_t n_classes = SPAN ? V.aoff[q + 1] - V.aoff[q] : 0;
		uint32_t n_an = 0, n_ns = 0, amb = 0;
		for (uint32_t sm = lane; sm < n_samples; sm += 64) {
			bool any = false;
			for (uint32_t sl = slot_first[sm]; sl < slot_first[sm + 1]; sl++) {
				uint32_t code = POVU_HIP_GT_MISSING;
				if (sl == own) {
					code = 0;
				} else {
					const uint32_t mn = smin[base + sl], mx = smax[base + sl];
					if (mn != 0xFFFFFFFFu && mn == mx)
						code = mn == ra ? 0 : mn < ra ? mn + 1 : mn;
					else if (mn != 0xFFFFFFFFu)
						amb = 1;
					else if (SPAN)
						code = span_gt_code(code, (spanned[sl >> 6] >> (sl & 63u)) & 1ull, n_classes);
				}
				gt[(uint64_t)i * S + sl] = (uint16_t)code;
				if (code != POVU_HIP_GT_MISSING) {
					any = true;
					n_an++;
					if (code)
						atomicAdd(ac + ac_off[i] + code - 1, 1u);
				}
			}
			n_ns += any;
		}
		n_an = wave_sum(n_an);
		n_ns = wave_sum(n_ns);
		amb = wave_sum(amb);
		if (lane == 0) {
			o.o_an[i] = n_an;
			o.o_ns[i] = n_ns;
			uint8_t f = 0;
			const uint32_t j = perm[i0];
			const uint8_t st = V.rstate[j];
			if (st & RS_ANCHORED)
				f |= POVU_HIP_CALL_ANCHORED | ((st & RS_REF_EMPTY) ? POVU_HIP_CALL_INS : POVU_HIP_CALL_DEL);
			if (V.trav.qstatus[q] || amb)
				f |= POVU_HIP_CALL_TANGLED;
			if (collapsed && collapsed[q])
				f |= POVU_HIP_CALL_TANGLED | POVU_HIP_CALL_COLLAPSED;
			if (rescued && rescued[j])
				f |= POVU_HIP_CALL_RESCUED;
			if (st & RS_NORMALIZED)
				f |= POVU_HIP_CALL_NORMALIZED;
			o.o_flags[i] = f;
		}
	}
}

__global__ void k_cl_blocks(uint64_t n2, const uint32_t *__restrict__ need, const uint32_t *__restrict__ boff, uint32_t *__restrict__ blist)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x < n2; x += (uint64_t)gridDim.x * Q_TPB)
		if (need[x])
			blist[boff[x]] = (uint32_t)x;
}
__global__ void k_cl_rec_block(uint32_t nrec, const uint32_t *__restrict__ perm, CallView V, const uint32_t *__restrict__ boff,
			       uint32_t *__restrict__ o_block, const uint32_t *__restrict__ dst, const uint32_t *__restrict__ xoff,
			       uint32_t *__restrict__ xrow)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < nrec; i += gridDim.x * Q_TPB) {
		const uint32_t j = perm[i], t = V.rlist[j], d = dst ? dst[i] : i;
		o_block[d] = boff[4 * (size_t)V.trav.rq[t] + ((V.rstate[j] & RS_ANCHORED) ? 2 : 0) + V.trav.orv[t]];
		xrow[d] = (V.rstate[j] & RS_OWN_REF) ? xoff[i] : NO_QUERY;
	}
}
// the extra blocks (one spelled allele each: the REF of a record that is not its class's representative) and their records
__global__ void k_cl_extra(uint32_t nrec, const uint32_t *__restrict__ perm, const uint8_t *__restrict__ rstate, const uint32_t *__restrict__ xoff,
			   BlockLayout L, uint32_t *__restrict__ xlist, uint64_t *__restrict__ bcnt)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < nrec; i += gridDim.x * Q_TPB)
		if (rstate[perm[i]] & RS_OWN_REF) {
			xlist[xoff[i]] = perm[i];
			bcnt[L.extra_block(xoff[i])] = 1;
		}
}
// REF among the spelled alleles: the extra block's one allele, or allele ref_allele of the record's block
__global__ void k_cl_ref_spelled(uint32_t nrec, const uint32_t *__restrict__ o_block, const uint32_t *__restrict__ o_ref,
				 const uint32_t *__restrict__ xrow, const uint64_t *__restrict__ block_off, BlockLayout L,
				 uint64_t *__restrict__ ref_spelled)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < nrec; i += gridDim.x * Q_TPB)
		ref_spelled[i] = xrow[i] != NO_QUERY ? block_off[L.extra_block(xrow[i])] : block_off[o_block[i]] + o_ref[i];
}
__global__ void k_cl_block_cnt(uint32_t nb, const uint32_t *__restrict__ blist, const uint32_t *__restrict__ aoff, uint64_t *__restrict__ cnt)
{
	for (uint32_t b = blockIdx.x * Q_TPB + threadIdx.x; b < nb; b += gridDim.x * Q_TPB) {
		const uint32_t q = blist[b] >> 2;
		cnt[b] = aoff[q + 1] - aoff[q];
	}
}

// where the flubble family's spelled alleles are found: the blocks' offsets, the class blocks' (site, anchored, orientation),
// the extra blocks' records
struct FlubbleBlocks {
	BlockLayout L;
	const uint64_t *block_off;
	const uint32_t *blist, *xlist;
};
__device__ __forceinline__ WrittenAllele spelled_allele(uint64_t j, const CallView &V, const FlubbleBlocks &B)
{
	const uint32_t b = span_of(B.block_off, B.L.nfb, j);
	if (B.L.is_class(b))
		return allele_of_block(V, B.blist[b], (uint32_t)(j - B.block_off[b]));
	return own_ref_of_record(V, B.xlist[b - B.L.nfc]);
}

__global__ void k_cl_spell_len(CallView V, FlubbleBlocks B, uint64_t *__restrict__ slen, uint64_t *__restrict__ alen)
{
	for (uint64_t j = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; j < B.L.nfsp; j += (uint64_t)gridDim.x * Q_TPB) {
		const WrittenAllele s = spelled_allele(j, V, B);
		slen[j] = s.text_len();
		alen[j] = s.at_len(V.paths);
	}
}

// one wave per spelled allele: the bases, then the AT string
__global__ __launch_bounds__(Q_TPB) void k_cl_emit(CallView V, FlubbleBlocks B, const uint64_t *__restrict__ s_off, const uint64_t *__restrict__ a_off,
						   char *__restrict__ o_seq, char *__restrict__ o_at, unsigned long long *__restrict__ bad)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t waves = (uint64_t)gridDim.x * (Q_TPB / 64);
	// what the copy loops read, out of the view
	const uint32_t *__restrict__ steps = V.paths.steps, *__restrict__ vid = V.paths.vid;
	const uint64_t *__restrict__ seq_off = V.paths.seq_off;
	const char *__restrict__ seq = V.paths.seq;
	for (uint64_t j = (uint64_t)blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); j < B.L.nfsp; j += waves) {
		const WrittenAllele s = spelled_allele(j, V, B);
		uint64_t w = s_off[j], wa = a_off[j];
		// the anchor: last base of the first step, and its step text
		if (s.anchored) {
			const uint32_t v = s.anchor >> 1;
			if (s.anchor_base) {
				if (lane == 0) {
					const uint8_t c = (uint8_t)seq[s.anchor_at], r = comp(c);
					if (!r)
						atomicMin(bad, (unsigned long long)v);
					o_seq[w] = (char)((s.anchor & 1u) ? r : c);
				}
				w++;
			}
			const uint32_t width = 1 + ndig(vid[v]);
			if (lane == 0)
				put_step(o_at, vid, s.anchor, wa, width);
			wa += width;
		}
		emit_steps(lane, s.inner_steps(), [&](uint32_t k) { return s.inner_step(steps, k); }, seq_off, seq, vid, w, wa, o_seq, o_at, bad);
	}
}

} // namespace povu_hip

// ---- C ABI

extern "C" int povu_hip_segments_upload(povu_hip_ctx *ctx, uint32_t n_vtx, const uint64_t *seq_off, const char *seq, char *err,
					size_t errlen)
{
	return guarded_call(ctx, err, errlen, 1, [&] {
		if (!ctx)
			throw HipError("null context");
		if (!ctx->g.block)
			throw HipError("sequences need a resident graph (povu_hip_graph_upload first)");
		ctx->seq_valid = false;
		if (n_vtx != ctx->g.V)
			throw HipError("sequences of " + std::to_string(n_vtx) + " segments for a resident graph of " + std::to_string(ctx->g.V));
		if (!seq_off || seq_off[0] != 0)
			throw HipError("seq_off[0] must be 0");
		for (uint32_t v = 0; v < n_vtx; v++)
			if (seq_off[v + 1] < seq_off[v])
				throw HipError("sequence offsets of vertex " + std::to_string(v) + " decrease");
		const uint64_t B = seq_off[n_vtx];
		if (B && !seq)
			throw HipError("null sequence bytes");
		HIP_CHECK(hipSetDevice(ctx->device));
		ctx->wait_tail();
		carve(
			ctx->seq_buf,
			[&](Spans &take) {
				take((size_t)n_vtx + 1, ctx->seq_off);
				take(B + 8, ctx->seq);
			},
			false);
		hipStream_t s = ctx->stream;
		HIP_CHECK(copy_async(ctx->seq_off, seq_off, ((size_t)n_vtx + 1) * 8, hipMemcpyHostToDevice, s));
		if (B)
			HIP_CHECK(copy_async(ctx->seq, seq, B, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipStreamSynchronize(s));
		ctx->seq_gen = ctx->g.gen;
		ctx->seq_valid = true;
		return 0;
	});
}

namespace
{
struct CallsOwner {
	povu_hip_calls view{}; // first member: the owner is recovered from it in povu_hip_calls_free
	PinnedVec<uint32_t> query, path, first, ref_allele, n_alleles, an, ns, block, ac, n_steps, level, parent_query, norm_block, norm_shift, norm_chop,
		norm_trim;
	PinnedVec<uint64_t> pos, ac_off, block_off, seq_off, at_off, ref_spelled, raw_pos;
	PinnedVec<uint8_t> flags;
	// the rows of the `decomposed` profile
	PinnedVec<uint32_t> row_record, row_alt, row_index, row_ref_start, row_ref_len, row_alt_start, row_alt_len, row_ac, row_an, row_ns;
	PinnedVec<uint8_t> row_kind, row_reason, row_lead;
	PinnedVec<uint64_t> row_pos;
	// ... merged (POVU_HIP_T_MERGE)
	PinnedVec<uint64_t> mrow_off;
	PinnedVec<uint32_t> mrow_member, mrow_ac, mrow_an, mrow_ns;
	PinnedVec<uint8_t> mrow_gt;
	PinnedVec<uint16_t> gt;
	PinnedVec<char> seq, at;
	std::vector<uint64_t> contig_len;
	// POVU_HIP_T_OFFREF
	PinnedVec<uint8_t> rec_offref;
	PinnedVec<uint32_t> host_query, host_allele;
	std::vector<uint32_t> off_contig_path;
	std::vector<uint64_t> off_contig_len;
	// POVU_HIP_T_UNTANGLE
	PinnedVec<uint8_t> rec_unt;
	PinnedVec<uint32_t> lap, n_laps;
	PinnedVec<uint16_t> lap_count;
	// clustered calls
	PinnedVec<uint8_t> rec_clustered;
	PinnedVec<uint32_t> cl_minsim, cl_nx;
	// POVU_HIP_T_SPANNING
	PinnedVec<uint8_t> rec_star;
};

using namespace povu_hip;

// what a call is given, checked, and the host tables made of it
struct CallInputs {
	const povu_hip_sites *sites;
	const povu_hip_call_refs *refs;
	const uint32_t *slot_of_path;
	const povu_hip_trav_opts *opts;
	uint32_t n, P, nR, S, NS, n_trees = 0;
	bool inversions, nested, normalized, decomposed, merge, offref, untangle;
	bool spanning = false;	  // POVU_HIP_T_SPANNING: an option of the nested call
	uint32_t cluster_ppm = 0; // clustered calls: the threshold T, 0: not clustered
	bool cluster_no_bound = false;
	bool classes() const { return nested || cluster_ppm; } // the call reads classes of exact alleles where it reads alleles
	uint32_t prim_cap = 0; // decomposed: the longest text that is aligned
	povu_hip_call_profile_opts prof; // (raw-graph without a profile)
	std::vector<uint32_t> ref_of_path, slot_first, qa, qz; // reference number of every path (NO_QUERY: none), first slot of every sample, the queries
	std::vector<uint8_t> qor;
};
// cl_ws and cl_slot: the references, the sites' callability, the slot table, the flubble records before they have rows
struct CallWs {
	std::vector<uint64_t> ref_base; // first reference step of every reference, the references concatenated
	uint64_t NR;			// reference steps
	uint64_t *d_ref_base, *rlen64, *roff, *ilen, *atl, *s64;
	uint32_t *d_ref_path, *d_ref_of_path, *d_slot, *d_slot_first, *d_parent, *d_tree, *scnt, *soffv, *scur, *sval, *qv, *hit, *pres, *keep, *qidx,
		*words;
	uint8_t *d_fam, *callable, *called, *rflag;
	uint32_t *zc, *d_height; // per site: alleles without an inner base, PVST height
	uint32_t n_eal = 0; // the alleles the call reads: the exact alleles, or with POVU_HIP_T_NESTED the classes
	CallView v;	    // what the kernels read of all this (call_common.hpp)
	SlotsView slots;
	NestClasses nc;
	ClusterClasses cc;
	uint32_t n_vanished = 0;
	NestRecs nr;
	uint8_t *collapsed, *rstate;		    // per site / per flubble record before the sort (RS_*)
	uint64_t *xilen, *xatl, *ref_len, *max_len; // per flubble record: its own REF's inner bases and AT width, its written lengths
	uint32_t nfl_all = 0, n_collapsed = 0;	    // flubble records before the profile dropped any
	uint32_t *rlist, *perm, *perm2, *key, *key2; // perm: the flubble records sorted by (reference, POS), once flubble_records has run
	uint64_t *pos;
	void *tmp;
	size_t tmp_bytes;
	uint32_t nQ = 0, nfl = 0; // kept sites, flubble records
	uint32_t *smin, *smax;
	NormRecs nm; // left-normalized profile: per flubble record what the normalisation found
	// POVU_HIP_T_OFFREF: `refs` stays the view of the reference paths (callability and the inversions read it), v.ref becomes
	// that of the calling paths (references and surrogates, ascending) once surrogate_offsets has run
	RefView refs;
	std::vector<uint64_t> path_off, call_base; // the paths' first words; first step of every calling path, concatenated
	std::vector<uint32_t> call_path;
	OffrefSites os;
	OffrefHosts oh;
	RegionDevice rg; // region calls: the marks and the passing sites (rg.pass null: no regions)
};
// the inversion records and where the flubble records go in the one list
struct CallInv {
	InvIn in;
	InvDevice v;
	uint32_t *f_dst = nullptr;
};
// cl_rec: the per-record arrays and the spelling's inputs
struct CallRecs {
	uint32_t nrec = 0; // records
	BlockLayout L;	   // their blocks of spelled alleles
	uint32_t *xneed, *xoff, *xlist, *xrow, *o_level, *o_parent; // the extra blocks (REFs spelled on their own)
	uint8_t *rec_clustered; // clustered calls: per record
	uint8_t *o_star = nullptr; // POVU_HIP_T_SPANNING: per record, its last ALT is `*` (else null)
	uint32_t *cl_minsim;
	uint64_t *ref_spelled;
	uint64_t n_ac = 0; // ALT counts
	InvRows rows;
	uint32_t *need, *boff, *blist;
	uint64_t *ac_off, *bcnt, *block_off;
	NormRows nrows; // left-normalized profile: the rows' fields, the changed records in sorted order
};
// cl_spell and cl_bytes
struct CallSpelled {
	uint32_t *ac, *cl_nx;
	uint64_t *sp_off, *at_off;
	char *o_seq, *o_at;
	uint64_t nbytes[2] = {0, 0};
	std::vector<uint64_t> h_roff; // bases in front of every reference's first step
};

// the host-side refusals and the host tables
CallInputs check_call_inputs(povu_hip_ctx *ctx, const povu_hip_sites *sites, const povu_hip_call_refs *refs, const uint32_t *slot_of_path,
			     const povu_hip_trav_opts *opts, const povu_hip_call_profile_opts *profile, const povu_hip_call_regions *regions,
			     const povu_hip_call_cluster_opts *cluster)
{
	if (!ctx || !sites || !refs)
		throw HipError("null context, sites or references");
	if (!ctx->g.block)
		throw HipError("a call needs a resident graph (povu_hip_graph_upload first)");
	if (!ctx->seq_valid || ctx->seq_gen != ctx->g.gen)
		throw HipError("no sequences are resident for the graph now uploaded (povu_hip_segments_upload after povu_hip_graph_upload)");
	if (!ctx->paths_valid || ctx->paths_gen != ctx->g.gen)
		throw HipError("no paths are resident for the graph now uploaded (povu_hip_paths_upload after povu_hip_graph_upload)");
	CallInputs in{sites, refs, slot_of_path, opts, sites->n, ctx->n_paths, refs->n_refs, refs->n_slots, refs->n_samples};
	const uint32_t n = in.n, P = in.P, nR = in.nR, S = in.S, NS = in.NS;
	const uint32_t tflags = opts ? opts->flags : 0;
	in.prof = profile ? *profile : povu_hip_call_profile_opts{POVU_HIP_PROFILE_RAW_GRAPH, 0, 0, 0};
	if (in.prof.profile > POVU_HIP_PROFILE_DECOMPOSED)
		throw HipError("unknown profile " + std::to_string(in.prof.profile));
	// which modes combine: call_modes.hpp.  The refusal is thrown at the stage its rule names, among the other checks
	const uint32_t asked = in.prof.profile;
	const modes::Rule *no = modes::refused(modes::LIBRARY, modes::set_of(tflags, regions && regions->n, cluster && cluster->min_similarity_ppm), asked);
	auto refuse = [&](modes::Stage at) {
		if (no && no->stage == at)
			throw HipError(modes::message(*no, modes::LIBRARY, asked));
	};
	refuse(modes::AT_FLAGS);
	in.inversions = tflags & POVU_HIP_T_INVERSIONS;
	in.offref = tflags & POVU_HIP_T_OFFREF;
	in.untangle = tflags & POVU_HIP_T_UNTANGLE;
	in.merge = tflags & POVU_HIP_T_MERGE;
	in.normalized = asked == POVU_HIP_PROFILE_LEFT_NORMALIZED; // (keeps every record, ignores the limits, implies nothing)
	in.decomposed = asked == POVU_HIP_PROFILE_DECOMPOSED;	   // (the same; max_allele_length is the cap of the aligner)
	if (in.decomposed) {
		if (in.prof.max_allele_length > POVU_HIP_PRIM_MAX_LENGTH)
			throw HipError("max_allele_length " + std::to_string(in.prof.max_allele_length) + " is above the ceiling " +
				       std::to_string(POVU_HIP_PRIM_MAX_LENGTH) + " of the decomposed profile");
		in.prim_cap = in.prof.max_allele_length ? (uint32_t)in.prof.max_allele_length : POVU_HIP_PRIM_MAX_LENGTH;
	}
	if (in.normalized || in.decomposed)
		in.prof = povu_hip_call_profile_opts{POVU_HIP_PROFILE_RAW_GRAPH, 0, 0, 0};
	in.nested = (tflags & POVU_HIP_T_NESTED) || in.prof.profile != POVU_HIP_PROFILE_RAW_GRAPH;
	// the spanning alleles are an option of the nested call, no mode of their own: their refusals stand here, not in the table
	in.spanning = (tflags & POVU_HIP_T_SPANNING) != 0;
	if (in.spanning)
		if (const char *why = span_refused(false, in.nested, asked))
			throw HipError(why);
	if (cluster && cluster->min_similarity_ppm) {
		const std::string who = "a clustered call (povu_hip_call_clustered) is refused ";
		if (cluster->min_similarity_ppm > cluster::PPM)
			throw HipError(who + "with a threshold of " + std::to_string(cluster->min_similarity_ppm) + " ppm: at most 1000000");
		if (cluster->flags & ~POVU_HIP_CLUSTER_NO_BOUND)
			throw HipError(who + "with unknown cluster flags");
		in.cluster_ppm = cluster->min_similarity_ppm;
		in.cluster_no_bound = (cluster->flags & POVU_HIP_CLUSTER_NO_BOUND) != 0;
	}
	refuse(modes::AT_CLUSTER);
	if (n >= 0x7FFFFFFFu)
		throw HipError("too many sites");
	if (n && (!sites->id1 || !sites->id2 || !sites->or1 || !sites->or2 || !sites->parent || !sites->family || !sites->tree))
		throw HipError("null site arrays");
	if (!nR || !refs->ref_path)
		throw HipError("no reference path");
	if (!slot_of_path || !S || !NS || !refs->sample_of_slot)
		throw HipError("no genotype slots");
	in.ref_of_path.assign(P, NO_QUERY);
	in.slot_first.assign(NS + 1, 0);
	for (uint32_t r = 0; r < nR; r++) {
		if (refs->ref_path[r] >= P || (r && refs->ref_path[r] <= refs->ref_path[r - 1]))
			throw HipError("reference paths must be ascending indices of resident paths");
		in.ref_of_path[refs->ref_path[r]] = r;
	}
	for (uint32_t k = 0; k < P; k++)
		if (slot_of_path[k] >= S)
			throw HipError("path " + std::to_string(k) + " has no genotype slot");
	for (uint32_t sl = 0; sl < S; sl++) {
		const uint32_t sm = refs->sample_of_slot[sl];
		if (sm >= NS || (sl && sm < refs->sample_of_slot[sl - 1]) || (sl && sm > refs->sample_of_slot[sl - 1] + 1) || (!sl && sm))
			throw HipError("the slots of a sample must be consecutive, samples in order");
		in.slot_first[sm + 1] = sl + 1;
	}
	in.qa.resize(n), in.qz.resize(n), in.qor.resize(n);
	for (uint32_t q = 0; q < n; q++) {
		if (sites->parent[q] != POVU_HIP_NIL && sites->parent[q] >= n)
			throw HipError("site " + std::to_string(q) + " has a parent that is no site");
		in.n_trees = std::max(in.n_trees, sites->tree[q] + 1);
		in.qa[q] = sites->id1[q];
		in.qz[q] = sites->id2[q];
		in.qor[q] = (uint8_t)((sites->or1[q] & 1u) | ((sites->or2[q] & 1u) << 1));
	}
	refuse(modes::AT_END);
	return in;
}

// the reference steps concatenated, the call's workspace and uploads, the bases in front of every reference step
void reference_offsets(povu_hip_ctx *ctx, const CallInputs &in, const TravDevice &d, CallWs &w)
{
	const ResidentGraph &g = ctx->g;
	hipStream_t s = ctx->stream;
	const uint32_t n = in.n, P = in.P, nR = in.nR, NS = in.NS, R = d.R;
	std::vector<uint64_t> &path_off = w.path_off;
	path_off.resize((size_t)P + 1);
	w.ref_base.assign((size_t)nR + 1, 0);
	HIP_CHECK(copy_async(path_off.data(), ctx->path_off, ((size_t)P + 1) * 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	for (uint32_t r = 0; r < nR; r++)
		w.ref_base[r + 1] = w.ref_base[r] + path_off[in.refs->ref_path[r] + 1] - path_off[in.refs->ref_path[r]];
	const uint64_t NR = w.NR = w.ref_base[nR];
	const size_t n1 = (size_t)n + 1, hit_words = ((uint64_t)n * nR * 2 + 31) / 32 + 1, pres_words = ((uint64_t)in.n_trees * nR + 31) / 32 + 1;
	w.tmp_bytes = std::max(prim_tmp_bytes(std::max<size_t>({(size_t)g.V + 1, n1, 2 * (size_t)n + 1}), false), prim_tmp_bytes((size_t)R + 1, true)) + 256;
	carve(ctx->cl_ws, [&](Spans &take) {
		take((size_t)nR + 1, w.d_ref_base, w.d_ref_path);
		take((size_t)P + 1, w.d_ref_of_path, w.d_slot);
		take((size_t)NS + 1, w.d_slot_first);
		take(n1, w.d_parent, w.d_tree, w.d_fam, w.callable, w.called, w.zc, w.d_height, w.collapsed, w.keep, w.qidx);
		take(NR + 1, w.rlen64, w.roff);
		take((size_t)g.V + 1, w.scnt, w.soffv, w.scur);
		take(2 * n1, w.sval, w.qv);
		take(hit_words, w.hit);
		take(pres_words, w.pres);
		take((size_t)d.n_al + 1, w.ilen, w.atl);
		take((size_t)R + 1, w.rflag, w.rlist, w.perm, w.perm2, w.key, w.key2, w.pos, w.rstate, w.xilen, w.xatl, w.ref_len, w.max_len);
		take(scan_exclusive_u64_tmp(std::max<uint64_t>(NR + 1, 1)), w.s64);
		take(8, w.words);
		take(w.tmp_bytes, w.tmp);
	});
	// the views: everything but the allele table (site_classes) and the number of flubble records (flubble_records)
	CallView &v = w.v;
	v.paths = paths_view(ctx), v.trav = trav_view(d), v.ref = w.refs = RefView{NR, nR, w.d_ref_of_path, w.d_ref_path, w.d_ref_base, w.roff};
	v.on_ref = w.d_ref_of_path, v.sur = nullptr;
	v.ilen = w.ilen, v.atl = w.atl, v.keep = w.keep, v.zc = w.zc, v.height = w.d_height;
	v.nfl = 0, v.rlist = w.rlist, v.rstate = w.rstate, v.xilen = w.xilen, v.xatl = w.xatl, v.ref_len = w.ref_len, v.max_len = w.max_len;
	v.raw_pos = v.pos = w.pos; // (one array until a left-normalisation moves `pos` and keeps the raw POS itself)
	w.slots = SlotsView{in.S, NS, w.d_slot, w.d_slot_first};
	HIP_CHECK(copy_async(w.d_ref_base, w.ref_base.data(), ((size_t)nR + 1) * 8, hipMemcpyHostToDevice, s));
	HIP_CHECK(copy_async(w.d_ref_path, in.refs->ref_path, (size_t)nR * 4, hipMemcpyHostToDevice, s));
	if (P) {
		HIP_CHECK(copy_async(w.d_ref_of_path, in.ref_of_path.data(), (size_t)P * 4, hipMemcpyHostToDevice, s));
		HIP_CHECK(copy_async(w.d_slot, in.slot_of_path, (size_t)P * 4, hipMemcpyHostToDevice, s));
	}
	HIP_CHECK(copy_async(w.d_slot_first, in.slot_first.data(), ((size_t)NS + 1) * 4, hipMemcpyHostToDevice, s));
	if (n) {
		HIP_CHECK(copy_async(w.d_parent, in.sites->parent, (size_t)n * 4, hipMemcpyHostToDevice, s));
		HIP_CHECK(copy_async(w.d_tree, in.sites->tree, (size_t)n * 4, hipMemcpyHostToDevice, s));
		HIP_CHECK(copy_async(w.d_fam, in.sites->family, n, hipMemcpyHostToDevice, s));
		if (in.sites->height)
			HIP_CHECK(copy_async(w.d_height, in.sites->height, (size_t)n * 4, hipMemcpyHostToDevice, s));
		else
			HIP_CHECK(hipMemsetAsync(w.d_height, 0, (size_t)n * 4, s));
	}
	HIP_CHECK(hipMemsetAsync(w.words, 0, 32, s));
	HIP_CHECK(hipMemsetAsync(w.scnt, 0, ((size_t)g.V + 1) * 4, s));
	HIP_CHECK(hipMemsetAsync(w.scur, 0, ((size_t)g.V + 1) * 4, s));
	HIP_CHECK(hipMemsetAsync(w.hit, 0, hit_words * 4, s));
	HIP_CHECK(hipMemsetAsync(w.pres, 0, pres_words * 4, s));

	HIP_CHECK(hipMemsetAsync(w.rlen64 + NR, 0, 8, s));
	if (NR)
		KLAUNCH(k_cl_ref_len, dim3(stride_blocks(NR)), dim3(Q_TPB), 0, s, v.ref, v.paths, w.rlen64);
	scan_exclusive_u64(w.rlen64, w.roff, NR + 1, w.s64, s);
}

// the called sites
void callability(povu_hip_ctx *ctx, const CallInputs &in, const TravDevice &d, CallWs &w)
{
	const ResidentGraph &g = ctx->g;
	hipStream_t s = ctx->stream;
	const uint32_t n = in.n, nR = in.nR;
	const uint64_t NR = w.NR;
	if (n) {
		KLAUNCH(k_cl_seg_count, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, d.q.qa, d.q.qz, g.vid, g.V, w.scnt, w.qv);
		scan_exclusive_u32(w.scnt, w.soffv, (size_t)g.V + 1, w.tmp, w.tmp_bytes, s);
		KLAUNCH(k_cl_seg_fill, dim3(stride_blocks(2 * (size_t)n)), dim3(Q_TPB), 0, s, n, w.qv, w.soffv, w.scur, w.sval);
		if (NR)
			KLAUNCH(k_cl_hits, dim3(stride_blocks(NR)), dim3(Q_TPB), 0, s, w.refs, w.v.paths, w.soffv, w.sval, w.hit);
		KLAUNCH(k_cl_present, dim3(stride_blocks((size_t)n * nR)), dim3(Q_TPB), 0, s, (uint64_t)n, nR, w.hit, w.d_tree, w.pres);
		KLAUNCH(k_cl_callable, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, nR, w.hit, w.pres, w.d_tree, w.d_parent, w.d_fam, w.callable, w.called);
		KLAUNCH(k_cl_unparent, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, w.callable, w.d_parent, w.called);
	}
}

// POVU_HIP_T_OFFREF: the sites called off-reference and their surrogates; `called` becomes the union
void offref_sites_step(povu_hip_ctx *ctx, const CallInputs &in, const TravDevice &d, CallWs &w)
{
	w.os = offref_sites(ctx, d, in.n, w.d_parent, w.d_fam, w.callable, w.called, w.d_ref_of_path);
	w.v.sur = w.os.sur;
}
// ... the offsets of the calling paths, exactly as for the references: their steps concatenated, k_cl_ref_len's gather, one
// u64 scan; the call's view of "the reference paths" is theirs from here on
void surrogate_offsets(povu_hip_ctx *ctx, const CallInputs &in, CallWs &w)
{
	hipStream_t s = ctx->stream;
	const uint32_t nC = w.os.n_call;
	w.call_path.resize(nC);
	if (nC)
		HIP_CHECK(copy_async(w.call_path.data(), w.os.call_path, (size_t)nC * 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	w.call_base.assign((size_t)nC + 1, 0);
	for (uint32_t k = 0; k < nC; k++) {
		if (w.call_path[k] >= in.P)
			throw HipError("off-reference calls: a calling path is no resident path");
		w.call_base[k + 1] = w.call_base[k] + w.path_off[w.call_path[k] + 1] - w.path_off[w.call_path[k]];
	}
	const uint64_t NC = w.call_base[nC];
	const OffrefView ov = offref_view(ctx, w.os, NC);
	HIP_CHECK(copy_async(ov.ref_base, w.call_base.data(), ((size_t)nC + 1) * 8, hipMemcpyHostToDevice, s));
	w.v.ref = RefView{NC, nC, ov.ref_of_path, w.os.call_path, ov.ref_base, ov.roff};
	HIP_CHECK(hipMemsetAsync(ov.rlen + NC, 0, 8, s));
	if (NC)
		KLAUNCH(k_cl_ref_len, dim3(stride_blocks(NC)), dim3(Q_TPB), 0, s, w.v.ref, w.v.paths, ov.rlen);
	scan_exclusive_u64(ov.rlen, ov.roff, NC + 1, ov.s64, s);
}

// what the rest of the call reads as the alleles of a site: the exact alleles, or the classes of a nested call
void site_classes(povu_hip_ctx *ctx, const CallInputs &in, const TravDevice &d, CallWs &w)
{
	CallView &v = w.v;
	v.aoff = d.aoff, v.oa = d.oa, v.afirst = d.afirst, v.crep = nullptr, w.n_eal = d.n_al;
	if (in.cluster_ppm) {
		w.cc = cluster_classes(ctx, d, w.called, in.cluster_ppm, in.cluster_no_bound, in.opts && (in.opts->flags & POVU_HIP_T_FORCE_TIER2));
		v.aoff = w.cc.coff, v.oa = w.cc.oc, v.afirst = w.cc.cfirst, v.crep = w.cc.crep, w.n_eal = w.cc.n_cl;
		return;
	}
	if (!in.nested)
		return;
	w.nc = nest_classes(ctx, d, w.called, in.opts && in.opts->max_steps ? in.opts->max_steps : 65536,
			    in.opts && (in.opts->flags & POVU_HIP_T_FORCE_TIER2));
	v.aoff = w.nc.coff, v.oa = w.nc.oc, v.afirst = w.nc.cfirst, v.crep = w.nc.crep, w.n_eal = w.nc.n_cl;
}

// the sites kept (called, two alleles or more), their alleles' inner lengths
void kept_sites(povu_hip_ctx *ctx, const CallInputs &in, const TravDevice &d, CallWs &w)
{
	hipStream_t s = ctx->stream;
	const uint32_t n = in.n, n_al = w.n_eal;
	const size_t n1 = (size_t)n + 1;
	KLAUNCH(k_cl_keep, dim3(stride_blocks(n1)), dim3(Q_TPB), 0, s, n, w.called, w.v.aoff, w.keep, w.words + 1);
	scan_exclusive_u32(w.keep, w.qidx, n1, w.tmp, w.tmp_bytes, s);
	uint32_t hw[2] = {0, 0};
	HIP_CHECK(copy_async(hw, w.qidx + n, 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(copy_async(hw + 1, w.words + 1, 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	w.nQ = hw[0];
	if (hw[1] > MAX_ALLELES)
		throw HipError("a called site has " + std::to_string(hw[1]) + " alleles: more than 65534 in one record are refused");
	if (n_al)
		KLAUNCH(k_cl_inner, dim3(stride_blocks(n_al)), dim3(Q_TPB), 0, s, n_al, w.v, w.ilen, w.atl);
	if (n)
		KLAUNCH(k_cl_zero_len, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, w.keep, w.v.aoff, w.ilen, w.zc);
	if (n && in.classes()) {
		KLAUNCH(k_cl_collapsed, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, w.keep, d.aoff, w.v.aoff, w.called, w.collapsed, w.words + 3, w.words + 5);
		w.n_collapsed = read_back(w.words + 3, s);
		w.n_vanished = read_back(w.words + 5, s);
	}
}

// per kept site and genotype slot, the min and max allele
void slot_table(povu_hip_ctx *ctx, const CallInputs &in, const TravDevice &d, CallWs &w)
{
	hipStream_t s = ctx->stream;
	const size_t cells = (size_t)w.nQ * in.S + 1;
	carve(ctx->cl_slot, [&](Spans &take) { take(cells, w.smin, w.smax); });
	HIP_CHECK(hipMemsetAsync(w.smin, 0xFF, cells * 4, s));
	HIP_CHECK(hipMemsetAsync(w.smax, 0, cells * 4, s));
	if (d.R && w.nQ)
		KLAUNCH(k_cl_slots, dim3(stride_blocks(d.R)), dim3(Q_TPB), 0, s, d.R, d.rq, d.op, w.v.oa, w.keep, w.qidx, w.d_slot, in.S, w.smin, w.smax);
}

// flag, compact, POS, the sort by (reference, POS)
void flubble_records(povu_hip_ctx *ctx, const CallInputs &in, const TravDevice &d, CallWs &w)
{
	hipStream_t s = ctx->stream;
	const uint32_t R = d.R, nR = w.v.ref.nR; // (the calling paths)
	if (R && w.nQ) {
		KLAUNCH(k_cl_rec_flag, dim3(stride_blocks(R)), dim3(Q_TPB), 0, s, w.v, w.rflag);
		compact_flagged_u8(w.rflag, R, w.rlist, w.words + 2, w.tmp, w.tmp_bytes, s);
		w.nfl = read_back(w.words + 2, s);
	}
	const uint32_t nfl_all = w.nfl_all = w.v.nfl = w.nfl;
	refuse_2_32(nfl_all, "the call needs ", "records");
	const uint64_t ref_bases = read_back(w.v.ref.roff + w.v.ref.NR, s);
	if (!nfl_all)
		return;
	// per record: anchored, REF's own lengths; POS; with POVU_HIP_T_NESTED parents, levels and the profile's choice
	const bool filter = in.prof.profile != POVU_HIP_PROFILE_RAW_GRAPH;
	KLAUNCH(k_cl_rec_state, dim3(stride_blocks(nfl_all)), dim3(Q_TPB), 0, s, w.v, filter ? 1u : 0u, w.rstate, w.xilen, w.xatl, w.ref_len, w.max_len);
	KLAUNCH(k_cl_pos, dim3(stride_blocks(nfl_all)), dim3(Q_TPB), 0, s, w.v, w.pos);
	if (in.normalized) { // chop, shift and trim of every record, its POS moved before the sort keys are made
		w.nm = norm_records(ctx, w.v, w.rstate, w.pos);
		w.v.raw_pos = w.nm.raw_pos;
	}
	if (in.nested) {
		NestSpan span;
		if (in.spanning)
			span = NestSpan{true, w.qidx, w.smin, w.d_slot, in.S, w.rg.pass};
		w.nr = nest_records(ctx, w.v, w.nc.ix, in.prof, span);
		w.nfl = w.nr.n_kept;
		if (w.nfl)
			HIP_CHECK(copy_async(w.perm, w.nr.kept, (size_t)w.nfl * 4, hipMemcpyDeviceToDevice, s));
	} else {
		launch_iota(nfl_all, w.perm, s);
	}
	if (w.rg.pass && w.nfl) { // region calls: the records of the passing sites alone, in front of the sort
		const uint32_t kept = region_select(ctx, w.v, w.rg.pass, w.perm, w.nfl, w.rflag, w.key, w.perm2, w.words + 4, w.tmp, w.tmp_bytes);
		w.rg.n_dropped = w.nfl - kept;
		w.nfl = kept;
		std::swap(w.perm, w.perm2);
	}
	const uint32_t nfl = w.nfl;
	if (!nfl)
		return;
	LsdSort sort{w.perm, w.perm2, w.key, w.key2, nfl, w.tmp, w.tmp_bytes, s};
	auto write_key = [&](int which, const uint32_t *perm, uint32_t *k) {
		KLAUNCH(k_cl_key, dim3(stride_blocks(nfl)), dim3(Q_TPB), 0, s, nfl, which, perm, w.v, k);
	};
	sort.pass(0, 32, write_key);
	if (ref_bases + 1 >= (1ull << 32))
		sort.pass(1, 32, write_key);
	if (nR > 1)
		sort.pass(2, bits_for(nR), write_key);
	w.perm = sort.cur;
}

// POVU_HIP_T_OFFREF: the rows' arrays, and the surrogates that are no reference path with their lengths
struct CallOffref {
	OffrefRows rows;
	std::vector<uint32_t> contig_path;
	std::vector<uint64_t> contig_len;
};
void offref_rows_step(povu_hip_ctx *ctx, const CallInputs &in, const CallWs &w, const CallInv &inv, const CallRecs &r, CallOffref &o)
{
	hipStream_t s = ctx->stream;
	o.rows = offref_rows(ctx, w.v, w.os, w.oh, r.nrec, w.nfl, w.perm, inv.f_dst);
	const uint32_t nC = w.os.n_call;
	std::vector<uint64_t> at((size_t)nC + 1, 0);
	for (uint32_t k = 0; k <= nC; k++)
		HIP_CHECK(copy_async(at.data() + k, w.v.ref.roff + w.call_base[k], 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	for (uint32_t k = 0; k < nC; k++)
		if (in.ref_of_path[w.call_path[k]] == NO_QUERY) {
			o.contig_path.push_back(w.call_path[k]);
			o.contig_len.push_back(at[k + 1] - at[k]);
		}
}

// the inversion records, and every record's row in the one list; gives the number of all records
uint32_t inversion_rows(povu_hip_ctx *ctx, const CallInputs &in, const CallWs &w, CallInv &inv)
{
	hipStream_t s = ctx->stream;
	const uint32_t nfl = w.nfl;
	if (!in.inversions)
		return nfl;
	InvIn &iin = inv.in;
	iin.paths = w.v.paths, iin.ref = w.refs, iin.slots = w.slots;
	iin.max_steps = in.opts->max_steps ? in.opts->max_steps : 65536;
	iin.force_tier2 = (in.opts->flags & POVU_HIP_T_FORCE_TIER2) != 0;
	iin.marked = w.rg.marked;
	inv.v = inv_find(ctx, iin);
	refuse_2_32((uint64_t)nfl + inv.v.n, "the call needs ", "records");
	if (!inv.v.n)
		return nfl;
	uint32_t *f_ref;
	uint64_t *f_pos;
	carve(ctx->iv_rows, [&](Spans &take) { take((size_t)nfl + 1, f_ref, inv.f_dst, f_pos); });
	if (nfl)
		KLAUNCH(k_cl_sorted_keys, dim3(stride_blocks(nfl)), dim3(Q_TPB), 0, s, nfl, w.perm, w.v, f_ref, f_pos);
	if (in.offref) { // the one list is ordered by the calling paths: the inversion records' references numbered among them
		InvDevice m = inv.v;
		m.ref = offref_inv_refs(ctx, inv.v.n, inv.v.ref, w.refs.ref_path, w.v.ref.ref_of_path);
		inv_merge(ctx, m, nfl, f_ref, f_pos, inv.f_dst);
	} else {
		inv_merge(ctx, inv.v, nfl, f_ref, f_pos, inv.f_dst);
	}
	return nfl + inv.v.n;
}

// the per-record fields, the AC offsets, the blocks a record needs spelled and their alleles
void record_arrays(povu_hip_ctx *ctx, const CallInputs &in, const CallWs &w, const CallInv &inv, CallRecs &r)
{
	hipStream_t s = ctx->stream;
	const uint32_t n = in.n, nfl = w.nfl, nrec = r.nrec;
	const InvDevice &iv = inv.v;
	const size_t r1 = (size_t)nrec + 1, n2 = 4 * (size_t)n + 1, f1 = (size_t)nfl + 1;
	InvRows &o = r.rows;
	NormRows &nw = r.nrows;
	uint64_t *s64;
	uint32_t nn = 0; // records the normalisation changed
	carve(ctx->cl_rec, [&](Spans &take) {
		take(r1, o.o_q, o.o_path, o.o_first, o.o_ref, o.o_nal, o.o_an, o.o_ns, o.o_block, o.o_nsteps, o.o_pos, o.nalt, r.ac_off, o.o_flags);
		take(r1, r.o_level, r.o_parent, r.xrow, r.ref_spelled);
		take(in.cluster_ppm ? r1 : 1, r.rec_clustered, r.cl_minsim);
		if (in.spanning) // (without the option the arena is laid out as before)
			take(r1, r.o_star);
		take(f1, r.xneed, r.xoff, r.xlist);
		take((size_t)nrec * in.S + 1, o.gt);
		take(n2, r.need, r.boff, r.blist);
		take(n2 + 2 * (size_t)nfl + iv.n, r.bcnt, r.block_off);
		take(scan_exclusive_u64_tmp(std::max(r1, n2 + 2 * (size_t)nfl + iv.n)), s64);
		take(in.normalized ? r1 : 1, nw.o_raw_pos, nw.o_block, nw.o_shift, nw.o_chop, nw.o_trim);
		take(in.normalized ? f1 : 1, nw.need, nw.off, nw.list);
	});
	HIP_CHECK(hipMemsetAsync(o.o_nsteps, 0, r1 * 4, s));
	HIP_CHECK(hipMemsetAsync(r.need, 0, n2 * 4, s));
	HIP_CHECK(hipMemsetAsync(o.nalt + nrec, 0, 8, s));
	HIP_CHECK(hipMemsetAsync(r.o_level, 0, r1 * 4, s));
	HIP_CHECK(hipMemsetAsync(r.o_parent, 0xFF, r1 * 4, s));
	HIP_CHECK(hipMemsetAsync(r.xrow, 0xFF, r1 * 4, s));
	HIP_CHECK(hipMemsetAsync(r.xneed, 0, f1 * 4, s));
	if (in.spanning)
		HIP_CHECK(hipMemsetAsync(r.o_star, 0, r1, s)); // (an inversion record never carries a `*`)
	if (nfl)
		KLAUNCH(k_cl_rec_fields, dim3(stride_blocks(nfl)), dim3(Q_TPB), 0, s, nfl, w.perm, w.v, o, r.need, inv.f_dst, in.nested ? w.nr.level : nullptr,
			in.nested ? w.nr.parent_q : nullptr, r.o_level, r.o_parent, r.xneed, w.nr.star, r.o_star);
	inv_fields(ctx, inv.in, iv, o);
	if (in.normalized) {
		// every row as an unchanged record's (the inversion records stay so), then the flubble records' own
		HIP_CHECK(hipMemsetAsync(nw.o_block, 0xFF, r1 * 4, s));
		HIP_CHECK(hipMemsetAsync(nw.o_shift, 0, r1 * 4, s));
		HIP_CHECK(hipMemsetAsync(nw.o_chop, 0, r1 * 4, s));
		HIP_CHECK(hipMemsetAsync(nw.o_trim, 0, r1 * 4, s));
		if (nrec)
			HIP_CHECK(copy_async(nw.o_raw_pos, o.o_pos, (size_t)nrec * 8, hipMemcpyDeviceToDevice, s));
		norm_row_fields(ctx, w.v, w.nm, nfl, w.perm, inv.f_dst, nw);
		scan_exclusive_u32(nw.need, nw.off, f1, w.tmp, w.tmp_bytes, s);
		HIP_CHECK(copy_async(&nn, nw.off + nfl, 4, hipMemcpyDeviceToHost, s));
	}
	scan_exclusive_u64(o.nalt, r.ac_off, r1, s64, s);
	HIP_CHECK(copy_async(&r.n_ac, r.ac_off + nrec, 8, hipMemcpyDeviceToHost, s));
	scan_exclusive_u32(r.need, r.boff, n2, w.tmp, w.tmp_bytes, s);
	BlockLayout &L = r.L;
	HIP_CHECK(copy_async(&L.nfc, r.boff + 4 * (size_t)n, 4, hipMemcpyDeviceToHost, s));
	uint32_t nx = 0; // the extra blocks: the REFs of a call with classes that are no representatives
	if (in.classes() && nfl) {
		scan_exclusive_u32(r.xneed, r.xoff, f1, w.tmp, w.tmp_bytes, s);
		HIP_CHECK(copy_async(&nx, r.xoff + nfl, 4, hipMemcpyDeviceToHost, s));
	}
	HIP_CHECK(hipStreamSynchronize(s));
	if (n)
		KLAUNCH(k_cl_blocks, dim3(stride_blocks(4 * (size_t)n)), dim3(Q_TPB), 0, s, 4 * (uint64_t)n, r.need, r.boff, r.blist);
	// the four families of blocks in the layout's order: one extra block per own REF, one block per inversion record, one per
	// record the normalisation changed
	refuse_2_32((uint64_t)L.nfc + nx, "the call needs ", "blocks");
	L.nfb = L.nfc + nx;
	refuse_2_32((uint64_t)L.nfb + iv.n, "the call needs ", "blocks");
	L.nb0 = L.nfb + iv.n;
	refuse_2_32((uint64_t)L.nb0 + nn, "the call needs ", "blocks");
	L.nb = L.nb0 + nn;
	HIP_CHECK(hipMemsetAsync(r.bcnt + L.nb, 0, 8, s));
	if (L.nfc)
		KLAUNCH(k_cl_block_cnt, dim3(stride_blocks(L.nfc)), dim3(Q_TPB), 0, s, L.nfc, r.blist, w.v.aoff, r.bcnt);
	if (nx)
		KLAUNCH(k_cl_extra, dim3(stride_blocks(nfl)), dim3(Q_TPB), 0, s, nfl, w.perm, w.rstate, r.xoff, L, r.xlist, r.bcnt);
	inv_genotypes(ctx, inv.in, iv, o, L.inversion().b0, r.bcnt);
	if (nn)
		norm_blocks(ctx, w.v, nfl, w.perm, inv.f_dst, nw, L.normalised().b0, r.bcnt);
	scan_exclusive_u64(r.bcnt, r.block_off, (size_t)L.nb + 1, s64, s);
	HIP_CHECK(copy_async(&L.nsp, r.block_off + L.nb, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(copy_async(&L.nsp0, r.block_off + L.nb0, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(copy_async(&L.nfsp, r.block_off + L.nfb, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
}

// GT rows and counts, then the spelled alleles: lengths, offsets, bytes, the bad-byte refusal
void spelling(povu_hip_ctx *ctx, const CallInputs &in, const CallWs &w, const CallInv &inv, const CallRecs &r, CallSpelled &sp)
{
	hipStream_t s = ctx->stream;
	const uint32_t nR = in.nR, nfl = w.nfl;
	const BlockLayout &L = r.L;
	const uint64_t nsp = L.nsp, nfsp = L.flubble().ns;
	const InvDevice &iv = inv.v;
	const InvRows &o = r.rows;
	uint64_t *slen, *alen, *s64;
	unsigned long long *bad;
	carve(ctx->cl_spell, [&](Spans &take) {
		take(r.n_ac + 1, sp.ac);
		take(in.cluster_ppm ? r.n_ac + r.nrec + 1 : 1, sp.cl_nx);
		take(nsp + 1, slen, alen, sp.sp_off, sp.at_off);
		take(scan_exclusive_u64_tmp(nsp + 1), s64);
		take(1, bad);
	});
	HIP_CHECK(hipMemsetAsync(sp.ac, 0, (r.n_ac + 1) * 4, s));
	HIP_CHECK(hipMemsetAsync(bad, 0xFF, 8, s));
	if (nfl) {
		auto *records = w.nr.span_bits ? k_cl_records<true> : k_cl_records<false>;
		KLAUNCH(records, dim3(wave_blocks(nfl)), dim3(Q_TPB), 0, s, nfl, w.v, w.slots, o, w.qidx, w.smin, w.smax, r.ac_off, w.perm,
			in.nested ? w.collapsed : nullptr, in.nested ? w.nr.rescued : nullptr, sp.ac, inv.f_dst,
			w.nr.span_bits, w.nr.span_words);
		KLAUNCH(k_cl_rec_block, dim3(stride_blocks(nfl)), dim3(Q_TPB), 0, s, nfl, w.perm, w.v, r.boff, o.o_block, inv.f_dst, r.xoff, r.xrow);
	}
	inv_counts(ctx, inv.in, iv, o, r.ac_off, sp.ac);
	if (in.cluster_ppm) { // (an inversion record: not clustered, no similarity, no exact alleles)
		HIP_CHECK(hipMemsetAsync(sp.cl_nx, 0, (r.n_ac + r.nrec + 1) * 4, s));
		HIP_CHECK(hipMemsetAsync(r.rec_clustered, 0, (size_t)r.nrec + 1, s));
		HIP_CHECK(hipMemsetAsync(r.cl_minsim, 0, ((size_t)r.nrec + 1) * 4, s));
		if (nfl)
			KLAUNCH(k_cl_provenance, dim3(stride_blocks(nfl)), dim3(Q_TPB), 0, s, nfl, w.perm, w.v, inv.f_dst, w.collapsed, w.cc.minsim, w.cc.csize,
				r.ac_off, r.rec_clustered, r.cl_minsim, sp.cl_nx);
	}
	HIP_CHECK(hipMemsetAsync(slen + nsp, 0, 8, s));
	HIP_CHECK(hipMemsetAsync(alen + nsp, 0, 8, s));
	const FlubbleBlocks B{L, r.block_off, r.blist, r.xlist};
	if (nfsp)
		KLAUNCH(k_cl_spell_len, dim3(stride_blocks(nfsp)), dim3(Q_TPB), 0, s, w.v, B, slen, alen);
	inv_spell_len(ctx, inv.in, iv, L, slen, alen);
	norm_spell_len(ctx, w.v, w.nm, r.nrows, L, r.block_off, slen, alen);
	scan_exclusive_u64(slen, sp.sp_off, nsp + 1, s64, s);
	scan_exclusive_u64(alen, sp.at_off, nsp + 1, s64, s);
	HIP_CHECK(copy_async(sp.nbytes, sp.sp_off + nsp, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(copy_async(sp.nbytes + 1, sp.at_off + nsp, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	carve(ctx->cl_bytes, [&](Spans &take) { take(sp.nbytes[0] + 1, sp.o_seq), take(sp.nbytes[1] + 1, sp.o_at); });
	if (nfsp)
		KLAUNCH(k_cl_emit, dim3(wave_blocks(nfsp)), dim3(Q_TPB), 0, s, w.v, B, sp.sp_off, sp.at_off, sp.o_seq, sp.o_at, bad);
	inv_emit(ctx, inv.in, iv, L, sp.sp_off, sp.at_off, sp.o_seq, sp.o_at, bad);
	norm_emit(ctx, w.v, w.nm, r.nrows, L, r.block_off, sp.sp_off, sp.o_seq, bad);
	if (r.nrec)
		KLAUNCH(k_cl_ref_spelled, dim3(stride_blocks(r.nrec)), dim3(Q_TPB), 0, s, r.nrec, o.o_block, o.o_ref, r.xrow, r.block_off, L, r.ref_spelled);
	uint64_t hbad = 0;
	HIP_CHECK(copy_async(&hbad, bad, 8, hipMemcpyDeviceToHost, s));
	sp.h_roff.resize(nR ? nR + 1 : 1);
	for (uint32_t k = 0; k <= nR; k++)
		HIP_CHECK(copy_async(sp.h_roff.data() + k, w.roff + w.ref_base[k], 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	if (hbad != ~0ull)
		throw HipError("segment " + std::to_string(read_back(ctx->g.vid + hbad, s)) + " holds a byte that is no nucleotide code (ACGTN, lower case, IUPAC)");
}

// POVU_HIP_T_UNTANGLE: the rows of the sites a path laps, rewritten from the lap alignments
UntangleRows untangle_step(povu_hip_ctx *ctx, const CallInputs &in, const CallWs &w, const CallInv &inv, const CallRecs &r, const CallSpelled &sp)
{
	UntangleIn u{};
	u.v = w.v, u.slots = w.slots, u.qidx = w.qidx, u.nQ = w.nQ;
	u.nfl = w.nfl, u.nrec = r.nrec, u.perm = w.perm, u.dst = inv.f_dst;
	u.rows = r.rows, u.smin = w.smin, u.smax = w.smax, u.ac_off = r.ac_off, u.ac = sp.ac;
	return untangle_rows(ctx, u);
}

// what the `decomposed` profile reads: every (REF, ALT) of the records as they are written (prim_kernels.hip aligns and splits
// them, merge_kernels.hip merges the rows)
PrimIn primitive_input(const CallInputs &in, const CallWs &w, const CallRecs &r, const CallSpelled &sp)
{
	const InvRows &o = r.rows;
	PrimIn p{};
	p.nrec = r.nrec, p.n_pairs = r.n_ac;
	p.ac_off = r.ac_off, p.pos = o.o_pos, p.ref_spelled = r.ref_spelled;
	p.path = o.o_path, p.ref_allele = o.o_ref, p.block = o.o_block, p.flags = o.o_flags, p.gt = o.gt;
	p.block_off = r.block_off, p.sp_off = sp.sp_off, p.seq = sp.o_seq;
	p.paths = w.v.paths, p.ref = w.v.ref, p.slots = w.slots;
	p.cap = in.prim_cap;
	p.force_tier2 = in.opts && (in.opts->flags & POVU_HIP_T_FORCE_TIER2);
	p.ref_bases = sp.h_roff.back() - sp.h_roff.front();
	return p;
}

povu_hip_calls *calls_to_host(povu_hip_ctx *ctx, const CallInputs &in, const CallWs &w, const CallInv &inv, const CallRecs &r, const CallSpelled &sp,
			      const PrimRows &pr, const MergedRows &mg, const CallOffref &orf, const UntangleRows &un, CallTimer &timer)
{
	const uint32_t nrec = r.nrec, nb = r.L.nb, nR = in.nR, S = in.S;
	const uint64_t nsp = r.L.nsp;
	const InvRows &d = r.rows;
	const NormRows &nw = r.nrows;
	const InvDevice &iv = inv.v;
	auto o = std::make_unique<CallsOwner>();
	povu_hip_calls &v = o->view;
	// a result array: the owner's vector, the field of the view, the n elements on the device.  The copies go in this order
	auto give = [&](auto &vec, auto &field, const auto *dev, size_t n) { hand_off(vec, n, dev, n, ctx), field = vec.data(); };
	// ... of the left-normalisation: per record; without the profile what says that nothing was normalised, filled on the host
	// once the device time is taken
	std::vector<std::function<void()>> defaults;
	auto give_norm = [&](auto &vec, auto &field, const auto *dev, auto fill) {
		if (in.normalized)
			return give(vec, field, dev, nrec);
		defaults.push_back([&vec, &field, fill] { fill(vec), field = vec.data(); });
	};
	auto all = [nrec](auto value) { return [=](auto &vec) { vec.assign(nrec, value); }; };
	give(o->query, v.query, d.o_q, nrec);
	give(o->path, v.path, d.o_path, nrec);
	give(o->first, v.first, d.o_first, nrec);
	give(o->ref_allele, v.ref_allele, d.o_ref, nrec);
	give(o->n_alleles, v.n_alleles, d.o_nal, nrec);
	give(o->an, v.an, d.o_an, nrec);
	give(o->ns, v.ns, d.o_ns, nrec);
	give(o->block, v.block, d.o_block, nrec);
	give(o->n_steps, v.n_steps, d.o_nsteps, nrec);
	give(o->pos, v.pos, d.o_pos, nrec);
	give(o->flags, v.flags, d.o_flags, nrec);
	give(o->level, v.level, r.o_level, nrec);
	give(o->parent_query, v.parent_query, r.o_parent, nrec);
	give(o->ref_spelled, v.ref_spelled, r.ref_spelled, nrec);
	give(o->ac_off, v.ac_off, r.ac_off, (size_t)nrec + 1);
	give(o->ac, v.ac, sp.ac, r.n_ac);
	give(o->gt, v.gt, d.gt, (size_t)nrec * S);
	give(o->block_off, v.block_off, r.block_off, (size_t)nb + 1);
	give(o->seq_off, v.seq_off, sp.sp_off, nsp + 1);
	give(o->at_off, v.at_off, sp.at_off, nsp + 1);
	give(o->seq, v.seq, sp.o_seq, sp.nbytes[0]);
	give(o->at, v.at, sp.o_at, sp.nbytes[1]);
	give_norm(o->raw_pos, v.raw_pos, nw.o_raw_pos, [&](auto &vec) { vec.assign(o->pos.data(), o->pos.data() + nrec); });
	give_norm(o->norm_block, v.norm_block, nw.o_block, all(POVU_HIP_NIL));
	give_norm(o->norm_shift, v.norm_shift, nw.o_shift, all(0u));
	give_norm(o->norm_chop, v.norm_chop, nw.o_chop, all(0u));
	give_norm(o->norm_trim, v.norm_trim, nw.o_trim, all(0u));
	if (in.decomposed) { // (outside the profile: no rows, the arrays NULL)
		const size_t m = (size_t)pr.n_rows;
		give(o->row_record, v.row_record, pr.record, m);
		give(o->row_alt, v.row_alt, pr.alt, m);
		give(o->row_kind, v.row_kind, pr.kind, m);
		give(o->row_reason, v.row_reason, pr.reason, m);
		give(o->row_index, v.row_index, pr.index, m);
		give(o->row_pos, v.row_pos, pr.pos, m);
		give(o->row_ref_start, v.row_ref_start, pr.ref_start, m);
		give(o->row_ref_len, v.row_ref_len, pr.ref_len, m);
		give(o->row_alt_start, v.row_alt_start, pr.alt_start, m);
		give(o->row_alt_len, v.row_alt_len, pr.alt_len, m);
		give(o->row_lead, v.row_lead, pr.lead, m);
		give(o->row_ac, v.row_ac, pr.ac, m);
		give(o->row_an, v.row_an, pr.an, m);
		give(o->row_ns, v.row_ns, pr.ns, m);
	}
	if (in.merge) { // (without the flag: the arrays NULL)
		const size_t g = (size_t)mg.n_mrows;
		give(o->mrow_off, v.mrow_off, mg.off, g + 1);
		give(o->mrow_member, v.mrow_member, mg.member, (size_t)pr.n_rows);
		give(o->mrow_gt, v.mrow_gt, mg.gt, g * S);
		give(o->mrow_ac, v.mrow_ac, mg.ac, g);
		give(o->mrow_an, v.mrow_an, mg.an, g);
		give(o->mrow_ns, v.mrow_ns, mg.ns, g);
	}
	if (in.offref) { // (without the flag: the arrays NULL, the counts 0)
		give(o->rec_offref, v.rec_offref, orf.rows.rec_offref, nrec);
		give(o->host_query, v.host_query, orf.rows.host_query, nrec);
		give(o->host_allele, v.host_allele, orf.rows.host_allele, nrec);
		o->off_contig_path = orf.contig_path, o->off_contig_len = orf.contig_len;
		v.off_contig_path = o->off_contig_path.data(), v.off_contig_len = o->off_contig_len.data();
		v.n_off_contigs = orf.contig_path.size();
		v.offref = 1;
		v.n_offref_sites = w.os.n_sites, v.n_offref_records = orf.rows.n_records, v.n_offref_hosted = orf.rows.n_hosted;
	}
	if (in.untangle) { // (without the flag: the arrays NULL, the counts 0)
		give(o->rec_unt, v.rec_unt, un.rec_unt, nrec);
		give(o->lap, v.lap, un.lap, nrec);
		give(o->n_laps, v.n_laps, un.n_laps, nrec);
		give(o->lap_count, v.lap_count, un.lap_count, (size_t)nrec * S);
		v.untangled = 1;
		v.n_unt_tasks = un.n_tasks, v.n_unt_records = un.n_records, v.n_unt_missing = un.n_missing, v.n_unt_extra = un.n_extra;
		v.n_unt_fallback = un.n_fallback;
	}
	if (in.cluster_ppm) { // (without a threshold: the arrays NULL, the counts 0)
		give(o->rec_clustered, v.rec_clustered, r.rec_clustered, nrec);
		give(o->cl_minsim, v.cl_minsim, r.cl_minsim, nrec);
		give(o->cl_nx, v.cl_nx, sp.cl_nx, r.n_ac + nrec);
		v.cluster_ppm = in.cluster_ppm;
		v.n_cluster_sites = w.cc.n_sites, v.n_clustered_sites = w.n_collapsed, v.n_cluster_vanished = w.n_vanished;
		v.n_cluster_keys = w.cc.n_keys, v.n_cluster_pairs = w.cc.n_pairs, v.n_cluster_pruned = w.cc.n_pruned, v.n_cluster_tier2 = w.cc.n_tier2;
	}
	if (in.spanning) { // (without the flag: the array NULL, the counts 0)
		give(o->rec_star, v.rec_star, r.o_star, nrec);
		v.spanning = 1;
		v.n_star_records = w.nr.n_star_records, v.n_star_entries = w.nr.n_star_entries;
	}
	v.device_ms = timer.stop(ctx->stream);
	for (const auto &fill : defaults)
		fill();
	o->contig_len.resize(nR);
	for (uint32_t k = 0; k < nR; k++)
		o->contig_len[k] = sp.h_roff[k + 1] - sp.h_roff[k];
	v.contig_len = o->contig_len.data();
	v.n_records = nrec;
	v.n_slots = S;
	v.n_blocks = nb;
	v.n_spelled = nsp;
	v.n_seq_bytes = sp.nbytes[0];
	v.n_at_bytes = sp.nbytes[1];
	v.n_refs = nR;
	v.n_inv_records = iv.n, v.n_inv_heads = iv.n_heads, v.n_inv_long = iv.n_long, v.n_inv_tier2 = iv.n_tier2;
	v.nested = in.nested ? 1 : 0;
	v.n_enclosed = w.nr.n_enclosed, v.n_collapsed_sites = in.nested ? w.n_collapsed : 0, v.n_popped = w.nr.n_popped, v.n_rescued = w.nr.n_rescued;
	v.n_normalized = w.nm.n_changed, v.max_shift = w.nm.max_shift, v.n_norm_compared = w.nm.n_compared;
	v.n_rows = pr.n_rows;
	v.n_decomposed_alts = pr.n_decomposed, v.n_passthrough_alts = pr.n_passthrough, v.n_prim_tier2 = pr.n_tier2, v.n_prim_cells = pr.n_cells;
	v.merged = in.merge ? 1 : 0;
	v.n_mrows = mg.n_mrows;
	v.n_merged_groups = mg.n_groups, v.n_merged_members = mg.n_members, v.n_merge_splits = mg.n_splits;
	v.n_ref_consistent = mg.n_ref_consistent, v.n_gt_conflicts = mg.n_conflicts;
	v.n_regions = w.rg.n_regions, v.n_region_sites = w.rg.n_sites, v.n_region_masked = w.rg.n_masked, v.n_region_dropped = w.rg.n_dropped;
	CallsOwner *raw = o.release();
	return &raw->view;
}

// a call, with whatever of a profile, regions and a cluster threshold its entry point takes (NULL: none)
povu_hip_calls *call(povu_hip_ctx *ctx, const povu_hip_sites *sites, const povu_hip_call_refs *refs, const uint32_t *slot_of_path,
		     const povu_hip_trav_opts *opts, const povu_hip_call_profile_opts *profile, const povu_hip_call_regions *regions,
		     const povu_hip_call_cluster_opts *cluster, char *err, size_t errlen)
{
	CallTimer timer;
	return guarded_call(ctx, err, errlen, (povu_hip_calls *)nullptr, [&] {
		const CallInputs in = check_call_inputs(ctx, sites, refs, slot_of_path, opts, profile, regions, cluster);
		// region calls: masking is allowed when the call is not nested (a nested call computes its classes over every site)
		const RegionIn rin = region_prepare(ctx, regions, !in.nested);
		RegionDevice rg;
		const TravDevice d = trav_pipeline(
			ctx,
			[&](CallTimer &tm, const QueryLayout &more) {
				if (!rin.active)
					return query_front(ctx, in.qa, in.qz, in.qor, ctx->tr_ws, tm, more);
				RegionWs rw; // next to the queries, in the front end's arena
				const QueryFront q = query_front(ctx, in.qa, in.qz, in.qor, ctx->tr_ws, tm, [&](Spans &take, uint32_t n) {
					more(take, n);
					region_spans(ctx, rin, n, rw, take);
				});
				rg = region_sites(ctx, rin, q, rw);
				return q;
			},
			opts, timer);
		CallWs w;
		w.rg = rg;
		reference_offsets(ctx, in, d, w);
		callability(ctx, in, d, w);
		if (in.offref) {
			offref_sites_step(ctx, in, d, w);
			surrogate_offsets(ctx, in, w);
		}
		site_classes(ctx, in, d, w);
		kept_sites(ctx, in, d, w);
		slot_table(ctx, in, d, w);
		flubble_records(ctx, in, d, w);
		if (in.offref)
			w.oh = offref_hosts(ctx, d, w.v, w.os);
		CallInv inv;
		CallRecs r;
		r.nrec = inversion_rows(ctx, in, w, inv);
		record_arrays(ctx, in, w, inv, r);
		CallSpelled sp;
		spelling(ctx, in, w, inv, r, sp);
		CallOffref orf;
		if (in.offref)
			offref_rows_step(ctx, in, w, inv, r, orf);
		const UntangleRows un = in.untangle ? untangle_step(ctx, in, w, inv, r, sp) : UntangleRows{};
		const PrimIn pin = in.decomposed ? primitive_input(in, w, r, sp) : PrimIn{};
		const PrimRows pr = in.decomposed ? prim_rows(ctx, pin) : PrimRows{};
		const MergedRows mg = in.merge ? merge_rows(ctx, pin, pr) : MergedRows{};
		return calls_to_host(ctx, in, w, inv, r, sp, pr, mg, orf, un, timer);
	});
}
} // namespace

extern "C" povu_hip_calls *povu_hip_call(povu_hip_ctx *ctx, const povu_hip_sites *sites, const povu_hip_call_refs *refs,
					 const uint32_t *slot_of_path, const povu_hip_trav_opts *opts, char *err, size_t errlen)
{
	return call(ctx, sites, refs, slot_of_path, opts, nullptr, nullptr, nullptr, err, errlen);
}

extern "C" povu_hip_calls *povu_hip_call_profile(povu_hip_ctx *ctx, const povu_hip_sites *sites, const povu_hip_call_refs *refs,
						 const uint32_t *slot_of_path, const povu_hip_trav_opts *opts,
						 const povu_hip_call_profile_opts *profile, char *err, size_t errlen)
{
	return call(ctx, sites, refs, slot_of_path, opts, profile, nullptr, nullptr, err, errlen);
}

extern "C" povu_hip_calls *povu_hip_call_restricted(povu_hip_ctx *ctx, const povu_hip_sites *sites, const povu_hip_call_refs *refs,
						    const uint32_t *slot_of_path, const povu_hip_trav_opts *opts,
						    const povu_hip_call_profile_opts *profile, const povu_hip_call_regions *regions, char *err,
						    size_t errlen)
{
	return call(ctx, sites, refs, slot_of_path, opts, profile, regions, nullptr, err, errlen);
}

extern "C" povu_hip_calls *povu_hip_call_clustered(povu_hip_ctx *ctx, const povu_hip_sites *sites, const povu_hip_call_refs *refs,
						   const uint32_t *slot_of_path, const povu_hip_trav_opts *opts,
						   const povu_hip_call_profile_opts *profile, const povu_hip_call_regions *regions,
						   const povu_hip_call_cluster_opts *cluster, char *err, size_t errlen)
{
	return call(ctx, sites, refs, slot_of_path, opts, profile, regions, cluster, err, errlen);
}

extern "C" void povu_hip_calls_free(povu_hip_calls *c)
{
	delete reinterpret_cast<CallsOwner *>(c);
}
