// call_common.hpp -- what the flubble calls (call_kernels.hip) and the inversion calls (inv_kernels.hip) share beyond
// query_common.hpp: nucleotide complements, decimal widths, the bases and AT strings of a step sequence (one wave each), the
// device views of a call, an allele as a record writes it, the layout of the blocks of spelled alleles, and the inversion
// pipeline's interface to povu_hip_call.
#pragma once
#include "query_common.hpp"

namespace povu_hip
{

// what differs per flubble record before the sort (call_kernels.hip "rstate"): anchored, REF without an inner base, REF spelled
// on its own, changed by the left-normalisation (norm_kernels.hip)
static constexpr uint8_t RS_ANCHORED = 1, RS_REF_EMPTY = 2, RS_OWN_REF = 4, RS_NORMALIZED = 8;

// complement of a nucleotide code (ACGTN, lower case, IUPAC), 0 for any other byte
__device__ __forceinline__ uint8_t comp(uint8_t c)
{
	const bool lower = c >= 'a' && c <= 'z';
	uint8_t u = lower ? (uint8_t)(c - 32) : c, r;
	switch (u) {
	case 'A': r = 'T'; break;
	case 'C': r = 'G'; break;
	case 'G': r = 'C'; break;
	case 'T': r = 'A'; break;
	case 'N': r = 'N'; break;
	case 'R': r = 'Y'; break;
	case 'Y': r = 'R'; break;
	case 'K': r = 'M'; break;
	case 'M': r = 'K'; break;
	case 'S': r = 'S'; break;
	case 'W': r = 'W'; break;
	case 'B': r = 'V'; break;
	case 'V': r = 'B'; break;
	case 'D': r = 'H'; break;
	case 'H': r = 'D'; break;
	default: return 0;
	}
	return lower ? (uint8_t)(r + 32) : r;
}

__device__ __forceinline__ uint32_t ndig(uint32_t x)
{
	uint32_t d = 1;
	while (x >= 10) {
		x /= 10;
		d++;
	}
	return d;
}

// ---- the text of a step sequence, one wave: `step(k)` is step k of m
// '>id' or '<id' of step x at o_at[at .. at + width)
__device__ __forceinline__ void put_step(char *__restrict__ o_at, const uint32_t *__restrict__ vid, uint32_t x, uint64_t at, uint32_t width)
{
	uint32_t id = vid[x >> 1];
	o_at[at] = (x & 1u) ? '<' : '>';
	for (uint32_t d = width - 1; d >= 1; d--) {
		o_at[at + d] = (char)('0' + id % 10);
		id /= 10;
	}
}
// the bases from o_seq[w] on (reverse-complemented on '<' steps, lanes across a segment's bytes; a byte that is no nucleotide
// code leaves its segment in *bad) and the AT string from o_at[wa] on (lanes across steps, a wave prefix sum of the widths)
template <class StepFn>
__device__ __forceinline__ void emit_steps(uint32_t lane, uint32_t m, StepFn step, const uint64_t *__restrict__ seq_off,
					   const char *__restrict__ seq, const uint32_t *__restrict__ vid, uint64_t w, uint64_t wa,
					   char *__restrict__ o_seq, char *__restrict__ o_at, unsigned long long *__restrict__ bad)
{
	for (uint32_t k = 0; k < m; k++) {
		const uint32_t x = step(k), v = x >> 1;
		const uint64_t b0 = seq_off[v], n = seq_off[v + 1] - b0;
		for (uint64_t i = lane; i < n; i += 64) {
			const uint8_t c = (uint8_t)seq[(x & 1u) ? b0 + n - 1 - i : b0 + i], r = comp(c);
			if (!r)
				atomicMin(bad, (unsigned long long)v);
			o_seq[w + i] = (char)((x & 1u) ? r : c);
		}
		w += n;
	}
	for (uint32_t k0 = 0; k0 < m; k0 += 64) {
		const uint32_t k = k0 + lane;
		const uint32_t x = k < m ? step(k) : 0;
		const uint32_t width = k < m ? 1 + ndig(vid[x >> 1]) : 0;
		const uint32_t incl = wave_inclusive_sum(width);
		if (k < m)
			put_step(o_at, vid, x, wa + incl - width, width);
		wa += __shfl(incl, 63, 64);
	}
}

// ---- the device views of a call: built once on the host (call_kernels.hip), passed to the kernels by value
// the arrays of the traversal pipeline the call reads (TravDevice; oa and aoff are the exact alleles)
struct TravView {
	uint32_t R;
	const uint32_t *rq, *op, *of, *oa, *aoff, *rlen, *qstatus;
	const uint8_t *orv;
	const uint64_t *rpos;
};
static inline TravView trav_view(const TravDevice &d) { return TravView{d.R, d.rq, d.op, d.of, d.oa, d.aoff, d.rlen, d.qstatus, d.orv, d.rpos}; }
// the reference paths: NR reference steps, the nR reference paths concatenated ("reference index")
struct RefView {
	uint64_t NR;
	uint32_t nR;
	const uint32_t *ref_of_path, *ref_path; // [P] reference number of a path (NO_QUERY: none), [nR] path of a reference
	const uint64_t *ref_base;		 // [nR + 1] reference index of every reference path's first step
	const uint64_t *roff;			 // [NR + 1] bases in front of every reference step (one scan over the concatenation)
};
// len[i] of every step of the view's concatenated paths: the bases of its segment (call_kernels.hip).  One exclusive u64 scan
// of it gives roff; the references, the surrogates and the region paths all get their offsets so
void launch_ref_len(const RefView &R, const PathsView &P, uint64_t *len, hipStream_t s);
// the genotype slots
struct SlotsView {
	uint32_t S, NS;
	const uint32_t *slot_of_path, *slot_first; // [P], [NS + 1]
};
// what the call's kernels read: the views above and the call's own tables.  What a kernel writes is a parameter of its own
struct CallView {
	PathsView paths;
	TravView trav;
	RefView ref;
	// the alleles the call reads, per site q [aoff[q], aoff[q + 1]): the exact alleles, or with POVU_HIP_T_NESTED the classes
	// (crep: the exact allele that represents a class, else null).  oa: allele of a traversal within its site, afirst: an
	// allele's first traversal, ilen / atl: its inner bases and AT width
	const uint32_t *aoff, *oa, *afirst, *crep;
	const uint64_t *ilen, *atl;
	// per site: kept, alleles without an inner base, PVST height
	const uint32_t *keep, *zc, *height;
	// per flubble record j before the sort (traversal rlist[j]): RS_*, the inner bases and AT width of its own REF, the written
	// lengths of REF and of its longest allele, POS as the graph gives it (read-only once set) and POS as written (the sort
	// key; the left-normalisation moves it)
	uint32_t nfl;
	const uint32_t *rlist;
	const uint8_t *rstate;
	const uint64_t *xilen, *xatl, *ref_len, *max_len, *raw_pos, *pos;
	// which traversals of a kept site are records: those by the reference paths (on_ref: [P] reference number of a path,
	// NO_QUERY: none), or with POVU_HIP_T_OFFREF for a site called off-reference those by its surrogate (sur: [n] that path,
	// NO_QUERY for a site the references call; null without the flag).  `ref` then holds the references and the surrogates
	const uint32_t *on_ref, *sur;
};
// traversal t of a kept site q by path p is a record
__device__ __forceinline__ bool is_record_path(const CallView &V, uint32_t q, uint32_t p)
{
	if (V.sur && V.sur[q] != NO_QUERY)
		return p == V.sur[q];
	return V.on_ref[p] != NO_QUERY;
}

// ---- a base of a step and of a reference path
__device__ __forceinline__ uint64_t path_step_len(const PathsView &P, uint32_t x) { return P.seq_off[(x >> 1) + 1] - P.seq_off[x >> 1]; }
// base `within` of step x as the step spells it (0 for a byte that is no nucleotide code on a '<' step)
__device__ __forceinline__ uint8_t path_step_base(const PathsView &P, uint32_t x, uint64_t within)
{
	const uint64_t b0 = P.seq_off[x >> 1], n = P.seq_off[(x >> 1) + 1] - b0;
	const uint8_t c = (uint8_t)P.seq[(x & 1u) ? b0 + n - 1 - within : b0 + within];
	return (x & 1u) ? comp(c) : c;
}
// reference path r: its slice of roff (n steps from reference index b) and its first path word
struct RefPathSlice {
	uint64_t b, n, gs;
};
__device__ __forceinline__ RefPathSlice ref_path_slice(const RefView &R, const PathsView &P, uint32_t r)
{
	return {R.ref_base[r], R.ref_base[r + 1] - R.ref_base[r], P.path_off[R.ref_path[r]]};
}
// base ci (0-based) of the reference path as the path spells it; *seg its segment.  ci is below the path's length
__device__ __forceinline__ uint8_t ref_path_base(const PathsView &P, const uint64_t *__restrict__ roff, const RefPathSlice &R, uint64_t ci, uint32_t *seg)
{
	const uint64_t *__restrict__ off = roff + R.b;
	const uint64_t target = off[0] + ci;
	// the first step that ends behind the base (steps of no base are passed over)
	const uint64_t lo = first_not(uint64_t(0), R.n - 1, [=](uint64_t k) { return off[k + 1] <= target; });
	const uint32_t x = P.steps[R.gs + lo];
	*seg = x >> 1;
	return path_step_base(P, x, target - off[lo]);
}

// inner bases and AT width of a traversal: its steps but the first and the last
struct InnerSize {
	uint64_t bases, at;
};
__device__ __forceinline__ InnerSize span_inner_size(const TravSpan &sp, const PathsView &P)
{
	InnerSize n{0, 0};
	for (uint32_t k = 1; k + 1 < sp.len; k++) {
		const uint32_t v = sp.step(P.steps, k) >> 1;
		n.bases += P.seq_off[v + 1] - P.seq_off[v];
		n.at += 1 + ndig(P.vid[v]);
	}
	return n;
}

// ---- an allele as a record writes it, in the reference's direction
struct WrittenAllele {
	TravSpan span;
	bool o;		   // the reference runs Z -> S through the site
	uint32_t anchor;   // the boundary step the reference enters by
	bool anchored;	   // the text and the AT string begin with the anchor (RS_ANCHORED) ...
	bool anchor_base;  // ... and its segment is not empty: the text begins with its last base,
	uint64_t anchor_at; // which is this byte of the sequences (complemented when the anchor is a '<' step)
	uint64_t ilen, atl; // inner bases, AT width of the inner steps
	__device__ __forceinline__ uint32_t inner_steps() const { return span.len - 2; }
	__device__ __forceinline__ uint32_t inner_step(const uint32_t *__restrict__ steps, uint32_t k) const
	{
		return o ? span.step(steps, span.len - 2 - k) ^ 1u : span.step(steps, k + 1);
	}
	__device__ __forceinline__ uint64_t text_len() const { return ilen + (anchor_base ? 1 : 0); }
	__device__ __forceinline__ uint64_t at_len(const PathsView &P) const { return atl + (anchored ? 1 + ndig(P.vid[anchor >> 1]) : 0); }
};
// traversal t written with orientation o
__device__ __forceinline__ WrittenAllele written_allele(const CallView &V, uint32_t t, bool o, bool anchored, uint64_t ilen, uint64_t atl)
{
	WrittenAllele s;
	s.span = trav_span(V.trav.rpos, V.trav.rlen, t);
	s.o = o;
	s.anchor = o ? s.span.step(V.paths.steps, s.span.len - 1) ^ 1u : s.span.step(V.paths.steps, 0);
	s.anchored = anchored;
	s.anchor_base = false;
	s.anchor_at = 0;
	if (anchored) {
		const uint64_t b0 = V.paths.seq_off[s.anchor >> 1], b1 = V.paths.seq_off[(s.anchor >> 1) + 1];
		s.anchor_base = b1 > b0;
		s.anchor_at = (s.anchor & 1u) ? b0 : b1 - 1;
	}
	s.ilen = ilen;
	s.atl = atl;
	return s;
}
// the three ways a spelled allele is found.  Allele `index` of a class block (site << 2 | anchored << 1 | orientation: the
// block's own bit)
__device__ __forceinline__ WrittenAllele allele_of_block(const CallView &V, uint32_t block, uint32_t index)
{
	const uint32_t a = V.aoff[block >> 2] + index;
	return written_allele(V, V.afirst[a], block & 1u, (block & 2u) != 0, V.ilen[a], V.atl[a]);
}
// the own REF of record j (an extra block): its traversal, oriented as the traversal is
__device__ __forceinline__ WrittenAllele own_ref_of_record(const CallView &V, uint32_t j)
{
	const uint32_t t = V.rlist[j];
	return written_allele(V, t, V.trav.orv[t] != 0, (V.rstate[j] & RS_ANCHORED) != 0, V.xilen[j], V.xatl[j]);
}
// written allele i of record j: 0 its REF, then the other alleles of its site in order, all oriented as the record's traversal
__device__ __forceinline__ uint32_t other_allele(const CallView &V, uint32_t j, uint32_t i)
{
	const uint32_t t = V.rlist[j], ra = V.oa[t];
	return V.aoff[V.trav.rq[t]] + (i - 1 < ra ? i - 1 : i);
}
__device__ __forceinline__ WrittenAllele allele_of_record(const CallView &V, uint32_t j, uint32_t i)
{
	if (!i)
		return own_ref_of_record(V, j);
	const uint32_t a = other_allele(V, j, i);
	return written_allele(V, V.afirst[a], V.trav.orv[V.rlist[j]] != 0, (V.rstate[j] & RS_ANCHORED) != 0, V.ilen[a], V.atl[a]);
}

// ---- the blocks of spelled alleles.  Four families, in this order: the class blocks [0, nfc), one per (site, anchored,
// orientation) some record needs, an allele each of the site; the extra blocks [nfc, nfb), the one own REF of a nested record
// that is not its class's representative; the inversion blocks [nfb, nb0), REF and ALT of an inversion record; the
// normalised blocks [nb0, nb), the written alleles of a record the left-normalisation changed.  block_off, slen, alen,
// sp_off and at_off run over all of them: the class and the extra blocks hold the spelled alleles [0, nfsp) (one launch
// spells both), the inversion blocks [nfsp, nsp0), the normalised blocks [nsp0, nsp).
struct BlockLayout {
	uint32_t nfc = 0, nfb = 0, nb0 = 0, nb = 0;
	uint64_t nfsp = 0, nsp0 = 0, nsp = 0;
	struct Family {
		uint32_t b0, nb; // first block, blocks
		uint64_t s0, ns; // first spelled allele, spelled alleles
	};
	__host__ __device__ Family flubble() const { return {0, nfb, 0, nfsp}; } // class and extra blocks
	__host__ __device__ Family inversion() const { return {nfb, nb0 - nfb, nfsp, nsp0 - nfsp}; }
	__host__ __device__ Family normalised() const { return {nb0, nb - nb0, nsp0, nsp - nsp0}; }
	__host__ __device__ bool is_class(uint32_t b) const { return b < nfc; }
	__host__ __device__ uint32_t extra_block(uint32_t x) const { return nfc + x; } // of the x-th own REF
};

// ---- the inversion calls of povu_hip_call (inv_kernels.hip; INTEGRATION.md "Inversion calls")
// what povu_hip_call has on the device when it asks for them
struct InvIn {
	PathsView paths;
	RefView ref;
	SlotsView slots;
	uint32_t max_steps = 65536;
	bool force_tier2 = false;
	const uint32_t *marked = nullptr; // region calls: bit v set for a marked segment; a run whose two end steps miss it is no record
};
// the records found, on the device (the context's inversion arenas, valid until the next call with inversions): per record, in
// (reference, first, steps) order, its reference number, reference index, steps and POS; per reported run, in (record, slot)
// order, its record and its path's slot
struct InvDevice {
	uint32_t n = 0, n_runs = 0;
	uint64_t n_heads = 0, n_long = 0, n_tier2 = 0;
	uint32_t *ref = nullptr, *at = nullptr, *steps = nullptr, *run_rec = nullptr, *run_slot = nullptr;
	uint64_t *pos = nullptr;
	uint32_t *dst = nullptr; // [n] row of every record in the merged record list (inv_merge)
	// the step index: the global positions occ[ioff[x] .. ioff[x + 1]) hold path word x, ascending
	const uint32_t *ioff = nullptr, *occ = nullptr;
};
// where the flubble records go in one list with the inversion records
struct InvRows {
	uint32_t *o_q, *o_path, *o_first, *o_ref, *o_nal, *o_an, *o_ns, *o_block, *o_nsteps;
	uint64_t *o_pos, *nalt;
	uint8_t *o_flags;
	uint16_t *gt;
};
InvDevice inv_find(povu_hip_ctx *ctx, const InvIn &in);
// The step index alone, for the inversion calls and the VCF checks (vcfcheck_kernels.hip): the occurrences of every path word,
// carved from `A` (from its offset 0) in front of the caller's own spans (`more`) and built on the context's stream.  The
// caller has refused 2^32 - 4096 path steps or more; at least one step is resident
struct StepIndex {
	const uint32_t *ioff, *occ;
};
StepIndex build_step_index(povu_hip_ctx *ctx, Arena &A, const std::function<void(Spans &)> &more);
// rows of the merged list: f_dst[i] for flubble record i (sorted; its reference number f_ref[i] and POS f_pos[i]), v.dst
void inv_merge(povu_hip_ctx *ctx, InvDevice &v, uint32_t nrec, const uint32_t *f_ref, const uint64_t *f_pos, uint32_t *f_dst);
// the per-record fields of the inversion records (AC count 1 into nalt)
void inv_fields(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, const InvRows &o);
// their blocks (the layout's inversion family, two spelled alleles each: bcnt) and GT rows
void inv_genotypes(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, const InvRows &o, uint32_t first_block, uint64_t *bcnt);
// their AC, AN, NS and flags
void inv_counts(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, const InvRows &o, const uint64_t *ac_off, uint32_t *ac);
// lengths of the bases and AT strings of their spelled alleles (REF, then ALT), and the strings; slen, alen, s_off and a_off
// are the whole arrays
void inv_spell_len(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, const BlockLayout &L, uint64_t *slen, uint64_t *alen);
void inv_emit(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, const BlockLayout &L, const uint64_t *s_off, const uint64_t *a_off, char *o_seq,
	      char *o_at, unsigned long long *bad);

} // namespace povu_hip
