// call_common.hpp -- what the flubble calls (call_kernels.hip) and the inversion calls (inv_kernels.hip) share beyond
// query_common.hpp: nucleotide complements, decimal widths, the bases and AT strings of a step sequence (one wave each), and
// the inversion pipeline's interface to povu_hip_call.
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

// ---- the inversion calls of povu_hip_call (inv_kernels.hip; INTEGRATION.md "Inversion calls")
// what povu_hip_call has on the device when it asks for them
struct InvIn {
	uint64_t NR = 0;		  // reference steps, the reference paths concatenated ("reference index")
	uint32_t nR = 0, S = 0, NS = 0;
	const uint64_t *ref_base = nullptr; // [nR + 1] reference index of every reference path's first step
	const uint32_t *ref_path = nullptr, *slot_of_path = nullptr, *slot_first = nullptr;
	const uint64_t *roff = nullptr; // [NR + 1] bases in front of every reference step (one scan over the concatenation)
	uint32_t max_steps = 65536;
	bool force_tier2 = false;
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
// rows of the merged list: f_dst[i] for flubble record i (sorted; its reference number f_ref[i] and POS f_pos[i]), v.dst
void inv_merge(povu_hip_ctx *ctx, InvDevice &v, uint32_t nrec, const uint32_t *f_ref, const uint64_t *f_pos, uint32_t *f_dst);
// the per-record fields of the inversion records (AC count 1 into nalt)
void inv_fields(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, const InvRows &o);
// their blocks (nb + record, two spelled alleles each: bcnt) and GT rows
void inv_genotypes(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, const InvRows &o, uint32_t nb, uint64_t *bcnt);
// their AC, AN, NS and flags
void inv_counts(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, const InvRows &o, const uint64_t *ac_off, uint32_t *ac);
// lengths of the bases and AT strings of their spelled alleles, slen[2 b + alt] (alt 0 REF, 1 ALT)
void inv_spell_len(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, uint64_t *slen, uint64_t *alen);
void inv_emit(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, const uint64_t *s_off, const uint64_t *a_off, char *o_seq, char *o_at,
	      unsigned long long *bad);

} // namespace povu_hip
