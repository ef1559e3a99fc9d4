// norm_kernels.hpp -- left-normalisation of the flubble records of povu_hip_call under POVU_HIP_PROFILE_LEFT_NORMALIZED
// (INTEGRATION.md "Left-normalised calls"; norm_kernels.hip): what call_kernels.hip hands over and what it gets back.
#pragma once
#include "call_common.hpp"

namespace povu_hip
{

// per record j (the context's normalisation arena, valid until the next call under the profile): raw POS, chop r, shift s,
// trim u (all 0 for an unchanged record); the counters
struct NormRecs {
	uint64_t *raw_pos = nullptr, *chop = nullptr, *shift = nullptr, *trim = nullptr;
	uint64_t n_changed = 0, max_shift = 0, n_compared = 0;
};
// reads the call's view (v.raw_pos: the raw POS, still in `pos`); sets RS_NORMALIZED in the rstate of a changed record and moves
// its `pos`.  The caller then points v.raw_pos at the raw POS kept here
NormRecs norm_records(povu_hip_ctx *ctx, const CallView &v, uint8_t *rstate, uint64_t *pos);

// the rows of the sorted records (row dst[i], or i, of record perm[i]) and the blocks of the changed ones: block first_block + k
// for the k-th changed record in sorted order, one spelled allele per written allele (REF first); gives their number
struct NormRows {
	uint64_t *o_raw_pos;
	uint32_t *o_block, *o_shift, *o_chop, *o_trim;
	uint32_t *need, *off, *list; // [nrec + 1] changed, its exclusive sums, the changed records in sorted order
};
void norm_row_fields(povu_hip_ctx *ctx, const CallView &v, const NormRecs &n, uint32_t nrec, const uint32_t *perm, const uint32_t *dst, const NormRows &o);
void norm_blocks(povu_hip_ctx *ctx, const CallView &v, uint32_t nrec, const uint32_t *perm, const uint32_t *dst, const NormRows &o, uint32_t first_block,
		 uint64_t *bcnt);
// lengths of the spelled alleles of the layout's normalised family (slen; their AT strings are empty), and their bases;
// block_off, slen, alen and s_off are the whole arrays
void norm_spell_len(povu_hip_ctx *ctx, const CallView &v, const NormRecs &n, const NormRows &o, const BlockLayout &L, const uint64_t *block_off,
		    uint64_t *slen, uint64_t *alen);
void norm_emit(povu_hip_ctx *ctx, const CallView &v, const NormRecs &n, const NormRows &o, const BlockLayout &L, const uint64_t *block_off,
	       const uint64_t *s_off, char *o_seq, unsigned long long *bad);

} // namespace povu_hip
