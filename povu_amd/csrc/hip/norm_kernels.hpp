// norm_kernels.hpp -- left-normalisation of the flubble records of povu_hip_call under POVU_HIP_PROFILE_LEFT_NORMALIZED
// (INTEGRATION.md "Left-normalised calls"; norm_kernels.hip): what call_kernels.hip hands over and what it gets back.
#pragma once
#include "call_common.hpp"

namespace povu_hip
{

// the flubble records before the sort (record j is traversal rlist[j]), the alleles they write and the reference paths
struct NormIn {
	uint32_t nfl = 0;
	const uint32_t *rlist = nullptr, *rq = nullptr, *op = nullptr, *rlen = nullptr;
	const uint32_t *aoff = nullptr, *oa = nullptr, *afirst = nullptr; // (the classes of a nested call)
	const uint8_t *orv = nullptr;
	const uint64_t *rpos = nullptr, *ilen = nullptr, *xilen = nullptr;
	uint8_t *rstate = nullptr; // RS_NORMALIZED is set in a changed record's
	uint64_t *pos = nullptr;   // raw POS in, normalised POS out
	uint32_t nR = 0;
	const uint32_t *ref_of_path = nullptr, *ref_path = nullptr;
	const uint64_t *ref_base = nullptr, *roff = nullptr;
};
// per record j (the context's normalisation arena, valid until the next call under the profile): raw POS, chop r, shift s,
// trim u (all 0 for an unchanged record); the counters
struct NormRecs {
	uint64_t *raw_pos = nullptr, *chop = nullptr, *shift = nullptr, *trim = nullptr;
	uint64_t n_changed = 0, max_shift = 0, n_compared = 0;
};
NormRecs norm_records(povu_hip_ctx *ctx, const NormIn &in);

// the rows of the sorted records (row dst[i], or i, of record perm[i]) and the blocks of the changed ones: block nb0 + k
// for the k-th changed record in sorted order, one spelled allele per written allele (REF first); gives their number
struct NormRows {
	uint64_t *o_raw_pos;
	uint32_t *o_block, *o_shift, *o_chop, *o_trim;
	uint32_t *need, *off, *list; // [nrec + 1] changed, its exclusive sums, the changed records in sorted order
};
void norm_row_fields(povu_hip_ctx *ctx, const NormIn &in, const NormRecs &n, uint32_t nrec, const uint32_t *perm, const uint32_t *dst,
		     const NormRows &o);
void norm_blocks(povu_hip_ctx *ctx, const NormIn &in, uint32_t nrec, const uint32_t *perm, const uint32_t *dst, const NormRows &o, uint32_t nb0,
		 uint64_t *bcnt);
// lengths of the nsp spelled alleles of the nn blocks from block_off[0] on (slen; their AT strings are empty), and their bases
void norm_spell_len(povu_hip_ctx *ctx, const NormIn &in, const NormRecs &n, const NormRows &o, uint32_t nn, const uint64_t *block_off, uint64_t nsp,
		    uint64_t *slen, uint64_t *alen);
void norm_emit(povu_hip_ctx *ctx, const NormIn &in, const NormRecs &n, const NormRows &o, uint32_t nn, const uint64_t *block_off, uint64_t nsp,
	       const uint64_t *s_off, char *o_seq, unsigned long long *bad);

} // namespace povu_hip
