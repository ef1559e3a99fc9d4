// vcfhap_edits.hpp -- a parsed VCF's (record, ALT) items as edits on the device: what the haplotype comparison
// (vcfhap_kernels.hip) and the consensus haplotypes (vcfcons_kernels.hip) do alike before they differ.  The reference as a view
// over the CHROM paths, the placing kernel (a lane per record: placed or not, its span [POS, POS + |REF|)), the edit arrays
// and their writers, EditPolicy -- the policy of the two tiers of vcf_pair.hpp that settles the items of unplaced records
// first, trims to vh_trim_limit, hashes T and writes an edit or none --, and SameEdit, the exact comparison behind the edit
// groups of exact_groups.hpp.  Coordinates carry one more than the 0-based value (vcfhap_rules.hpp).
#pragma once
#include "call_common.hpp"
#include "exact_groups.hpp"
#include "vcf_pair.hpp"
#include "vcfhap_rules.hpp"

namespace povu_hip
{

constexpr uint64_t POS_LIMIT = 1ull << 40;
enum { CN_PLACED_A = 0, CN_PLACED_B, CN_CAPPED, CN_BAD_WINDOWS, CN_TASKS, CN_WORDS = 8 };
enum { KIND_REF = 0, KIND_UNSPELLED = 1, KIND_EDIT = 2 };

// the reference: CHROM id -> reference number (NO_QUERY: no path of that name), the view over those paths
struct VhRef {
	uint32_t on;
	const uint32_t *chrom_ref;
	RefView R;
	PathsView P;
	__device__ __forceinline__ uint64_t path_len(uint32_t c) const { return R.roff[R.ref_base[c + 1]] - R.roff[R.ref_base[c]]; }
	// folded base ci of reference c (ci below its length)
	__device__ __forceinline__ uint8_t base(uint32_t c, uint64_t ci) const
	{
		uint32_t seg;
		return vm_fold((char)ref_path_base(P, R.roff, ref_path_slice(R, P, c), ci, &seg));
	}
};
// what the edit kernels write per item
struct VhEdits {
	uint8_t *state, *keep; // (keep: 1 for an item with an edit, which the group numbering counts)
	uint64_t *bs, *be, *t_at; // [s, e) with one added; where T begins in the uploaded text
	uint32_t *t_len, *suffix, *prefix;
	uint32_t *rq, *rlen; // the grouping's query (CHROM id; n_chroms for an item without an edit) and length
	uint64_t *rhash;
	uint64_t mask;
	uint32_t n_chroms;
	const uint8_t *placed;
};

[[maybe_unused]] static __global__ __launch_bounds__(Q_TPB) void k_vh_place(PairView A, VhRef F, uint8_t *__restrict__ placed, uint64_t *__restrict__ sp_lo,
						     uint64_t *__restrict__ sp_hi, unsigned long long *__restrict__ cnt)
{
	const uint32_t lane = threadIdx.x & 63u;
	unsigned long long na = 0, nb = 0;
	for (uint64_t b = ((uint64_t)blockIdx.x * Q_TPB + threadIdx.x) & ~63ull; b < A.nR; b += (uint64_t)gridDim.x * Q_TPB) {
		const uint64_t r = b + lane;
		bool ok = false;
		if (r < A.nR) {
			const uint64_t nr = A.ref_len((uint32_t)r), pos = A.pos[r];
			ok = nr && !(nr == 1 && A.text[A.toff[A.aoff[r]]] == '.');
			if (ok && F.on) {
				const uint32_t c = F.chrom_ref[A.chrom[r]];
				ok = c != NO_QUERY && pos >= 1 && pos - 1 + nr <= F.path_len(c);
			}
			placed[r] = ok;
			sp_lo[r] = pos, sp_hi[r] = pos + nr;
		}
		na += __popcll(__ballot(ok && r < A.nRa));
		nb += __popcll(__ballot(ok && r >= A.nRa));
	}
	if (lane == 0 && na)
		atomicAdd(cnt + CN_PLACED_A, na);
	if (lane == 0 && nb)
		atomicAdd(cnt + CN_PLACED_B, nb);
}

__device__ __forceinline__ void write_none(const VhEdits &O, uint32_t i, uint8_t state)
{
	O.state[i] = state, O.keep[i] = 0;
	O.bs[i] = 0, O.be[i] = 0, O.t_at[i] = 0, O.t_len[i] = 0, O.suffix[i] = 0, O.prefix[i] = 0;
	O.rq[i] = O.n_chroms, O.rlen[i] = 0, O.rhash[i] = vm_mix64(i) & O.mask; // (equal to no item: SameEdit)
}
__device__ __forceinline__ void write_edit(const VhEdits &O, const PairView &A, uint32_t i, const PairView::Texts &T, uint64_t s, uint64_t p, uint64_t t_hash)
{
	const uint32_t r = A.record_of(i);
	const VhEdit e = vh_edit(A.pos[r], T.nr, T.na, s, p);
	O.state[i] = POVU_HIP_H_EDIT, O.keep[i] = 1;
	O.bs[i] = e.bs, O.be[i] = e.be, O.t_at[i] = (uint64_t)(T.alt - A.text) + e.t_at, O.t_len[i] = (uint32_t)e.t_len;
	O.suffix[i] = (uint32_t)s, O.prefix[i] = (uint32_t)p;
	O.rq[i] = A.chrom[r], O.rlen[i] = (uint32_t)e.t_len, O.rhash[i] = vh_edit_hash(e.bs, e.be, e.t_len, t_hash) & O.mask;
}

// the edits as a policy of the two tiers (vcf_pair.hpp): the items of an unplaced record are settled before their texts
struct EditPolicy {
	VhEdits O;
	static constexpr bool HASH_REF = false;
	static __device__ __forceinline__ uint64_t trim_limit(uint64_t nr, uint64_t na) { return vh_trim_limit(nr, na); }
	__device__ __forceinline__ bool refused(const PairView &A, uint32_t i) const { return !O.placed[A.record_of(i)]; }
	__device__ __forceinline__ void on_refused(uint32_t i) const { write_none(O, i, POVU_HIP_H_UNPLACED); }
	__device__ __forceinline__ void on_skipped(uint32_t i) const { write_none(O, i, POVU_HIP_H_UNSPELLED); }
	__device__ __forceinline__ void on_trimmed(const PairView &A, uint32_t i, const PairView::Texts &T, uint64_t s, uint64_t p, uint64_t, uint64_t t_hash) const
	{
		write_edit(O, A, i, T, s, p, t_hash);
	}
};

// items a and b of one CHROM have the same edit
struct SameEdit {
	const char *text;
	const uint8_t *state;
	const uint64_t *bs, *be, *t_at;
	const uint32_t *t_len;
	__device__ __forceinline__ bool operator()(uint32_t a, uint32_t b) const
	{
		if (state[a] != POVU_HIP_H_EDIT || state[b] != POVU_HIP_H_EDIT || bs[a] != bs[b] || be[a] != be[b] || t_len[a] != t_len[b])
			return false;
		const char *ta = text + t_at[a], *tb = text + t_at[b];
		for (uint32_t i = 0, n = t_len[a]; i < n; i++)
			if (vm_fold(ta[i]) != vm_fold(tb[i]))
				return false;
		return true;
	}
};

} // namespace povu_hip
