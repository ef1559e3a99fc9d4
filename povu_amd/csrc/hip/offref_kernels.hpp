// offref_kernels.hpp -- the off-reference calls of povu_hip_call with POVU_HIP_T_OFFREF (offref_kernels.hip; INTEGRATION.md
// "Off-reference calls"): what the call hands the steps and what they leave on the device (the context's off-reference
// arenas, valid until the next such call on the context).  Without the flag povu_hip_call runs none of this.
#pragma once
#include "call_common.hpp"

namespace povu_hip
{

// offref_sites: per site the surrogate path of a site called off-reference (NO_QUERY elsewhere; such a site is set in the
// call's `called` too); per path whether it is the surrogate of such a site of two alleles or more; the calling paths, the
// reference paths and those surrogates in one ascending list of n_call
struct OffrefSites {
	uint32_t *sur = nullptr;   // [n]
	uint8_t *is_sur = nullptr; // [P]
	uint32_t *call_path = nullptr; // [n_call]
	uint32_t n_call = 0;
	uint64_t n_sites = 0; // called off-reference, two alleles or more
};
OffrefSites offref_sites(povu_hip_ctx *ctx, const TravDevice &d, uint32_t n, const uint32_t *parent, const uint8_t *fam, const uint8_t *callable,
			 uint8_t *called, const uint32_t *ref_of_path);

// surrogate_offsets, the part that is the off-reference calls' own: the arrays of the view of the calling paths (the caller
// fills ref_base and runs the gather and the scan of the references' offsets over them), ref_of_path filled from call_path
struct OffrefView {
	uint32_t *ref_of_path = nullptr; // [P]
	uint64_t *ref_base = nullptr;	 // [n_call + 1]
	uint64_t *rlen = nullptr, *roff = nullptr, *s64 = nullptr; // [NR + 1] twice, the scan's scratch
};
OffrefView offref_view(povu_hip_ctx *ctx, const OffrefSites &o, uint64_t NR);

// the reference numbers of the inversion records (`ref`, numbered among the reference paths `ref_path`) as numbers among the
// calling paths: the key the one record list is merged by
uint32_t *offref_inv_refs(povu_hip_ctx *ctx, uint32_t n_inv, const uint32_t *ref, const uint32_t *ref_path, const uint32_t *call_of_path);

// offref_hosts: per flubble record j before the sort (traversal v.rlist[j]) the winning offer of a host (offref_rules.hpp;
// OFFREF_NO_HOST: none) and the host traversal
struct OffrefHosts {
	unsigned long long *key = nullptr; // [nfl]
	uint32_t *trav = nullptr;	   // [nfl]
};
OffrefHosts offref_hosts(povu_hip_ctx *ctx, const TravDevice &d, const CallView &v, const OffrefSites &o);

// the rows' own arrays: per row of the record list whether it is an off-reference record, its host's site and exact allele
// (NO_QUERY: none; inversion rows: 0 and none); perm / dst as in call_kernels.hip (row dst[i], or i, holds record perm[i])
struct OffrefRows {
	uint8_t *rec_offref = nullptr;
	uint32_t *host_query = nullptr, *host_allele = nullptr;
	uint64_t n_records = 0, n_hosted = 0;
};
OffrefRows offref_rows(povu_hip_ctx *ctx, const CallView &v, const OffrefSites &o, const OffrefHosts &h, uint32_t nrec, uint32_t nfl,
		       const uint32_t *perm, const uint32_t *dst);

} // namespace povu_hip
