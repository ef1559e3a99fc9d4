// cluster_kernels.hpp -- the clustered calls of povu_hip_call_clustered (cluster_kernels.hip; INTEGRATION.md "Clustered
// calls"): what the call hands the step and what it leaves on the device (the context's nest arenas ns_cls and ns_ws, which a
// clustered call does not otherwise use: nested is refused with it; valid until the next clustered or nested call).
#pragma once
#include "call_common.hpp"

namespace povu_hip
{

// the clusters: of site q the clusters [coff[q], coff[q + 1]), numbered in the order of their founding exact allele; of cluster
// c its representative's global exact allele crep[c], that allele's first traversal cfirst[c] and its exact alleles csize[c];
// of traversal t its cluster within its site, oc[t]; of site q the lowest sim_ppm of a member to its representative, minsim[q].
// A site that is not called or has fewer than two exact alleles keeps its exact alleles as clusters of one
struct ClusterClasses {
	uint32_t n_cl = 0;
	uint32_t *coff = nullptr, *crep = nullptr, *cfirst = nullptr, *oc = nullptr, *csize = nullptr, *minsim = nullptr;
	uint64_t n_sites = 0, n_keys = 0, n_pairs = 0, n_pruned = 0, n_tier2 = 0;
};
// `called`: [n] the called sites; T: the threshold in ppm; no_bound: no pair is skipped; force_tier2: every bag through the
// device-wide sort
ClusterClasses cluster_classes(povu_hip_ctx *ctx, const TravDevice &d, const uint8_t *called, uint32_t T, bool no_bound, bool force_tier2);

} // namespace povu_hip
