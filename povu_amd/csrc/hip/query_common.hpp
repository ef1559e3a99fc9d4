// query_common.hpp -- what the walks (walk_kernels.hip) and the traversals (trav_kernels.hip) share: the queries of a forest
// (every PVST vertex but the roots, tree order then vertex order), the refusals of forests they cannot read, and the
// resolution of a query's boundary steps to entered sides on the device (segment ids must ascend with the vertex index).
#pragma once
#include "context.hpp"

namespace povu_hip
{

static constexpr uint32_t NO_QUERY = 0xFFFFFFFFu;

// vertex index of segment `id` in the ascending `vid`, NO_QUERY when the graph has no such segment
__device__ __forceinline__ uint32_t find_vertex(const uint32_t *__restrict__ vid, uint32_t V, uint32_t id)
{
	uint32_t lo = 0, hi = V;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (vid[mid] < id)
			lo = mid + 1;
		else
			hi = mid;
	}
	return (lo < V && vid[lo] == id) ? lo : NO_QUERY;
}

// throws unless `f` was made by povu_hip_decompose on `ctx` from the graph now resident there (no shard, merge or attach);
// `what` names the caller in the message ("walks", "traversals")
void check_query_forest(const povu_hip_ctx *ctx, const povu_hip_forest *f, const char *what);
// (S id, Z id, or1 | or2 << 1) of every query of `f`
void forest_queries(povu_hip_forest *f, std::vector<uint32_t> &qa, std::vector<uint32_t> &qz, std::vector<uint8_t> &qor);
// bit 0 of *bad when vid does not ascend
void launch_vid_ascending(uint32_t V, const uint32_t *vid, uint32_t *bad, hipStream_t s);
// entered sides of both boundaries (ys = 2 a + or1, yz = 2 z + or2; NO_QUERY for a query whose boundaries are one segment);
// bit 1 of *bad when a boundary is no segment of the graph
void launch_resolve(uint32_t n, const uint32_t *qa, const uint32_t *qz, const uint8_t *qor, const uint32_t *vid, uint32_t V,
		    uint32_t *ys, uint32_t *yz, uint32_t *bad, hipStream_t s);

} // namespace povu_hip
