// region_kernels.hpp -- the region calls of povu_hip_call_restricted (region_kernels.hip; INTEGRATION.md "Region calls";
// rules: region_rules.hpp): what the call hands the steps and what they leave on the device.  Everything lives in the arena of
// the call's query front end, next to the queries (no arena of its own), and is read until the flubble records are chosen
// (region_select) and the inversion records are reported.  Without regions povu_hip_call runs none of this.
#pragma once
#include "call_common.hpp"
#include "region_rules.hpp"

namespace povu_hip
{

// the regions of a call as the host made them (region_prepare): normalised, their paths' steps concatenated
struct RegionIn {
	bool active = false; // the call has regions
	bool mask = false;   // the sites that do not pass lose their scans (else the records are selected at the end alone)
	region::Normalised n;
	std::vector<uint64_t> base; // [paths + 1] first step of every region path in the concatenation
};
// the refusals of the regions and their normalisation; reads the resident paths' lengths (waits for the stream)
RegionIn region_prepare(povu_hip_ctx *ctx, const povu_hip_call_regions *regions, bool mask_allowed);

// the device arrays, carved by region_spans from the front end's layout
struct RegionWs {
	uint32_t *path = nullptr, *first = nullptr, *bitmap = nullptr, *words = nullptr; // words: [0] the sites that pass
	uint64_t *base = nullptr, *iv_s = nullptr, *iv_e = nullptr, *rlen = nullptr, *roff = nullptr, *s64 = nullptr;
	uint8_t *pass = nullptr;
};
void region_spans(const povu_hip_ctx *ctx, const RegionIn &in, uint32_t n, RegionWs &w, Spans &take);

// what the rest of the call reads
struct RegionDevice {
	const uint32_t *marked = nullptr; // [(V + 31) / 32] bit v: segment v is marked
	const uint8_t *pass = nullptr;	   // [n] the site passes
	uint32_t n_regions = 0;		   // after normalisation
	uint64_t n_sites = 0, n_masked = 0, n_dropped = 0;
};
// behind query_front: the offsets of the region paths, the marked segments, the sites that pass; with in.mask the others'
// entered sides become NO_QUERY (q.ys / q.yz: the front end's arrays).  Waits for the stream (the count of the sites)
RegionDevice region_sites(povu_hip_ctx *ctx, const RegionIn &in, const QueryFront &q, const RegionWs &w);

// The late filter: of the n flubble records list[0 .. n) (indices into v.rlist) those whose site passes, in order, into `out`;
// gives their number.  flag [n], idx [n], count: one cleared word, tmp as compact_flagged_u8 takes it
uint32_t region_select(povu_hip_ctx *ctx, const CallView &v, const uint8_t *pass, const uint32_t *list, uint32_t n, uint8_t *flag, uint32_t *idx,
		       uint32_t *out, uint32_t *count, void *tmp, size_t tmp_bytes);

} // namespace povu_hip
