// region_kernels.hip -- the region calls (region_kernels.hpp; INTEGRATION.md "Region calls"): the regions of a call turned
// into a mask of its sites in front of the traversal pipeline, and the selection of the records behind it.
//   offsets   the steps of the distinct region paths concatenated, the segment lengths gathered, one exclusive u64 scan (as for
//             the reference paths and the surrogates: launch_ref_len);
//   k_rg_mark a pass over those steps: the step's positions searched in its path's merged intervals (region_rules.hpp), a hit
//             sets the segment's bit.  Steps and offsets are read in order; the atomicOr is the one scattered access;
//   k_rg_sites  per site both boundaries' bits: the site passes when either is set; the passing sites are counted;
//   k_rg_mask   a site that does not pass gets NO_QUERY for both entered sides: it enters no boundary-table entry, starts no
//             scan and has no allele (trav_kernels.hip);
//   k_rg_flag / k_rg_gather  the late filter over a list of flubble records.
#include "region_kernels.hpp"

namespace povu_hip
{

__global__ void k_rg_mark(RefView R, PathsView P, const uint32_t *__restrict__ first, const uint64_t *__restrict__ iv_s,
			  const uint64_t *__restrict__ iv_e, uint32_t *__restrict__ bitmap)
{
	for (uint64_t i = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; i < R.NR; i += (uint64_t)gridDim.x * Q_TPB) {
		const uint32_t r = span_of(R.ref_base, R.nR, i);
		const uint64_t at = R.roff[i], off = at - R.roff[R.ref_base[r]], len = R.roff[i + 1] - at;
		if (region::step_in_any(iv_s, iv_e, first[r], first[r + 1], off, len)) {
			const uint32_t v = P.steps[P.path_off[R.ref_path[r]] + (i - R.ref_base[r])] >> 1;
			atomicOr(bitmap + (v >> 5), 1u << (v & 31));
		}
	}
}

__device__ __forceinline__ bool rg_marked(const uint32_t *__restrict__ bitmap, uint32_t v) { return v != NO_QUERY && ((bitmap[v >> 5] >> (v & 31)) & 1u); }

__global__ void k_rg_sites(uint32_t n, const uint32_t *__restrict__ qa, const uint32_t *__restrict__ qz, const uint32_t *__restrict__ vid, uint32_t V,
			   const uint32_t *__restrict__ bitmap, uint8_t *__restrict__ pass, uint32_t *__restrict__ n_pass)
{
	uint32_t mine = 0;
	for (uint32_t q = blockIdx.x * Q_TPB + threadIdx.x; q < n; q += gridDim.x * Q_TPB) {
		const bool p = rg_marked(bitmap, find_vertex(vid, V, qa[q])) || rg_marked(bitmap, find_vertex(vid, V, qz[q]));
		pass[q] = p;
		mine += p;
	}
	mine = wave_sum(mine);
	if ((threadIdx.x & 63u) == 0 && mine)
		atomicAdd(n_pass, mine);
}

__global__ void k_rg_mask(uint32_t n, const uint8_t *__restrict__ pass, uint32_t *__restrict__ ys, uint32_t *__restrict__ yz)
{
	for (uint32_t q = blockIdx.x * Q_TPB + threadIdx.x; q < n; q += gridDim.x * Q_TPB)
		if (!pass[q])
			ys[q] = yz[q] = NO_QUERY;
}

// flag[k]: the site of flubble record list[k] passes
__global__ void k_rg_flag(uint32_t n, const uint32_t *__restrict__ list, const uint32_t *__restrict__ rlist, const uint32_t *__restrict__ rq,
			  const uint8_t *__restrict__ pass, uint8_t *__restrict__ flag)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < n; k += gridDim.x * Q_TPB)
		flag[k] = pass[rq[rlist[list[k]]]];
}
__global__ void k_rg_gather(uint32_t m, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ list, uint32_t *__restrict__ out)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < m; k += gridDim.x * Q_TPB)
		out[k] = list[idx[k]];
}

RegionIn region_prepare(povu_hip_ctx *ctx, const povu_hip_call_regions *regions, bool mask_allowed)
{
	RegionIn in;
	if (!regions || !regions->n)
		return in;
	if (regions->n > region::MAX_REGIONS)
		throw HipError(std::to_string(regions->n) + " regions: more than " + std::to_string(region::MAX_REGIONS) + " are refused");
	if (!regions->region)
		throw HipError("null region array");
	const uint32_t P = ctx->n_paths;
	std::vector<region::Region> list(regions->n);
	for (uint32_t k = 0; k < regions->n; k++) {
		const povu_hip_region &r = regions->region[k];
		if (r.path >= P)
			throw HipError("region " + std::to_string(k) + ": path " + std::to_string(r.path) + " is no resident path (" + std::to_string(P) +
				       " are resident)");
		if (r.start >= r.end || r.end >= region::END_LIMIT)
			throw HipError("region " + std::to_string(k) + ": [" + std::to_string(r.start) + ", " + std::to_string(r.end) +
				       ") is no interval with start < end < 2^63");
		list[k] = region::Region{r.path, r.start, r.end};
	}
	in.active = true;
	in.mask = mask_allowed && !(regions->flags & POVU_HIP_REGION_NO_MASK);
	in.n = region::normalise(std::move(list));
	HIP_CHECK(hipSetDevice(ctx->device));
	ctx->wait_tail();
	std::vector<uint64_t> path_off((size_t)P + 1);
	HIP_CHECK(copy_async(path_off.data(), ctx->path_off, ((size_t)P + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
	HIP_CHECK(hipStreamSynchronize(ctx->stream));
	in.base.assign(in.n.path.size() + 1, 0);
	for (size_t k = 0; k < in.n.path.size(); k++)
		in.base[k + 1] = in.base[k] + path_off[in.n.path[k] + 1] - path_off[in.n.path[k]];
	return in;
}

void region_spans(const povu_hip_ctx *ctx, const RegionIn &in, uint32_t n, RegionWs &w, Spans &take)
{
	const size_t nP = in.n.path.size(), nI = in.n.s.size();
	const uint64_t NR = in.base.back();
	take(nP + 1, w.path, w.first, w.base);
	take(nI + 1, w.iv_s, w.iv_e);
	take(NR + 1, w.rlen, w.roff);
	take(scan_exclusive_u64_tmp(std::max<uint64_t>(NR + 1, 1)), w.s64);
	take(((size_t)ctx->g.V + 31) / 32 + 1, w.bitmap);
	take((size_t)n + 1, w.pass);
	take(8, w.words);
}

RegionDevice region_sites(povu_hip_ctx *ctx, const RegionIn &in, const QueryFront &q, const RegionWs &w)
{
	hipStream_t s = ctx->stream;
	const ResidentGraph &g = ctx->g;
	const uint32_t nP = (uint32_t)in.n.path.size(), nI = (uint32_t)in.n.s.size(), n = q.n;
	const uint64_t NR = in.base.back();
	const size_t words = ((size_t)g.V + 31) / 32 + 1;
	HIP_CHECK(copy_async(w.path, in.n.path.data(), (size_t)nP * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(copy_async(w.first, in.n.first.data(), ((size_t)nP + 1) * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(copy_async(w.base, in.base.data(), ((size_t)nP + 1) * 8, hipMemcpyHostToDevice, s));
	HIP_CHECK(copy_async(w.iv_s, in.n.s.data(), (size_t)nI * 8, hipMemcpyHostToDevice, s));
	HIP_CHECK(copy_async(w.iv_e, in.n.e.data(), (size_t)nI * 8, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemsetAsync(w.bitmap, 0, words * 4, s));
	HIP_CHECK(hipMemsetAsync(w.words, 0, 32, s));
	HIP_CHECK(hipMemsetAsync(w.rlen + NR, 0, 8, s));
	// the region paths as a view of "reference paths" (no path -> number table: nothing here asks for one)
	const RefView R{NR, nP, nullptr, w.path, w.base, w.roff};
	const PathsView P = paths_view(ctx);
	if (NR)
		launch_ref_len(R, P, w.rlen, s);
	scan_exclusive_u64(w.rlen, w.roff, NR + 1, w.s64, s);
	if (NR)
		KLAUNCH(k_rg_mark, dim3(stride_blocks(NR)), dim3(Q_TPB), 0, s, R, P, w.first, w.iv_s, w.iv_e, w.bitmap);
	RegionDevice d;
	d.marked = w.bitmap, d.pass = w.pass, d.n_regions = nI;
	if (n) {
		KLAUNCH(k_rg_sites, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, q.qa, q.qz, g.vid, g.V, w.bitmap, w.pass, w.words);
		if (in.mask) // (the arrays are the arena's: the const on QueryFront is the view's)
			KLAUNCH(k_rg_mask, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, w.pass, const_cast<uint32_t *>(q.ys), const_cast<uint32_t *>(q.yz));
	}
	d.n_sites = read_back(w.words, s);
	d.n_masked = in.mask ? n - d.n_sites : 0;
	return d;
}

uint32_t region_select(povu_hip_ctx *ctx, const CallView &v, const uint8_t *pass, const uint32_t *list, uint32_t n, uint8_t *flag, uint32_t *idx,
		       uint32_t *out, uint32_t *count, void *tmp, size_t tmp_bytes)
{
	hipStream_t s = ctx->stream;
	if (!n)
		return 0;
	KLAUNCH(k_rg_flag, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, list, v.rlist, v.trav.rq, pass, flag);
	compact_flagged_u8(flag, n, idx, count, tmp, tmp_bytes, s);
	const uint32_t m = read_back(count, s);
	if (m)
		KLAUNCH(k_rg_gather, dim3(stride_blocks(m)), dim3(Q_TPB), 0, s, m, idx, list, out);
	return m;
}

} // namespace povu_hip
