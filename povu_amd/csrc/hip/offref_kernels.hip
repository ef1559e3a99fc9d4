// offref_kernels.hip -- the off-reference calls of povu_hip_call with POVU_HIP_T_OFFREF (include/povu_hip.h).
//
// The definition is this project's own ("Off-reference calls (decided here, not reference behaviour)";
// restated in tests/offref_ref.py; the rules that are plain arithmetic live in offref_rules.hpp).  A site the reference
// paths do not cross is called on its surrogate, the path of its first traversal.  The steps of povu_hip_call, each
// skipped on the host without the flag:
//   offref_sites       (behind callability) a lane a site: candidate, from the climb to the root and the site's traversal
//                      range; an unparent pass clears "called off-reference" of every parent of a callable or candidate
//                      child; a lane a site then writes its surrogate, sets the call's `called` and flags the surrogate's
//                      path; the flags of the reference paths and the surrogates are compacted into the ascending list of the
//                      calling paths;
//   surrogate_offsets  (call_kernels.hip) k_cl_ref_len's gather and the u64 scan of the references' offsets, over the calling paths;
//   offref_hosts       (behind flubble_records) the index of nest_kernels.hip over the traversals of the kept sites by
//                      surrogate paths; a wave per entry of a site the references call walks the entries that start inside
//                      it and offers (steps, site) by atomic minimum to every enclosed off-reference record; a second walk
//                      names the traversal of the winning offer;
//   offref_rows        (behind spelling) a lane per sorted flubble record writes its row's three arrays.
// The kept sites, the slot table, the records and the spelling take the union through CallView (sur).
//
// What cannot hang: every trip count is fixed before its loop (the climb is bounded by the number of sites, the walk by two
// binary searches made before it); no kernel waits on another wave; the shuffles (wave_sum) run outside every divergent
// branch, with all 64 lanes; every store is range-checked against the length of its array.
#include "offref_kernels.hpp"
#include "nest_kernels.hpp"
#include "offref_rules.hpp"

namespace povu_hip
{

// ---- offref_sites
__global__ void k_or_candidate(uint32_t n, const uint32_t *__restrict__ parent, const uint8_t *__restrict__ fam, const uint8_t *__restrict__ callable,
			       const uint32_t *__restrict__ toff, uint8_t *__restrict__ cand, uint8_t *__restrict__ off)
{
	for (uint32_t q = blockIdx.x * Q_TPB + threadIdx.x; q < n; q += gridDim.x * Q_TPB) {
		bool under = false;
		for (uint32_t v = q, k = 0; v < n && k <= n; v = parent[v], k++)
			under |= offref_is_subflubble(fam[v]);
		cand[q] = off[q] = offref_candidate(under, callable[q] != 0, toff[q + 1] - toff[q]);
	}
}
__global__ void k_or_unparent(uint32_t n, const uint8_t *__restrict__ callable, const uint8_t *__restrict__ cand, const uint32_t *__restrict__ parent,
			      uint8_t *__restrict__ off)
{
	for (uint32_t q = blockIdx.x * Q_TPB + threadIdx.x; q < n; q += gridDim.x * Q_TPB)
		if (offref_clears_parent(callable[q] != 0, cand[q] != 0) && parent[q] < n)
			off[parent[q]] = 0;
}
__global__ void k_or_path_flag(uint32_t P, const uint32_t *__restrict__ ref_of_path, uint8_t *__restrict__ pflag, uint8_t *__restrict__ is_sur)
{
	for (uint32_t p = blockIdx.x * Q_TPB + threadIdx.x; p < P; p += gridDim.x * Q_TPB) {
		pflag[p] = ref_of_path[p] != NO_QUERY;
		is_sur[p] = 0;
	}
}
__global__ void k_or_surrogate(uint32_t n, uint32_t P, uint32_t R, const uint8_t *__restrict__ off, const uint32_t *__restrict__ toff,
			       const uint32_t *__restrict__ op, const uint32_t *__restrict__ aoff, uint32_t *__restrict__ sur, uint8_t *__restrict__ called,
			       uint8_t *__restrict__ is_sur, uint8_t *__restrict__ pflag, unsigned long long *__restrict__ cnt)
{
	for (uint32_t q = blockIdx.x * Q_TPB + threadIdx.x; q < n; q += gridDim.x * Q_TPB) {
		uint32_t s = NO_QUERY;
		if (off[q] && toff[q] < R) {
			s = op[toff[q]];
			called[q] = 1;
			if (aoff[q + 1] - aoff[q] >= 2 && s < P) {
				is_sur[s] = 1;
				pflag[s] = 1;
				atomicAdd(cnt, 1ull);
			}
		}
		sur[q] = s;
	}
}

OffrefSites offref_sites(povu_hip_ctx *ctx, const TravDevice &d, uint32_t n, const uint32_t *parent, const uint8_t *fam, const uint8_t *callable,
			 uint8_t *called, const uint32_t *ref_of_path)
{
	hipStream_t s = ctx->stream;
	const uint32_t P = ctx->n_paths;
	const size_t n1 = (size_t)n + 1, P1 = (size_t)P + 1;
	OffrefSites o;
	uint8_t *cand, *off, *pflag;
	uint32_t *count;
	unsigned long long *cnt;
	void *tmp;
	const size_t tmp_bytes = prim_tmp_bytes(P1, false) + 256;
	carve(ctx->or_ws, [&](Spans &take) {
		take(n1, o.sur, cand, off);
		take(P1, o.is_sur, pflag, o.call_path);
		take(2, count);
		take(1, cnt);
		take(tmp_bytes, tmp);
	});
	HIP_CHECK(hipMemsetAsync(count, 0, 8, s));
	HIP_CHECK(hipMemsetAsync(cnt, 0, 8, s));
	if (P)
		KLAUNCH(k_or_path_flag, dim3(stride_blocks(P)), dim3(Q_TPB), 0, s, P, ref_of_path, pflag, o.is_sur);
	if (n) {
		KLAUNCH(k_or_candidate, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, parent, fam, callable, d.toff, cand, off);
		KLAUNCH(k_or_unparent, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, callable, cand, parent, off);
		KLAUNCH(k_or_surrogate, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, P, d.R, off, d.toff, d.op, d.aoff, o.sur, called, o.is_sur, pflag, cnt);
	}
	if (P)
		compact_flagged_u8(pflag, P, o.call_path, count, tmp, tmp_bytes, s);
	HIP_CHECK(copy_async(&o.n_call, count, 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(copy_async(&o.n_sites, cnt, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	return o;
}

// ---- surrogate_offsets
__global__ void k_or_number(uint32_t n_call, uint32_t P, const uint32_t *__restrict__ call_path, uint32_t *__restrict__ ref_of_path)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < n_call; k += gridDim.x * Q_TPB)
		if (call_path[k] < P)
			ref_of_path[call_path[k]] = k;
}
OffrefView offref_view(povu_hip_ctx *ctx, const OffrefSites &o, uint64_t NR)
{
	hipStream_t s = ctx->stream;
	const uint32_t P = ctx->n_paths;
	OffrefView v;
	carve(ctx->or_view, [&](Spans &take) {
		take((size_t)P + 1, v.ref_of_path);
		take((size_t)o.n_call + 1, v.ref_base);
		take(NR + 1, v.rlen, v.roff);
		take(scan_exclusive_u64_tmp(NR + 1), v.s64);
	});
	HIP_CHECK(hipMemsetAsync(v.ref_of_path, 0xFF, ((size_t)P + 1) * 4, s));
	if (o.n_call)
		KLAUNCH(k_or_number, dim3(stride_blocks(o.n_call)), dim3(Q_TPB), 0, s, o.n_call, P, o.call_path, v.ref_of_path);
	return v;
}

__global__ void k_or_inv_refs(uint32_t n, uint32_t P, const uint32_t *__restrict__ ref, const uint32_t *__restrict__ ref_path,
			      const uint32_t *__restrict__ call_of_path, uint32_t *__restrict__ out)
{
	for (uint32_t b = blockIdx.x * Q_TPB + threadIdx.x; b < n; b += gridDim.x * Q_TPB) {
		const uint32_t p = ref_path[ref[b]];
		out[b] = p < P ? call_of_path[p] : NO_QUERY;
	}
}
uint32_t *offref_inv_refs(povu_hip_ctx *ctx, uint32_t n_inv, const uint32_t *ref, const uint32_t *ref_path, const uint32_t *call_of_path)
{
	uint32_t *out;
	carve(ctx->or_inv, [&](Spans &take) { take((size_t)n_inv + 1, out); });
	if (n_inv)
		KLAUNCH(k_or_inv_refs, dim3(stride_blocks(n_inv)), dim3(Q_TPB), 0, ctx->stream, n_inv, ctx->n_paths, ref, ref_path, call_of_path, out);
	return out;
}

// ---- offref_hosts
// the traversals of the kept sites by surrogate paths: every one of a site the references call, the surrogate's own of a site
// called off-reference (its records)
__global__ void k_or_index_flag(uint32_t R, const uint32_t *__restrict__ rq, const uint32_t *__restrict__ op, const uint32_t *__restrict__ keep,
				const uint32_t *__restrict__ sur, const uint8_t *__restrict__ is_sur, uint8_t *__restrict__ flag)
{
	for (uint32_t t = blockIdx.x * Q_TPB + threadIdx.x; t < R; t += gridDim.x * Q_TPB) {
		const uint32_t q = rq[t], p = op[t];
		flag[t] = keep[q] && is_sur[p] && (sur[q] == NO_QUERY || sur[q] == p);
	}
}
__global__ void k_or_rec_of(uint32_t nfl, uint32_t R, const uint32_t *__restrict__ rlist, uint32_t *__restrict__ rec_of)
{
	for (uint32_t j = blockIdx.x * Q_TPB + threadIdx.x; j < nfl; j += gridDim.x * Q_TPB)
		if (rlist[j] < R)
			rec_of[rlist[j]] = j;
}
// a wave per index entry of a site the references call: its offer to every off-reference record it encloses.  which 0: the
// minimum of the keys; which 1: the lowest traversal among the offers that won
__global__ __launch_bounds__(Q_TPB) void k_or_offer(NestIndex ix, uint32_t nfl, int which, const uint32_t *__restrict__ sur,
						    const uint32_t *__restrict__ rec_of, unsigned long long *__restrict__ key, uint32_t *__restrict__ trav)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	for (uint32_t x0 = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); x0 < ix.ni; x0 += waves) {
		const uint32_t q = ix.iq[x0];
		if (sur[q] != NO_QUERY)
			continue;
		const uint64_t pos = ix.ipos[x0], end = ix.iend[x0];
		const unsigned long long mine = offref_host_key((uint32_t)(end - pos + 1), q);
		const uint32_t lo = lower_bound(ix.ipos, 0u, ix.ni, pos), hi = lower_bound(ix.ipos, 0u, ix.ni, end + 1);
		for (uint32_t x = lo + lane; x < hi; x += 64) {
			if (sur[ix.iq[x]] == NO_QUERY || !offref_encloses(pos, end, ix.ipos[x], ix.iend[x]))
				continue;
			const uint32_t jj = rec_of[ix.it[x]];
			if (jj >= nfl)
				continue;
			if (which == 0)
				atomicMin(key + jj, mine);
			else if (key[jj] == mine)
				atomicMin(trav + jj, ix.it[x0]);
		}
	}
}

OffrefHosts offref_hosts(povu_hip_ctx *ctx, const TravDevice &d, const CallView &v, const OffrefSites &o)
{
	hipStream_t s = ctx->stream;
	const uint32_t R = d.R, nfl = v.nfl;
	const size_t R1 = (size_t)R + 1, F1 = (size_t)nfl + 1;
	OffrefHosts h;
	NestIndex ix;
	uint8_t *flag;
	uint32_t *ilist, *pb, *key, *kout, *count, *rec_of;
	void *tmp;
	const size_t tmp_bytes = prim_tmp_bytes(R1, true) + 256;
	carve(ctx->or_host, [&](Spans &take) {
		take(F1, h.key, h.trav);
		take(R1, ix.ipos, ix.iend, ix.iq, ix.it, flag, ilist, pb, key, kout, rec_of);
		take(2, count);
		take(tmp_bytes, tmp);
	});
	HIP_CHECK(hipMemsetAsync(h.key, 0xFF, F1 * 8, s));
	HIP_CHECK(hipMemsetAsync(h.trav, 0xFF, F1 * 4, s));
	if (!nfl || !R || !o.n_sites)
		return h;
	HIP_CHECK(hipMemsetAsync(count, 0, 8, s));
	HIP_CHECK(hipMemsetAsync(rec_of, 0xFF, R1 * 4, s));
	KLAUNCH(k_or_index_flag, dim3(stride_blocks(R)), dim3(Q_TPB), 0, s, R, d.rq, d.op, v.keep, o.sur, o.is_sur, flag);
	nest_index(ctx, d, flag, ix, NestIndexWs{ilist, pb, key, kout, count, tmp, tmp_bytes});
	if (!ix.ni)
		return h;
	KLAUNCH(k_or_rec_of, dim3(stride_blocks(nfl)), dim3(Q_TPB), 0, s, nfl, R, v.rlist, rec_of);
	for (int which = 0; which < 2; which++)
		KLAUNCH(k_or_offer, dim3(wave_blocks(ix.ni)), dim3(Q_TPB), 0, s, ix, nfl, which, o.sur, rec_of, h.key, h.trav);
	return h;
}

// ---- offref_rows
__global__ __launch_bounds__(Q_TPB) void k_or_rows(uint32_t nfl, uint32_t nrec, uint32_t R, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ dst,
						   const uint32_t *__restrict__ rlist, const uint32_t *__restrict__ rq, const uint32_t *__restrict__ oa,
						   const uint32_t *__restrict__ sur, const unsigned long long *__restrict__ key,
						   const uint32_t *__restrict__ trav, uint8_t *__restrict__ rec_offref, uint32_t *__restrict__ host_query,
						   uint32_t *__restrict__ host_allele, unsigned long long *__restrict__ cnt)
{
	for (uint32_t i0 = blockIdx.x * Q_TPB; i0 < nfl; i0 += gridDim.x * Q_TPB) {
		const uint32_t i = i0 + threadIdx.x;
		uint32_t is_off = 0, hosted = 0;
		if (i < nfl) {
			const uint32_t j = perm[i], d = dst ? dst[i] : i;
			is_off = sur[rq[rlist[j]]] != NO_QUERY;
			hosted = is_off && key[j] != OFFREF_NO_HOST && trav[j] < R;
			if (d < nrec) {
				rec_offref[d] = (uint8_t)is_off;
				host_query[d] = hosted ? offref_host_site(key[j]) : NO_QUERY;
				host_allele[d] = hosted ? oa[trav[j]] : NO_QUERY;
			}
		}
		is_off = wave_sum(is_off);
		hosted = wave_sum(hosted);
		if ((threadIdx.x & 63u) == 0) {
			if (is_off)
				atomicAdd(cnt, (unsigned long long)is_off);
			if (hosted)
				atomicAdd(cnt + 1, (unsigned long long)hosted);
		}
	}
}

OffrefRows offref_rows(povu_hip_ctx *ctx, const CallView &v, const OffrefSites &o, const OffrefHosts &h, uint32_t nrec, uint32_t nfl,
		       const uint32_t *perm, const uint32_t *dst)
{
	hipStream_t s = ctx->stream;
	const size_t r1 = (size_t)nrec + 1;
	OffrefRows r;
	unsigned long long *cnt;
	carve(ctx->or_rows, [&](Spans &take) {
		take(r1, r.rec_offref, r.host_query, r.host_allele);
		take(2, cnt);
	});
	HIP_CHECK(hipMemsetAsync(r.rec_offref, 0, r1, s));
	HIP_CHECK(hipMemsetAsync(r.host_query, 0xFF, r1 * 4, s));
	HIP_CHECK(hipMemsetAsync(r.host_allele, 0xFF, r1 * 4, s));
	HIP_CHECK(hipMemsetAsync(cnt, 0, 16, s));
	if (nfl)
		KLAUNCH(k_or_rows, dim3(stride_blocks(nfl)), dim3(Q_TPB), 0, s, nfl, nrec, v.trav.R, perm, dst, v.rlist, v.trav.rq, v.trav.oa, o.sur, h.key,
			h.trav, r.rec_offref, r.host_query, r.host_allele, cnt);
	unsigned long long hc[2] = {0, 0};
	HIP_CHECK(copy_async(hc, cnt, 16, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	r.n_records = hc[0], r.n_hosted = hc[1];
	return r;
}

} // namespace povu_hip
