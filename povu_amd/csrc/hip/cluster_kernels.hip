// cluster_kernels.hip -- the clustered calls of povu_hip_call_clustered (include/povu_hip.h).
//
// The definition is this project's own, modelled on `vg deconstruct -L` ("Clustered calls"; restated in
// tests/cluster_ref.py; the rules themselves: cluster_rules.hpp).  One step of the call, between callability and the kept
// sites, that fills what a nested call's classes fill (coff, oc, cfirst, crep):
//   bags     per exact allele of a called site of two exact alleles or more, from its first traversal: the segments of its inner
//            steps.  Counts, one u32 scan to bag_off, then a wave per allele writes the keys (lanes across the steps) and the
//            bag's weight W (a wave sum of the segments' bases, u64);
//   sort     every bag by segment, every key with its ordinal among the equal segments of its bag (u16), so that the multiset
//            intersection with a bag r is "key (s, o) counts when o < count_r(s)".  Tier 1: a bag of up to 64 keys is sorted
//            by one wave in registers (a bitonic network over the lanes) and numbered by a wave prefix maximum of the run
//            heads.  Tier 2: the keys of the longer bags are compacted and sorted device-wide (LsdSort: segment bits, then
//            the allele); a sorted key goes back to the slot of the same rank in its bag, run heads and
//            scan_exclusive_max_u32 give the ordinals;
//   cluster  a wave per site walks its exact alleles in order (leader clustering).  The allele's keys sit in the lanes, 64 a
//            chunk; for every representative so far the weight bound decides whether the pair is read at all, else every lane
//            finds count_r(s) by two binary searches in the representative's sorted bag and the weights that count are summed
//            over the wave in 64 bits; the best similar representative is kept by better().  Representatives are at most as
//            many as the site's exact alleles and live in the site's stretch of a global array;
//   close    the cluster counts scanned to coff; crep, cfirst, csize per cluster; oc per traversal.
// Work: per site (exact alleles) x (clusters) pairs, each at most (keys of the allele) x log(keys of the representative).
#include "cluster_kernels.hpp"

#include "cluster_rules.hpp"

namespace povu_hip
{

static constexpr uint32_t C1_KEYS = 64; // keys of the longest bag tier 1 sorts

// ---- bags
// site, key count and tier of every exact allele; cnt64[2] += candidate sites (counted at their first allele), cnt64[3] += bags
// of tier 2
__global__ void k_cu_count(uint32_t n_al, const uint32_t *__restrict__ afirst, const uint32_t *__restrict__ rq, const uint32_t *__restrict__ rlen,
			   const uint32_t *__restrict__ aoff, const uint8_t *__restrict__ called, uint32_t force2, uint32_t *__restrict__ aq,
			   uint32_t *__restrict__ cnt, uint8_t *__restrict__ hand, unsigned long long *__restrict__ cnt64)
{
	for (uint32_t a = blockIdx.x * Q_TPB + threadIdx.x; a <= n_al; a += gridDim.x * Q_TPB) {
		if (a == n_al) {
			cnt[a] = 0;
			continue;
		}
		const uint32_t t = afirst[a], q = rq[t];
		const bool cand = called[q] && aoff[q + 1] - aoff[q] >= 2;
		const uint32_t m = cand && rlen[t] > 2 ? rlen[t] - 2 : 0;
		aq[a] = q;
		cnt[a] = m;
		hand[a] = m && (force2 || m > C1_KEYS);
		if (cand && a == aoff[q])
			atomicAdd(cnt64 + 2, 1ull);
		if (hand[a])
			atomicAdd(cnt64 + 3, 1ull);
	}
}
// a wave per allele: its keys (the vertex of every inner step), their allele, the bag's weight
__global__ __launch_bounds__(Q_TPB) void k_cu_fill(uint32_t n_al, const uint32_t *__restrict__ afirst, const uint64_t *__restrict__ rpos,
						   const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ steps,
						   const uint64_t *__restrict__ seq_off, const uint32_t *__restrict__ bag_off,
						   uint32_t *__restrict__ seg, uint32_t *__restrict__ kal, uint64_t *__restrict__ W)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	for (uint32_t a = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); a < n_al; a += waves) {
		const uint32_t b = bag_off[a], m = bag_off[a + 1] - b;
		uint64_t w = 0;
		if (m) {
			const TravSpan sp = trav_span(rpos, rlen, afirst[a]);
			for (uint32_t k = lane; k < m; k += 64) {
				const uint32_t v = sp.step(steps, k + 1) >> 1;
				seg[b + k] = v;
				kal[b + k] = a;
				w += seq_off[v + 1] - seq_off[v];
			}
		}
		w = wave_sum(w);
		if (lane == 0)
			W[a] = w;
	}
}

// ---- sort, tier 1: a wave per bag of up to 64 keys
__global__ __launch_bounds__(Q_TPB) void k_cu_sort_t1(uint32_t n_al, const uint32_t *__restrict__ bag_off, const uint8_t *__restrict__ hand,
						      const uint32_t *__restrict__ seg, uint32_t *__restrict__ skey, uint16_t *__restrict__ sord)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	for (uint32_t a = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); a < n_al; a += waves) {
		const uint32_t b = bag_off[a], m = bag_off[a + 1] - b;
		if (!m || hand[a])
			continue;
		uint32_t key = lane < m ? seg[b + lane] : 0xFFFFFFFFu; // (a vertex index is below 2^32 - 1)
		for (uint32_t k = 2; k <= 64; k <<= 1)
			for (uint32_t j = k >> 1; j; j >>= 1) {
				const uint32_t other = __shfl_xor(key, (int)j, 64);
				const bool up = (lane & k) == 0, low = (lane & j) == 0;
				key = (low == up) ? min(key, other) : max(key, other);
			}
		const uint32_t prev = __shfl_up(key, 1, 64);
		const uint32_t start = wave_inclusive_max(lane && key != prev ? lane : 0u);
		if (lane < m) {
			skey[b + lane] = key;
			sord[b + lane] = (uint16_t)(lane - start);
		}
	}
}
// ---- sort, tier 2
__global__ void k_cu_key_flag(uint32_t nk, const uint32_t *__restrict__ kal, const uint8_t *__restrict__ hand, uint8_t *__restrict__ flag)
{
	for (uint32_t p = blockIdx.x * Q_TPB + threadIdx.x; p < nk; p += gridDim.x * Q_TPB)
		flag[p] = hand[kal[p]];
}
__global__ void k_cu_sort_key(uint32_t n2, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ of, uint32_t *__restrict__ key)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < n2; i += gridDim.x * Q_TPB)
		key[i] = of[perm[i]];
}
// head[i] = i where sorted key i begins a run of equal (allele, segment), else 0
__global__ void k_cu_heads(uint32_t n2, const uint32_t *__restrict__ cur, const uint32_t *__restrict__ seg, const uint32_t *__restrict__ kal,
			   uint32_t *__restrict__ head)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < n2; i += gridDim.x * Q_TPB) {
		const bool h = i && (kal[cur[i]] != kal[cur[i - 1]] || seg[cur[i]] != seg[cur[i - 1]]);
		head[i] = h ? i : 0;
	}
}
// sorted key i goes to the slot of rank i among the compacted slots: both lists hold the bags in allele order
__global__ void k_cu_place(uint32_t n2, const uint32_t *__restrict__ cur, const uint32_t *__restrict__ list0, const uint32_t *__restrict__ seg,
			   const uint32_t *__restrict__ head, const uint32_t *__restrict__ hmax, uint32_t *__restrict__ skey,
			   uint16_t *__restrict__ sord, uint32_t *__restrict__ bad)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < n2; i += gridDim.x * Q_TPB) {
		const uint32_t ord = i - max(head[i], hmax[i]), at = list0[i];
		skey[at] = seg[cur[i]];
		sord[at] = (uint16_t)min(ord, 0xFFFFu);
		if (ord > 0xFFFFu)
			atomicOr(bad, 1u);
	}
}

// ---- cluster: a wave per site
struct ClusterArgs {
	uint32_t n, T, no_bound;
	const uint32_t *aoff;
	const uint8_t *called;
	const uint32_t *bag_off, *skey;
	const uint16_t *sord;
	const uint64_t *W, *seq_off;
	uint32_t *clof, *reps, *ncl, *minsim; // reps: the representatives of site q at [aoff[q], aoff[q] + ncl[q])
	unsigned long long *cnt64;	      // [0] += pairs, [1] += pruned
};
__global__ __launch_bounds__(Q_TPB) void k_cu_cluster(ClusterArgs A)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	const uint32_t *__restrict__ skey = A.skey, *__restrict__ bag_off = A.bag_off;
	const uint16_t *__restrict__ sord = A.sord;
	const uint64_t *__restrict__ W = A.W, *__restrict__ seq_off = A.seq_off;
	for (uint32_t q = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); q < A.n; q += waves) {
		const uint32_t e0 = A.aoff[q], e1 = A.aoff[q + 1];
		if (!A.called[q] || e1 - e0 < 2) { // its exact alleles stay clusters of one
			for (uint32_t a = e0 + lane; a < e1; a += 64) {
				A.clof[a] = a - e0;
				A.reps[a] = a;
			}
			if (lane == 0) {
				A.ncl[q] = e1 - e0;
				A.minsim[q] = cluster::PPM;
			}
			continue;
		}
		uint32_t nc = 0, low = cluster::PPM;
		unsigned long long pairs = 0, pruned = 0;
		for (uint32_t a = e0; a < e1; a++) {
			const uint32_t ba = bag_off[a], ma = bag_off[a + 1] - ba;
			const uint64_t wa = W[a];
			bool has = false;
			cluster::Frac best{0, 0};
			uint32_t at = 0;
			for (uint32_t c = 0; c < nc; c++) {
				const uint32_t r = A.reps[e0 + c], br = bag_off[r], er = bag_off[r + 1];
				const uint64_t wr = W[r];
				pairs++;
				if (!A.no_bound && cluster::prunable(wa, wr, A.T, has, best)) {
					pruned++;
					continue;
				}
				uint64_t I = 0;
				for (uint32_t k0 = 0; k0 < ma; k0 += 64) {
					const uint32_t k = k0 + lane;
					if (k < ma) {
						const uint32_t s = skey[ba + k];
						if (cluster::key_counts(skey, br, er, s, (uint32_t)sord[ba + k]))
							I += seq_off[s + 1] - seq_off[s];
					}
				}
				I = wave_sum(I);
				const cluster::Frac f{I, wa + wr - I};
				if (cluster::similar(f, A.T) && (!has || cluster::better(f, best)))
					has = true, best = f, at = c;
			}
			if (!has) {
				if (lane == 0) {
					A.reps[e0 + nc] = a;
					A.clof[a] = nc;
				}
				__threadfence(); // (the wave reads its representatives back from memory)
				nc++;
			} else {
				if (lane == 0)
					A.clof[a] = at;
				low = min(low, cluster::sim_ppm(best));
			}
		}
		if (lane == 0) {
			A.ncl[q] = nc;
			A.minsim[q] = low;
			atomicAdd(A.cnt64, pairs);
			atomicAdd(A.cnt64 + 1, pruned);
		}
	}
}

// ---- close
__global__ void k_cu_close(uint32_t n_al, const uint32_t *__restrict__ aq, const uint32_t *__restrict__ aoff, const uint32_t *__restrict__ ncl,
			   const uint32_t *__restrict__ coff, const uint32_t *__restrict__ reps, const uint32_t *__restrict__ clof,
			   const uint32_t *__restrict__ afirst, uint32_t *__restrict__ crep, uint32_t *__restrict__ cfirst, uint32_t *__restrict__ csize)
{
	for (uint32_t x = blockIdx.x * Q_TPB + threadIdx.x; x < n_al; x += gridDim.x * Q_TPB) {
		const uint32_t q = aq[x], c = x - aoff[q];
		if (c < ncl[q]) {
			crep[coff[q] + c] = reps[x];
			cfirst[coff[q] + c] = afirst[reps[x]];
		}
		atomicAdd(csize + coff[q] + clof[x], 1u);
	}
}
__global__ void k_cu_trav_cluster(uint32_t R, const uint32_t *__restrict__ rq, const uint32_t *__restrict__ oa, const uint32_t *__restrict__ aoff,
				  const uint32_t *__restrict__ clof, uint32_t *__restrict__ oc)
{
	for (uint32_t t = blockIdx.x * Q_TPB + threadIdx.x; t < R; t += gridDim.x * Q_TPB)
		oc[t] = clof[aoff[rq[t]] + oa[t]];
}

ClusterClasses cluster_classes(povu_hip_ctx *ctx, const TravDevice &d, const uint8_t *called, uint32_t T, bool no_bound, bool force_tier2)
{
	hipStream_t s = ctx->stream;
	const uint32_t n = d.q.n, R = d.R, n_al = d.n_al;
	const size_t R1 = (size_t)R + 1, A1 = (size_t)n_al + 1, n1 = (size_t)n + 1, K1 = (size_t)d.n_steps + 1; // (the keys are allele steps)
	ClusterClasses c;
	uint32_t *cnt, *bag_off, *aq, *clof, *reps, *ncl, *seg, *kal, *skey, *list0, *cur, *nxt, *key, *kout, *head, *hmax, *words;
	uint16_t *sord;
	uint8_t *hand, *kflag;
	uint64_t *W;
	unsigned long long *cnt64;
	void *tmp;
	const size_t tmp_bytes = prim_tmp_bytes(std::max({A1, n1, K1}), true) + 256;
	carve(ctx->ns_cls, [&](Spans &take) {
		take(n1, c.coff, c.minsim);
		take(A1, c.crep, c.cfirst, c.csize);
		take(R1, c.oc);
	});
	carve(ctx->ns_ws, [&](Spans &take) {
		take(A1, cnt, bag_off, aq, clof, reps, hand, W);
		take(n1, ncl);
		take(K1, seg, kal, skey, sord, kflag, list0, cur, nxt, key, kout, head, hmax);
		take(8, words);
		take(4, cnt64);
		take(tmp_bytes, tmp);
	});
	HIP_CHECK(hipMemsetAsync(words, 0, 32, s));
	HIP_CHECK(hipMemsetAsync(cnt64, 0, 32, s));
	HIP_CHECK(hipMemsetAsync(ncl + n, 0, 4, s));
	HIP_CHECK(hipMemsetAsync(c.csize, 0, A1 * 4, s));
	if (!n_al) {
		HIP_CHECK(hipMemsetAsync(c.coff, 0, n1 * 4, s));
		if (n) {
			HIP_CHECK(hipMemsetAsync(c.minsim, 0, n1 * 4, s));
		}
		return c;
	}
	// ---- bags
	KLAUNCH(k_cu_count, dim3(stride_blocks(A1)), dim3(Q_TPB), 0, s, n_al, d.afirst, d.rq, d.rlen, d.aoff, called, force_tier2 ? 1u : 0u, aq, cnt, hand,
		cnt64);
	scan_exclusive_u32(cnt, bag_off, A1, tmp, tmp_bytes, s);
	const uint32_t nk = read_back(bag_off + n_al, s);
	c.n_keys = nk;
	KLAUNCH(k_cu_fill, dim3(wave_blocks(n_al)), dim3(Q_TPB), 0, s, n_al, d.afirst, d.rpos, d.rlen, ctx->path_steps, ctx->seq_off, bag_off, seg, kal, W);
	// ---- sort
	KLAUNCH(k_cu_sort_t1, dim3(wave_blocks(n_al)), dim3(Q_TPB), 0, s, n_al, bag_off, hand, seg, skey, sord);
	uint32_t n2 = 0;
	if (nk) {
		KLAUNCH(k_cu_key_flag, dim3(stride_blocks(nk)), dim3(Q_TPB), 0, s, nk, kal, hand, kflag);
		compact_flagged_u8(kflag, nk, list0, words, tmp, tmp_bytes, s);
		n2 = read_back(words, s);
	}
	if (n2) {
		HIP_CHECK(copy_async(cur, list0, (size_t)n2 * 4, hipMemcpyDeviceToDevice, s));
		LsdSort sort{cur, nxt, key, kout, n2, tmp, tmp_bytes, s};
		auto write_key = [&](int which, const uint32_t *perm, uint32_t *k) {
			KLAUNCH(k_cu_sort_key, dim3(stride_blocks(n2)), dim3(Q_TPB), 0, s, n2, perm, which ? kal : seg, k);
		};
		sort.pass(0, bits_for(ctx->g.V), write_key);
		sort.pass(1, bits_for(n_al), write_key);
		KLAUNCH(k_cu_heads, dim3(stride_blocks(n2)), dim3(Q_TPB), 0, s, n2, sort.cur, seg, kal, head);
		scan_exclusive_max_u32(head, hmax, n2, tmp, tmp_bytes, s);
		KLAUNCH(k_cu_place, dim3(stride_blocks(n2)), dim3(Q_TPB), 0, s, n2, sort.cur, list0, seg, head, hmax, skey, sord, words + 1);
		if (read_back(words + 1, s))
			throw HipError("clustered calls: an allele walks one segment more than 65 536 times: refused");
	}
	// ---- cluster
	if (n) {
		const ClusterArgs CA{n, T, no_bound ? 1u : 0u, d.aoff, called, bag_off, skey, sord, W, ctx->seq_off, clof, reps, ncl, c.minsim, cnt64};
		KLAUNCH(k_cu_cluster, dim3(wave_blocks(n)), dim3(Q_TPB), 0, s, CA);
	}
	// ---- close
	scan_exclusive_u32(ncl, c.coff, n1, tmp, tmp_bytes, s);
	KLAUNCH(k_cu_close, dim3(stride_blocks(n_al)), dim3(Q_TPB), 0, s, n_al, aq, d.aoff, ncl, c.coff, reps, clof, d.afirst, c.crep, c.cfirst, c.csize);
	if (R)
		KLAUNCH(k_cu_trav_cluster, dim3(stride_blocks(R)), dim3(Q_TPB), 0, s, R, d.rq, d.oa, d.aoff, clof, c.oc);
	unsigned long long h[4] = {0, 0, 0, 0};
	HIP_CHECK(copy_async(h, cnt64, 32, hipMemcpyDeviceToHost, s));
	c.n_cl = read_back(c.coff + n, s);
	c.n_pairs = h[0], c.n_pruned = h[1], c.n_sites = h[2], c.n_tier2 = h[3];
	return c;
}

} // namespace povu_hip
