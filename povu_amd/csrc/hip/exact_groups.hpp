// exact_groups.hpp -- grouping items of a query by exact equality behind a hash, and numbering the groups: the one copy that
// the alleles of the traversals (trav_kernels.hip: items = traversals, equal = the same step sequence), the classes of the
// nested calls (nest_kernels.hip: exact alleles, the same skeleton), the merged primitives (merge_kernels.hip: rows, the same
// written texts), the VCF comparison (vcfcmp_kernels.hip: (record, ALT) items, the same trimmed key) and the haplotype
// comparison (vcfhap_kernels.hip: items, the same edit) share.
//
// The items are stably sorted by (query, length, hash); every member of a run is compared with the run's first member by the
// caller's `same(a, b)`, and a run with a mismatch (a hash collision) is grouped exactly by one lane.  rep[k] of sorted
// position k is the sorted position of its group's first member -- the group's lowest item, the sort being stable.
#pragma once
#include "query_common.hpp"

#include <cstdlib>

namespace povu_hip
{

// bits of the 64-bit hash the groupings keep (test hook: fewer bits make collisions happen)
inline uint32_t hash_bits_hook()
{
	const char *e = std::getenv("POVU_HIP_TRAV_HASH_BITS");
	if (!e || !*e)
		return 64;
	const long b = std::strtol(e, nullptr, 10);
	return b < 1 ? 1 : b > 64 ? 64 : (uint32_t)b;
}
// the masks of the kept bits, high and low word
inline uint32_t hash_mask_hi(uint32_t hbits) { return hbits >= 64 ? 0xFFFFFFFFu : hbits > 32 ? (1u << (hbits - 32)) - 1 : 0u; }
inline uint32_t hash_mask_lo(uint32_t hbits) { return hbits >= 32 ? 0xFFFFFFFFu : (1u << hbits) - 1; }

__device__ __forceinline__ uint64_t mix64(uint64_t x) // splitmix64's finaliser
{
	x ^= x >> 30;
	x *= 0xbf58476d1ce4e5b9ull;
	x ^= x >> 27;
	x *= 0x94d049bb133111ebull;
	x ^= x >> 31;
	return x;
}
__device__ __forceinline__ uint64_t step_hash(uint32_t k, uint32_t side) { return mix64(((uint64_t)k << 32) | side); }

// sort keys through the current permutation: which = 0 hash low word, 1 hash high word, 2 length, 3 query
static __global__ void k_eg_sort_key(uint32_t R, int which, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ rhash,
				     const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ rq, uint32_t *__restrict__ key)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < R; k += gridDim.x * Q_TPB) {
		const uint32_t t = perm ? perm[k] : k;
		key[k] = which == 0 ? (uint32_t)rhash[t] : which == 1 ? (uint32_t)(rhash[t] >> 32) : which == 2 ? rlen[t] : rq[t];
	}
}

// run heads of the sorted order: (query, length, hash) differs from the previous one; mark[k] = k + 1 at a head
static __global__ void k_eg_heads(uint32_t R, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ rhash,
				  const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ rq, uint32_t *__restrict__ mark)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < R; k += gridDim.x * Q_TPB) {
		bool head = k == 0;
		if (!head) {
			const uint32_t a = perm[k], b = perm[k - 1];
			head = rq[a] != rq[b] || rlen[a] != rlen[b] || rhash[a] != rhash[b];
		}
		mark[k] = head ? k + 1 : 0;
	}
}

// every member of a run against the run's first member: rep[k] = the head, or NO_QUERY and the run flagged bad
template <class Same>
__global__ void k_eg_check(uint32_t R, Same same, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ hmax /* exclusive running max of mark */,
			   const uint32_t *__restrict__ mark, uint32_t *__restrict__ head, uint32_t *__restrict__ rep, uint8_t *__restrict__ bad)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < R; k += gridDim.x * Q_TPB) {
		const uint32_t h = max(hmax[k], mark[k]) - 1;
		head[k] = h;
		if (h == k) {
			rep[k] = k;
			continue;
		}
		if (same(perm[k], perm[h])) {
			rep[k] = h;
		} else {
			rep[k] = NO_QUERY;
			bad[h] = 1; // (cleared by a memset before the launch)
		}
	}
}

// a run with a mismatch, grouped exactly by one lane: every member either equals an earlier representative or becomes one
template <class Same>
__global__ void k_eg_regroup(uint32_t nb, const uint32_t *__restrict__ bad_heads, uint32_t R, Same same, const uint32_t *__restrict__ perm,
			     const uint32_t *__restrict__ head, uint32_t *__restrict__ rep, unsigned long long *__restrict__ splits)
{
	const uint32_t i = blockIdx.x * Q_TPB + threadIdx.x;
	if (i >= nb)
		return;
	const uint32_t h = bad_heads[i];
	uint32_t n_new = 0;
	for (uint32_t k = h + 1; k < R && head[k] == h; k++) {
		if (rep[k] == h)
			continue;
		const uint32_t a = perm[k];
		uint32_t r = k;
		for (uint32_t e = h + 1; e < k; e++)
			if (rep[e] == e && same(a, perm[e])) {
				r = e;
				break;
			}
		rep[k] = r;
		n_new += r == k;
	}
	atomicAdd(splits, (unsigned long long)n_new);
}

// first[t] = 1 when item t is the first of its group (its representative) and kept (keep: null, or a byte per item -- an item
// with a 0 there is the first of no group)
static __global__ void k_eg_first(uint32_t R, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ rep, const uint8_t *__restrict__ keep,
				  uint32_t *__restrict__ first)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < R; k += gridDim.x * Q_TPB)
		if (rep[k] == k && (!keep || keep[perm[k]]))
			first[perm[k]] = 1;
}
// group number of every item, from its group's first member (gidx: number_groups); NO_QUERY for an item that is not kept
[[maybe_unused]] static __global__ void k_eg_group_of(uint32_t n, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ rep, const uint32_t *__restrict__ gidx,
				     const uint8_t *__restrict__ keep, uint32_t *__restrict__ gid)
{
	for (uint64_t k = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; k < n; k += (uint64_t)gridDim.x * Q_TPB) {
		const uint32_t r = rep[k], i = perm[k];
		gid[i] = keep && !keep[i] ? NO_QUERY : gidx[perm[r < n ? r : k]];
	}
}

// the arrays of a grouping, R + 1 entries each (rbad: bytes); tmp: prim_tmp_bytes(R + 1, true)
struct GroupWs {
	uint32_t *pa, *pb, *key, *kout, *mark, *hmax, *head, *rep, *blist;
	uint8_t *rbad;
	void *tmp;
	size_t tmp_bytes;
};
// Groups the R > 0 items: gives the sorted order (w.pa or w.pb) and fills w.rep.  `count_word` (device) takes the number of
// runs with a mismatch; `splits` (device, cleared here) the groups split off by the exact comparison, copied to *h_splits
// when there are any (on its way to the host when this returns).
template <class Same>
const uint32_t *group_exact(uint32_t R, const uint32_t *rq, const uint32_t *rlen, const uint64_t *rhash, uint32_t hbits, unsigned len_bits,
			    unsigned query_bits, Same same, GroupWs &w, uint32_t *count_word, unsigned long long *splits, uint64_t *h_splits,
			    hipStream_t s)
{
	launch_iota(R, w.pa, s);
	LsdSort sort{w.pa, w.pb, w.key, w.kout, R, w.tmp, w.tmp_bytes, s};
	auto write_key = [&](int which, const uint32_t *perm, uint32_t *k) {
		KLAUNCH(k_eg_sort_key, dim3(stride_blocks(R)), dim3(Q_TPB), 0, s, R, which, perm, rhash, rlen, rq, k);
	};
	sort.pass(0, std::min(hbits, 32u), write_key);
	if (hbits > 32)
		sort.pass(1, hbits - 32, write_key);
	sort.pass(2, len_bits, write_key);
	sort.pass(3, query_bits, write_key);
	const uint32_t *sp = sort.cur;
	KLAUNCH(k_eg_heads, dim3(stride_blocks(R)), dim3(Q_TPB), 0, s, R, sp, rhash, rlen, rq, w.mark);
	scan_exclusive_max_u32(w.mark, w.hmax, R, w.tmp, w.tmp_bytes, s);
	HIP_CHECK(hipMemsetAsync(w.rbad, 0, (size_t)R + 1, s));
	HIP_CHECK(hipMemsetAsync(splits, 0, 8, s));
	KLAUNCH(k_eg_check<Same>, dim3(stride_blocks(R)), dim3(Q_TPB), 0, s, R, same, sp, w.hmax, w.mark, w.head, w.rep, w.rbad);
	compact_flagged_u8(w.rbad, R, w.blist, count_word, w.tmp, w.tmp_bytes, s);
	const uint32_t nb = read_back(count_word, s);
	if (nb) {
		KLAUNCH(k_eg_regroup<Same>, dim3(lane_blocks(nb)), dim3(Q_TPB), 0, s, nb, w.blist, R, same, sp, w.head, w.rep, splits);
		HIP_CHECK(copy_async(h_splits, splits, 8, hipMemcpyDeviceToHost, s));
	}
	return sp;
}

// Numbers the groups of group_exact's order `sp` and w.rep in the order of their first items: gidx[i] = the kept groups whose
// first item is below i, so gidx[first item] is a group's number and gidx[n] their count (on the device: the caller reads it
// back).  firstf, gidx: n + 1 entries; tmp: prim_tmp_bytes(n + 1, false)
inline void number_groups(uint32_t n, const uint32_t *sp, const uint32_t *rep, uint32_t *firstf, uint32_t *gidx, const uint8_t *keep, void *tmp,
			  size_t tmp_bytes, hipStream_t s)
{
	HIP_CHECK(hipMemsetAsync(firstf, 0, ((size_t)n + 1) * 4, s));
	KLAUNCH(k_eg_first, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, sp, rep, keep, firstf);
	scan_exclusive_u32(firstf, gidx, (size_t)n + 1, tmp, tmp_bytes, s);
}

} // namespace povu_hip
