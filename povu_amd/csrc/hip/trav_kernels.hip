// trav_kernels.hip -- the traversals of every flubble of a forest by the paths of the graph (povu_hip_paths_upload,
// povu_hip_forest_traversals; include/povu_hip.h).
//
// The definition is this project's own ("Flubble traversals"; restated in tests/traversals_ref.py).  A query
// (S, Z) is a PVST vertex, numbered as the walks number them (query_common.hpp).  Every path step equal to S starts a forward
// scan, every step equal to flip(Z) a reverse scan; a scan ends at the next step on either boundary segment and is a
// traversal when that step is Z (flip(S)) within max_steps steps.  Because a scan stops at the next occurrence of either
// boundary segment, the scans of one query and direction never overlap along a path: the work is the path steps times the
// nesting depth, plus max_steps per scan that does not close.
//
// A step is one word, `side`: vertex index << 1 | 1 for '<' -- the side it enters its segment by, as in the walks -- so
// flip(x) = x ^ 1.  Shape of a call:
//   boundary table  a CSR over the 2 V step values listing (query, role) -- role 0: S starts a forward scan, 1: flip(Z) a
//                   reverse scan -- built with one stable sort of the 2 n keys (entries of a step in (query, role) order);
//   start tasks     a count pass over every path step (per tile of T_TILE steps), an exclusive scan of the tile counts, an
//                   emit pass that writes the tasks in (path, position) order; a stable sort by query groups them, keeping
//                   that order within a query;
//   scans           tier 1: one lane per task, up to T1_STEPS steps; tier 2: one wave per task handed over, 64 steps a ballot
//                   (taken from an atomic counter: a long structural variant does not hold up a wave of SNPs).  Both give
//                   the same length and the same 64-bit hash of the S -> Z sequence: the sum over k of mix(k, step k);
//   dedup           the closed tasks (the traversals, in (query, path, position) order) are stably sorted by (query, length,
//                   hash); every member of a run is compared step by step with the run's first member, and a run with a
//                   mismatch (a hash collision) is grouped exactly by one lane; an allele is numbered by the scan of the
//                   "first of its group" flags in traversal order, and its steps are copied once from that traversal.
#include "query_common.hpp"

namespace povu_hip
{

static constexpr int T_TPB = 256;
static constexpr uint32_t T_PER_LANE = 16;		 // steps per lane of the start-task passes
static constexpr uint32_t T_TILE = T_TPB * T_PER_LANE; // steps per workgroup of the start-task passes
static constexpr uint32_t T1_STEPS = 64;		 // steps tier 1 looks at before it hands a scan over
static constexpr uint64_t ROLE_BIT = 1ull << 63;	 // role of a task, kept in the top bit of its position
static constexpr uint8_t TS_LONG = POVU_HIP_TRAV_LONG, TS_STRAY = POVU_HIP_TRAV_STRAY, TS_OPEN = POVU_HIP_TRAV_OPEN;

static inline unsigned tblk(size_t n) { return (unsigned)((n + T_TPB - 1) / T_TPB); }
static inline unsigned tgrid(size_t n) { return (unsigned)std::min<size_t>(tblk(n), 65536); } // (grid-stride kernels)

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

// step k (S -> Z) of the traversal that occupies path words [pos, pos + len), read backwards and flipped when reverse
__device__ __forceinline__ uint32_t trav_step(const uint32_t *__restrict__ steps, uint64_t pos, uint32_t len, bool rev, uint32_t k)
{
	return rev ? steps[pos + len - 1 - k] ^ 1u : steps[pos + k];
}

// path of global step `x`: the last k with off[k] <= x
__device__ __forceinline__ uint32_t path_of(const uint64_t *__restrict__ off, uint32_t n_paths, uint64_t x)
{
	uint32_t lo = 0, hi = n_paths;
	while (hi - lo > 1) {
		const uint32_t mid = (lo + hi) >> 1;
		if (off[mid] <= x)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

// ---- paths: segment ids -> step words (the ids were copied into `steps`, mapped in place); the lowest step whose id the
// graph does not have is kept in *bad
__global__ void k_tr_map_steps(uint64_t N, uint32_t *__restrict__ steps, const uint8_t *__restrict__ rev,
			       const uint32_t *__restrict__ vid, uint32_t V, unsigned long long *__restrict__ bad)
{
	for (uint64_t i = (uint64_t)blockIdx.x * T_TPB + threadIdx.x; i < N; i += (uint64_t)gridDim.x * T_TPB) {
		const uint32_t v = find_vertex(vid, V, steps[i]);
		if (v == NO_QUERY) {
			atomicMin(bad, (unsigned long long)i);
			steps[i] = 0;
			continue;
		}
		steps[i] = (v << 1) | (rev[i] & 1u);
	}
}

// ---- the boundary table: keys of (query, role), one per role (2 V: none)
__global__ void k_tr_keys(uint32_t n, uint32_t nS, const uint32_t *__restrict__ ys, const uint32_t *__restrict__ yz,
			  uint32_t *__restrict__ key, uint32_t *__restrict__ val, uint32_t *__restrict__ cnt)
{
	const uint32_t q = blockIdx.x * T_TPB + threadIdx.x;
	if (q >= n)
		return;
	const bool none = ys[q] == NO_QUERY;
	const uint32_t k0 = none ? nS : ys[q], k1 = none ? nS : (yz[q] ^ 1u);
	key[2 * q] = k0;
	key[2 * q + 1] = k1;
	val[2 * q] = 2 * q;
	val[2 * q + 1] = 2 * q + 1;
	if (!none) {
		atomicAdd(&cnt[k0], 1u);
		atomicAdd(&cnt[k1], 1u);
	}
}

// ---- start tasks.  Lane t of a workgroup looks at steps base + k T_TPB + t, k < T_PER_LANE (coalesced); the emit pass
// ranks them in step order with a workgroup scan per k.
__device__ __forceinline__ uint32_t wg_exclusive_scan(uint32_t v, uint32_t &total, uint32_t *lds /* [T_TPB / 64 + 1] */)
{
	const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
	uint32_t x = v;
	for (int o = 1; o < 64; o <<= 1) {
		const uint32_t y = __shfl_up(x, o);
		if ((int)lane >= o)
			x += y;
	}
	if (lane == 63)
		lds[wv] = x;
	__syncthreads();
	uint32_t before = 0, all = 0;
	for (uint32_t w = 0; w < T_TPB / 64; w++) {
		const uint32_t c = lds[w];
		before += w < wv ? c : 0;
		all += c;
	}
	__syncthreads();
	total = all;
	return before + x - v;
}

__global__ __launch_bounds__(T_TPB) void k_tr_count(uint64_t N, const uint32_t *__restrict__ steps, const uint32_t *__restrict__ boff,
						    uint32_t *__restrict__ tile_cnt)
{
	__shared__ uint32_t lds[T_TPB / 64 + 1];
	const uint64_t base = (uint64_t)blockIdx.x * T_TILE;
	uint32_t c = 0;
	for (uint32_t k = 0; k < T_PER_LANE; k++) {
		const uint64_t i = base + (uint64_t)k * T_TPB + threadIdx.x;
		if (i < N) {
			const uint32_t x = steps[i];
			c += boff[x + 1] - boff[x];
		}
	}
	uint32_t total;
	(void)wg_exclusive_scan(c, total, lds);
	if (threadIdx.x == 0)
		tile_cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(T_TPB) void k_tr_emit(uint64_t N, const uint32_t *__restrict__ steps, const uint32_t *__restrict__ boff,
						   const uint32_t *__restrict__ bval, const uint32_t *__restrict__ tile_off,
						   uint64_t *__restrict__ tpos, uint32_t *__restrict__ tkey)
{
	__shared__ uint32_t lds[T_TPB / 64 + 1];
	const uint64_t base = (uint64_t)blockIdx.x * T_TILE;
	uint32_t at = tile_off[blockIdx.x];
	for (uint32_t k = 0; k < T_PER_LANE; k++) {
		const uint64_t i = base + (uint64_t)k * T_TPB + threadIdx.x;
		uint32_t b = 0, e = 0;
		if (i < N) {
			const uint32_t x = steps[i];
			b = boff[x], e = boff[x + 1];
		}
		uint32_t total;
		const uint32_t mine = at + wg_exclusive_scan(e - b, total, lds);
		for (uint32_t j = b; j < e; j++) {
			const uint32_t qr = bval[j];
			tpos[mine + j - b] = i | ((qr & 1u) ? ROLE_BIT : 0ull);
			tkey[mine + j - b] = qr >> 1;
		}
		at += total;
	}
}

__global__ void k_tr_iota(uint32_t n, uint32_t *__restrict__ a)
{
	for (uint32_t i = blockIdx.x * T_TPB + threadIdx.x; i < n; i += gridDim.x * T_TPB)
		a[i] = i;
}

// out[k] = in[perm[k]] (u64 / u32)
__global__ void k_tr_gather64(uint32_t n, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ in, uint64_t *__restrict__ out)
{
	for (uint32_t k = blockIdx.x * T_TPB + threadIdx.x; k < n; k += gridDim.x * T_TPB)
		out[k] = in[perm[k]];
}

// ---- the scans
struct ScanArgs {
	const uint32_t *steps;
	const uint64_t *path_off;
	uint32_t n_paths;
	const uint32_t *ys, *yz;
	uint32_t max_steps, hash_mask_hi, hash_mask_lo; // (the hash keeps hash_mask_hi:lo of its bits: POVU_HIP_TRAV_HASH_BITS)
};
struct ScanOut {
	uint32_t *len; // 0: no traversal
	uint64_t *hash;
	uint32_t *status; // [n] bits of the query
};

// one task's query, role, start, the end of its window (exclusive) and whether the window ends with the path
struct TaskView {
	uint32_t q, a, z, close;
	bool rev;
	uint64_t pos, lim;
	bool lim_is_end;
};
__device__ __forceinline__ TaskView task_view(const ScanArgs &A, uint32_t q, uint64_t tp)
{
	TaskView t;
	t.q = q;
	t.rev = (tp & ROLE_BIT) != 0;
	t.pos = tp & ~ROLE_BIT;
	const uint32_t ys = A.ys[q], yz = A.yz[q];
	t.a = ys >> 1;
	t.z = yz >> 1;
	t.close = t.rev ? ys ^ 1u : yz;
	const uint64_t end = A.path_off[path_of(A.path_off, A.n_paths, t.pos) + 1];
	const uint64_t win = t.pos + A.max_steps; // position pos + max_steps existing: LONG
	t.lim_is_end = end <= win;
	t.lim = t.lim_is_end ? end : win;
	return t;
}

__device__ __forceinline__ uint64_t keep_bits(const ScanArgs &A, uint64_t h)
{
	return h & (((uint64_t)A.hash_mask_hi << 32) | A.hash_mask_lo);
}

// tier 1: one lane per task (sorted order); a scan not decided within T1_STEPS steps is handed over
__global__ __launch_bounds__(T_TPB) void k_tr_t1(uint32_t T, ScanArgs A, const uint32_t *__restrict__ tq, const uint64_t *__restrict__ tpos,
						 uint32_t force2, ScanOut O, uint8_t *__restrict__ handover)
{
	const uint32_t k = blockIdx.x * T_TPB + threadIdx.x;
	if (k >= T)
		return;
	O.len[k] = 0;
	O.hash[k] = 0;
	if (force2) {
		handover[k] = 1;
		return;
	}
	const TaskView t = task_view(A, tq[k], tpos[k]);
	uint64_t j = t.pos + 1;
	const uint64_t stop = t.pos + 1 + T1_STEPS;
	bool found = false;
	for (; j < t.lim && j < stop; j++) {
		const uint32_t v = A.steps[j] >> 1;
		if (v == t.a || v == t.z) {
			found = true;
			break;
		}
	}
	if (!found && j < t.lim) { // T1_STEPS steps looked at, the window goes on
		handover[k] = 1;
		return;
	}
	handover[k] = 0;
	if (!found) {
		atomicOr(&O.status[t.q], t.lim_is_end ? TS_OPEN : TS_LONG);
		return;
	}
	if (A.steps[j] != t.close) {
		atomicOr(&O.status[t.q], TS_STRAY);
		return;
	}
	const uint32_t len = (uint32_t)(j - t.pos + 1);
	uint64_t h = 0;
	for (uint32_t i = 0; i < len; i++)
		h += step_hash(i, trav_step(A.steps, t.pos, len, t.rev, i));
	O.len[k] = len;
	O.hash[k] = keep_bits(A, h);
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t x)
{
	for (int o = 32; o > 0; o >>= 1)
		x += __shfl_xor(x, o);
	return x;
}

// tier 2: one wave per task of `list`, every wave taking its next task from *next (zeroed before the launch); 64 steps a
// ballot to find the end, then 64 steps a pass to hash the sequence
__global__ __launch_bounds__(T_TPB) void k_tr_t2(const uint32_t *__restrict__ list, uint32_t n2, uint32_t *__restrict__ next, ScanArgs A,
						 const uint32_t *__restrict__ tq, const uint64_t *__restrict__ tpos, ScanOut O)
{
	const uint32_t lane = threadIdx.x & 63u;
	for (uint32_t it = 0; it < n2; it++) { // (a wave takes at most all n2 tasks: the loop is bounded whatever the counter says)
		uint32_t w = atomicAdd(next, lane == 0 ? 1u : 0u);
		w = __shfl(w, 0);
		if (w >= n2)
			break;
		const uint32_t k = list[w];
		const TaskView t = task_view(A, tq[k], tpos[k]);
		uint64_t j = ~0ull;
		for (uint64_t base = t.pos + 1; base < t.lim; base += 64) {
			const uint64_t x = base + lane;
			bool hit = false;
			if (x < t.lim) {
				const uint32_t v = A.steps[x] >> 1;
				hit = v == t.a || v == t.z;
			}
			const unsigned long long m = __ballot(hit);
			if (m) {
				j = base + (uint64_t)(__ffsll((long long)m) - 1);
				break;
			}
		}
		if (j == ~0ull) {
			if (lane == 0)
				atomicOr(&O.status[t.q], t.lim_is_end ? TS_OPEN : TS_LONG);
			continue;
		}
		if (A.steps[j] != t.close) {
			if (lane == 0)
				atomicOr(&O.status[t.q], TS_STRAY);
			continue;
		}
		const uint32_t len = (uint32_t)(j - t.pos + 1);
		uint64_t h = 0;
		for (uint32_t i = lane; i < len; i += 64)
			h += step_hash(i, trav_step(A.steps, t.pos, len, t.rev, i));
		h = wave_sum64(h);
		if (lane == 0) {
			O.len[k] = len;
			O.hash[k] = keep_bits(A, h);
		}
	}
}

__global__ void k_tr_closed(uint32_t T, const uint32_t *__restrict__ len, uint8_t *__restrict__ closed)
{
	for (uint32_t k = blockIdx.x * T_TPB + threadIdx.x; k < T; k += gridDim.x * T_TPB)
		closed[k] = len[k] != 0;
}

// the traversals (closed tasks, `list` in sorted task order): their query, position (with role), length and hash
__global__ void k_tr_trav_fields(uint32_t R, const uint32_t *__restrict__ list, const uint32_t *__restrict__ tq,
				 const uint64_t *__restrict__ tpos, const uint32_t *__restrict__ len, const uint64_t *__restrict__ hash,
				 uint32_t *__restrict__ rq, uint64_t *__restrict__ rpos, uint32_t *__restrict__ rlen,
				 uint64_t *__restrict__ rhash)
{
	for (uint32_t t = blockIdx.x * T_TPB + threadIdx.x; t < R; t += gridDim.x * T_TPB) {
		const uint32_t k = list[t];
		rq[t] = tq[k];
		rpos[t] = tpos[k];
		rlen[t] = len[k];
		rhash[t] = hash[k];
	}
}

// trav_off[q] = first traversal of query >= q (the traversals are grouped by query), q in [0, n]
__global__ void k_tr_query_off(uint32_t n, uint32_t R, const uint32_t *__restrict__ rq, uint32_t *__restrict__ off)
{
	const uint32_t q = blockIdx.x * T_TPB + threadIdx.x;
	if (q > n)
		return;
	uint32_t lo = 0, hi = R;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (rq[mid] < q)
			lo = mid + 1;
		else
			hi = mid;
	}
	off[q] = lo;
}

// sort keys through the current permutation: which = 0 hash low word, 1 hash high word, 2 length, 3 query
__global__ void k_tr_sort_key(uint32_t R, int which, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ rhash,
			      const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ rq, uint32_t *__restrict__ key)
{
	for (uint32_t k = blockIdx.x * T_TPB + threadIdx.x; k < R; k += gridDim.x * T_TPB) {
		const uint32_t t = perm ? perm[k] : k;
		key[k] = which == 0 ? (uint32_t)rhash[t] : which == 1 ? (uint32_t)(rhash[t] >> 32) : which == 2 ? rlen[t] : rq[t];
	}
}

// run heads of the sorted order: (query, length, hash) differs from the previous one; mark[k] = k + 1 at a head
__global__ void k_tr_heads(uint32_t R, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ rhash,
			   const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ rq, uint32_t *__restrict__ mark)
{
	for (uint32_t k = blockIdx.x * T_TPB + threadIdx.x; k < R; k += gridDim.x * T_TPB) {
		bool head = k == 0;
		if (!head) {
			const uint32_t a = perm[k], b = perm[k - 1];
			head = rq[a] != rq[b] || rlen[a] != rlen[b] || rhash[a] != rhash[b];
		}
		mark[k] = head ? k + 1 : 0;
	}
}

__device__ __forceinline__ bool same_sequence(const uint32_t *__restrict__ steps, uint64_t pa, uint64_t pb, uint32_t len)
{
	const bool ra = (pa & ROLE_BIT) != 0, rb = (pb & ROLE_BIT) != 0;
	pa &= ~ROLE_BIT;
	pb &= ~ROLE_BIT;
	for (uint32_t i = 0; i < len; i++)
		if (trav_step(steps, pa, len, ra, i) != trav_step(steps, pb, len, rb, i))
			return false;
	return true;
}

// every member of a run against the run's first member: rep[k] = the head, or NO_QUERY and the run flagged bad
__global__ void k_tr_check(uint32_t R, const uint32_t *__restrict__ steps, const uint32_t *__restrict__ perm,
			   const uint32_t *__restrict__ hmax /* exclusive running max of mark */, const uint32_t *__restrict__ mark,
			   const uint64_t *__restrict__ rpos, const uint32_t *__restrict__ rlen, uint32_t *__restrict__ head,
			   uint32_t *__restrict__ rep, uint8_t *__restrict__ bad)
{
	for (uint32_t k = blockIdx.x * T_TPB + threadIdx.x; k < R; k += gridDim.x * T_TPB) {
		const uint32_t h = max(hmax[k], mark[k]) - 1;
		head[k] = h;
		if (h == k) {
			rep[k] = k;
			continue;
		}
		const uint32_t a = perm[k], b = perm[h];
		if (same_sequence(steps, rpos[a], rpos[b], rlen[a])) {
			rep[k] = h;
		} else {
			rep[k] = NO_QUERY;
			bad[h] = 1; // (cleared by a memset before the launch)
		}
	}
}

// a run with a mismatch, grouped exactly by one lane: every member either equals an earlier representative or becomes one
__global__ void k_tr_regroup(uint32_t nb, const uint32_t *__restrict__ bad_heads, uint32_t R, const uint32_t *__restrict__ steps,
			     const uint32_t *__restrict__ perm, const uint32_t *__restrict__ head, const uint64_t *__restrict__ rpos,
			     const uint32_t *__restrict__ rlen, uint32_t *__restrict__ rep, unsigned long long *__restrict__ splits)
{
	const uint32_t i = blockIdx.x * T_TPB + threadIdx.x;
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
			if (rep[e] == e && same_sequence(steps, rpos[a], rpos[perm[e]], rlen[a])) {
				r = e;
				break;
			}
		rep[k] = r;
		n_new += r == k;
	}
	atomicAdd(splits, (unsigned long long)n_new);
}

// first[t] = 1 when traversal t is the first of its group (its representative)
__global__ void k_tr_first(uint32_t R, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ rep, uint32_t *__restrict__ first)
{
	for (uint32_t k = blockIdx.x * T_TPB + threadIdx.x; k < R; k += gridDim.x * T_TPB)
		if (rep[k] == k)
			first[perm[k]] = 1;
}

// allele of every traversal (global numbering: aidx of its group's first traversal); the first traversal of every allele
__global__ void k_tr_allele(uint32_t R, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ rep, const uint32_t *__restrict__ aidx,
			    const uint32_t *__restrict__ rlen, uint32_t *__restrict__ rallele, uint32_t *__restrict__ afirst,
			    uint32_t *__restrict__ alen)
{
	for (uint32_t k = blockIdx.x * T_TPB + threadIdx.x; k < R; k += gridDim.x * T_TPB) {
		const uint32_t t = perm[k], f = perm[rep[k]], a = aidx[f];
		rallele[t] = a;
		if (rep[k] == k) {
			afirst[a] = t;
			alen[a] = rlen[t];
		}
	}
}

// per traversal: path, first / last step within the path, reverse, allele within its query
__global__ void k_tr_out(uint32_t R, const uint64_t *__restrict__ path_off, uint32_t n_paths, const uint32_t *__restrict__ rq,
			 const uint64_t *__restrict__ rpos, const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ rallele,
			 const uint32_t *__restrict__ aidx, const uint32_t *__restrict__ toff, uint32_t *__restrict__ o_path,
			 uint32_t *__restrict__ o_first, uint32_t *__restrict__ o_last, uint32_t *__restrict__ o_allele,
			 uint8_t *__restrict__ o_rev)
{
	for (uint32_t t = blockIdx.x * T_TPB + threadIdx.x; t < R; t += gridDim.x * T_TPB) {
		const uint64_t pos = rpos[t] & ~ROLE_BIT;
		const uint32_t p = path_of(path_off, n_paths, pos);
		o_path[t] = p;
		o_first[t] = (uint32_t)(pos - path_off[p]);
		o_last[t] = (uint32_t)(pos - path_off[p]) + rlen[t] - 1;
		o_rev[t] = (rpos[t] & ROLE_BIT) ? 1 : 0;
		o_allele[t] = rallele[t] - aidx[toff[rq[t]]];
	}
}

// allele_off[q] = aidx[trav_off[q]]
__global__ void k_tr_allele_off(uint32_t n, const uint32_t *__restrict__ toff, const uint32_t *__restrict__ aidx, uint32_t *__restrict__ aoff)
{
	const uint32_t q = blockIdx.x * T_TPB + threadIdx.x;
	if (q <= n)
		aoff[q] = aidx[toff[q]];
}

// the steps of every allele (S -> Z), one wave per allele
__global__ __launch_bounds__(T_TPB) void k_tr_allele_steps(uint32_t n_al, const uint32_t *__restrict__ steps, const uint32_t *__restrict__ vid,
							   const uint32_t *__restrict__ afirst, const uint64_t *__restrict__ rpos,
							   const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ soff,
							   uint32_t *__restrict__ o_id, uint8_t *__restrict__ o_or)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (T_TPB / 64);
	for (uint32_t a = blockIdx.x * (T_TPB / 64) + (threadIdx.x >> 6); a < n_al; a += waves) {
		const uint32_t t = afirst[a], len = rlen[t], at = soff[a];
		const uint64_t p = rpos[t];
		const bool rev = (p & ROLE_BIT) != 0;
		for (uint32_t i = lane; i < len; i += 64) {
			const uint32_t x = trav_step(steps, p & ~ROLE_BIT, len, rev, i);
			o_id[at + i] = vid[x >> 1];
			o_or[at + i] = (uint8_t)(x & 1u);
		}
	}
}

static void check_32(uint64_t v, const char *what)
{
	if (v >= 0xFFFFFFFFull)
		throw HipError(std::string("the traversals need ") + std::to_string(v) + " " + what +
			       ": 2^32 or more are refused for now (the scans and sorts here are 32-bit)");
}

static uint32_t hash_bits_hook()
{
	const char *e = std::getenv("POVU_HIP_TRAV_HASH_BITS"); // (test hook: fewer bits make collisions happen)
	if (!e || !*e)
		return 64;
	const long b = std::strtol(e, nullptr, 10);
	return b < 1 ? 1 : b > 64 ? 64 : (uint32_t)b;
}

} // namespace povu_hip

// ---- C ABI

extern "C" int povu_hip_paths_upload(povu_hip_ctx *ctx, uint32_t n_paths, const uint64_t *step_off, const uint32_t *step_id,
				     const uint8_t *step_rev, char *err, size_t errlen)
{
	return guarded_call(ctx, err, errlen, 1, [&] {
		if (!ctx)
			throw HipError("null context");
		if (!ctx->g.block)
			throw HipError("paths need a resident graph (povu_hip_graph_upload first)");
		if (!step_off)
			throw HipError("null step offsets");
		ctx->paths_valid = false;
		const ResidentGraph &g = ctx->g;
		if (step_off[0] != 0)
			throw HipError("step_off[0] must be 0");
		for (uint32_t k = 0; k < n_paths; k++) {
			if (step_off[k + 1] < step_off[k])
				throw HipError("step offsets of path " + std::to_string(k) + " decrease");
			if (step_off[k + 1] - step_off[k] >= (1ull << 32))
				throw HipError("path " + std::to_string(k) + " has " + std::to_string(step_off[k + 1] - step_off[k]) +
					       " steps: 2^32 or more are refused");
		}
		const uint64_t N = step_off[n_paths];
		if (N && (!step_id || !step_rev))
			throw HipError("null step arrays");
		if ((uint64_t)g.V * 2 >= 0xFFFFFFFFull)
			throw HipError("graph too large for one-word path steps");
		HIP_CHECK(hipSetDevice(ctx->device));
		ctx->wait_tail();
		hipStream_t s = ctx->stream;
		carve(
			ctx->paths_buf,
			[&](Spans &take) {
				take(N + 4, ctx->path_steps);
				take((size_t)n_paths + 1, ctx->path_off);
			},
			false);
		uint8_t *rev;
		uint32_t *words;
		unsigned long long *bad;
		carve(ctx->tr_ws, [&](Spans &take) {
			take(N + 1, rev);
			take(4, words);
			take(1, bad);
		});
		HIP_CHECK(hipMemsetAsync(words, 0, 16, s));
		HIP_CHECK(hipMemsetAsync(bad, 0xFF, 8, s));
		HIP_CHECK(copy_async(ctx->path_off, step_off, ((size_t)n_paths + 1) * 8, hipMemcpyHostToDevice, s));
		if (N) {
			HIP_CHECK(copy_async(ctx->path_steps, step_id, N * 4, hipMemcpyHostToDevice, s));
			HIP_CHECK(copy_async(rev, step_rev, N, hipMemcpyHostToDevice, s));
		}
		launch_vid_ascending(g.V, g.vid, words, s);
		if (N)
			KLAUNCH(k_tr_map_steps, dim3(tgrid(N)), dim3(T_TPB), 0, s, N, ctx->path_steps, rev, g.vid, g.V, bad);
		uint32_t hw[4] = {0};
		uint64_t hb = 0;
		HIP_CHECK(copy_async(hw, words, 16, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(&hb, bad, 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		query_refusals(hw[0], "paths");
		if (hb != ~0ull) {
			const uint32_t k = (uint32_t)(std::upper_bound(step_off, step_off + n_paths + 1, hb) - step_off) - 1;
			throw HipError("path " + std::to_string(k) + " step " + std::to_string(hb - step_off[k]) + ": segment " +
				       std::to_string(step_id[hb]) + " is not in the resident graph");
		}
		ctx->n_paths = n_paths;
		ctx->n_path_steps = N;
		ctx->paths_gen = g.gen;
		ctx->paths_valid = true;
		return 0;
	});
}
namespace
{
struct TraversalsOwner {
	povu_hip_traversals view{}; // first member: the owner is recovered from it in povu_hip_traversals_free
	std::vector<uint64_t> trav_off, allele_off, step_off;
	std::vector<uint8_t> status;
	PinnedVec<uint32_t> path, first, last, allele, step_id;
	PinnedVec<uint8_t> reverse, step_or;
};
} // namespace

namespace povu_hip
{
TravDevice trav_pipeline(povu_hip_ctx *ctx, const QueryFrontFn &front, const povu_hip_trav_opts *opts, CallTimer &timer)
{
	if (!ctx->paths_valid || ctx->paths_gen != ctx->g.gen)
		throw HipError("no paths are resident for the graph now uploaded (povu_hip_paths_upload after povu_hip_graph_upload)");
	uint32_t max_steps = 65536, flags = 0;
	if (opts) {
		if (opts->max_steps == 1)
			throw HipError("max_steps must be at least 2");
		if (opts->max_steps)
			max_steps = opts->max_steps;
		flags = opts->flags;
	}
	const uint32_t hbits = hash_bits_hook();
	const ResidentGraph &g = ctx->g;
	hipStream_t s = ctx->stream;
	const uint64_t N = ctx->n_path_steps;
	const uint32_t P = ctx->n_paths, nS = 2 * g.V;
	const uint64_t n_tiles = (N + T_TILE - 1) / T_TILE;
	check_32(n_tiles + 1, "start-task tiles");

	// ---- phase A: queries, the boundary table, tile counts
	uint32_t *qstatus, *bkey, *bval, *bkey2, *bval2, *bcnt, *boff, *tile_cnt, *tile_off;
	unsigned long long *tot;
	void *sort_tmp_a, *scan_tmp_a;
	size_t sort_a = 0;
	const size_t scan_a = scan_tmp_bytes(std::max<size_t>((size_t)nS + 1, n_tiles + 1)) + 256;
	const QueryFront q = front(timer, [&](Spans &take, uint32_t n) {
		const size_t n2q = 2 * (size_t)n + 1;
		sort_a = sort_tmp_bytes(n2q) + 256;
		take((size_t)n + 1, qstatus);
		take(n2q, bkey, bval, bkey2, bval2);
		take((size_t)nS + 1, bcnt, boff);
		take(n_tiles + 1, tile_cnt, tile_off);
		take(2, tot);
		take(sort_a, sort_tmp_a);
		take(scan_a, scan_tmp_a);
	});
	const uint32_t n = q.n, *ys = q.ys, *yz = q.yz;
	uint32_t *words = q.words;
	const size_t n1 = (size_t)n + 1;
	HIP_CHECK(hipMemsetAsync(qstatus, 0, n1 * 4, s));
	HIP_CHECK(hipMemsetAsync(bcnt, 0, ((size_t)nS + 1) * 4, s));
	uint32_t hw[8] = {0};
	HIP_CHECK(copy_async(hw, words, 32, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	query_refusals(hw[0], "traversals");
	if (n) {
		KLAUNCH(k_tr_keys, dim3(tblk(n)), dim3(T_TPB), 0, s, n, nS, ys, yz, bkey, bval, bcnt);
		sort_pairs_u32(bkey, bkey2, bval, bval2, 2 * (size_t)n, bits_for(nS), sort_tmp_a, sort_a, s);
	}
	scan_exclusive_u32(bcnt, boff, (size_t)nS + 1, scan_tmp_a, scan_a, s);

	// ---- start tasks: count per tile, scan, emit
	if (n_tiles)
		KLAUNCH(k_tr_count, dim3((unsigned)n_tiles), dim3(T_TPB), 0, s, N, ctx->path_steps, boff, tile_cnt);
	HIP_CHECK(hipMemsetAsync(tile_cnt + n_tiles, 0, 4, s));
	uint64_t T64 = 0;
	totals_u32(tile_cnt, nullptr, n_tiles, tot, &T64, s);
	check_32(T64, "scan tasks");
	const uint32_t T = (uint32_t)T64;
	scan_exclusive_u32(tile_cnt, tile_off, n_tiles + 1, scan_tmp_a, scan_a, s);

	// ---- phase B: the tasks, sorted by query, and their scans
	const size_t T1 = (size_t)T + 1;
	const size_t sort_b = sort_tmp_bytes(T1) + 256, comp_b = compact_tmp_bytes(T1) + 256;
	uint64_t *tpos, *spos, *thash;
	uint32_t *tkey, *tval, *sq, *perm, *tlen, *list;
	uint8_t *handover, *closed;
	void *sort_tmp_b, *comp_tmp_b;
	carve(ctx->tr_task, [&](Spans &take) {
		take(T1, tpos, spos, thash, tkey, tval, sq, perm, tlen, list, handover, closed);
		take(sort_b, sort_tmp_b);
		take(comp_b, comp_tmp_b);
	});
	uint32_t n2 = 0, R = 0;
	ScanArgs SA{ctx->path_steps, ctx->path_off, P, ys, yz, max_steps, hbits >= 64 ? 0xFFFFFFFFu : hbits > 32 ? (1u << (hbits - 32)) - 1 : 0u,
		    hbits >= 32 ? 0xFFFFFFFFu : (1u << hbits) - 1};
	ScanOut SO{tlen, thash, qstatus};
	if (T) {
		KLAUNCH(k_tr_emit, dim3((unsigned)n_tiles), dim3(T_TPB), 0, s, N, ctx->path_steps, boff, bval2, tile_off, tpos, tkey);
		KLAUNCH(k_tr_iota, dim3(tgrid(T)), dim3(T_TPB), 0, s, T, tval);
		sort_pairs_u32(tkey, sq, tval, perm, T, bits_for(n), sort_tmp_b, sort_b, s);
		KLAUNCH(k_tr_gather64, dim3(tgrid(T)), dim3(T_TPB), 0, s, T, perm, tpos, spos);
		KLAUNCH(k_tr_t1, dim3(tblk(T)), dim3(T_TPB), 0, s, T, SA, sq, spos, (flags & POVU_HIP_T_FORCE_TIER2) ? 1u : 0u, SO, handover);
		compact_flagged_u8(handover, T, list, words + 1, comp_tmp_b, comp_b, s);
		HIP_CHECK(copy_async(&n2, words + 1, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		if (n2) {
			const unsigned wg = (unsigned)std::min<uint64_t>(((uint64_t)n2 + T_TPB / 64 - 1) / (T_TPB / 64), 4096);
			KLAUNCH(k_tr_t2, dim3(wg), dim3(T_TPB), 0, s, list, n2, words + 2, SA, sq, spos, SO);
		}
		KLAUNCH(k_tr_closed, dim3(tgrid(T)), dim3(T_TPB), 0, s, T, tlen, closed);
		compact_flagged_u8(closed, T, list, words + 3, comp_tmp_b, comp_b, s);
		HIP_CHECK(copy_async(&R, words + 3, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
	}

	// ---- phase C: the traversals, grouped into alleles
	const size_t R1 = (size_t)R + 1;
	const size_t sort_c = sort_tmp_bytes(R1) + 256, scan_c = scan_tmp_bytes(std::max(R1, n1)) + 256, comp_c = compact_tmp_bytes(R1) + 256;
	uint64_t *rpos, *rhash;
	uint32_t *rq, *rlen, *pa, *pb, *key, *kout, *mark, *hmax, *head, *rep, *firstf, *aidx, *rallele, *afirst, *alen, *soff, *blist;
	uint32_t *toff, *aoff;
	uint8_t *rbad;
	void *sort_tmp_c, *scan_tmp_c, *comp_tmp_c;
	carve(ctx->tr_trav, [&](Spans &take) {
		take(R1, rpos, rhash, rq, rlen, pa, pb, key, kout, mark, hmax, head, rep);
		take(R1, firstf, aidx, rallele, afirst, alen, soff, blist);
		take(n1, toff, aoff);
		take(R1, rbad);
		take(sort_c, sort_tmp_c);
		take(scan_c, scan_tmp_c);
		take(comp_c, comp_tmp_c);
	});
	// (`list` of tr_task holds the traversals' task indices)
	uint64_t n_splits = 0;
	uint32_t n_al = 0;
	if (R) {
		KLAUNCH(k_tr_trav_fields, dim3(tgrid(R)), dim3(T_TPB), 0, s, R, list, sq, spos, tlen, thash, rq, rpos, rlen, rhash);
	}
	KLAUNCH(k_tr_query_off, dim3(tblk(n1)), dim3(T_TPB), 0, s, n, R, rq, toff);
	if (R) {
		// stable LSD sort of the traversal indices by (query, length, hash): least significant key first
		KLAUNCH(k_tr_iota, dim3(tgrid(R)), dim3(T_TPB), 0, s, R, pa);
		uint32_t *cur = pa, *nxt = pb;
		auto pass = [&](int which, unsigned bits) {
			KLAUNCH(k_tr_sort_key, dim3(tgrid(R)), dim3(T_TPB), 0, s, R, which, cur, rhash, rlen, rq, key);
			sort_pairs_u32(key, kout, cur, nxt, R, bits, sort_tmp_c, sort_c, s);
			std::swap(cur, nxt);
		};
		pass(0, std::min(hbits, 32u));
		if (hbits > 32)
			pass(1, hbits - 32);
		pass(2, bits_for(max_steps));
		pass(3, bits_for(n));
		const uint32_t *sp = cur;
		KLAUNCH(k_tr_heads, dim3(tgrid(R)), dim3(T_TPB), 0, s, R, sp, rhash, rlen, rq, mark);
		scan_exclusive_max_u32(mark, hmax, R, scan_tmp_c, scan_c, s);
		HIP_CHECK(hipMemsetAsync(rbad, 0, R1, s));
		HIP_CHECK(hipMemsetAsync(tot, 0, 16, s));
		KLAUNCH(k_tr_check, dim3(tgrid(R)), dim3(T_TPB), 0, s, R, ctx->path_steps, sp, hmax, mark, rpos, rlen, head, rep, rbad);
		compact_flagged_u8(rbad, R, blist, words + 4, comp_tmp_c, comp_c, s);
		uint32_t nb = 0;
		HIP_CHECK(copy_async(&nb, words + 4, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		if (nb) {
			KLAUNCH(k_tr_regroup, dim3(tblk(nb)), dim3(T_TPB), 0, s, nb, blist, R, ctx->path_steps, sp, head, rpos, rlen, rep, tot + 1);
			HIP_CHECK(copy_async(&n_splits, tot + 1, 8, hipMemcpyDeviceToHost, s));
		}
		HIP_CHECK(hipMemsetAsync(firstf, 0, R1 * 4, s));
		KLAUNCH(k_tr_first, dim3(tgrid(R)), dim3(T_TPB), 0, s, R, sp, rep, firstf);
		scan_exclusive_u32(firstf, aidx, R1, scan_tmp_c, scan_c, s);
		HIP_CHECK(copy_async(&n_al, aidx + R, 4, hipMemcpyDeviceToHost, s));
		KLAUNCH(k_tr_allele, dim3(tgrid(R)), dim3(T_TPB), 0, s, R, sp, rep, aidx, rlen, rallele, afirst, alen);
		HIP_CHECK(hipStreamSynchronize(s));
	} else {
		HIP_CHECK(hipMemsetAsync(aidx, 0, 4, s));
	}
	KLAUNCH(k_tr_allele_off, dim3(tblk(n1)), dim3(T_TPB), 0, s, n, toff, aidx, aoff);
	uint64_t n_steps = 0;
	if (n_al)
		totals_u32(alen, nullptr, n_al, tot, &n_steps, s);
	check_32(n_steps, "allele steps");
	if (n_al) {
		HIP_CHECK(hipMemsetAsync(alen + n_al, 0, 4, s));
		scan_exclusive_u32(alen, soff, (size_t)n_al + 1, scan_tmp_c, scan_c, s);
	}

	// ---- outputs: per traversal and allele steps, in tr_steps
	uint32_t *op, *of, *ol, *oa, *sid;
	uint8_t *orv, *sor;
	carve(ctx->tr_steps, [&](Spans &take) {
		take(R1, op, of, ol, oa, orv);
		take(n_steps + 1, sid, sor);
	});
	if (R)
		KLAUNCH(k_tr_out, dim3(tgrid(R)), dim3(T_TPB), 0, s, R, ctx->path_off, P, rq, rpos, rlen, rallele, aidx, toff, op, of, ol, oa, orv);
	if (n_al)
		KLAUNCH(k_tr_allele_steps, dim3((unsigned)std::min<uint64_t>(((uint64_t)n_al + 3) / 4, 65536)), dim3(T_TPB), 0, s, n_al,
			ctx->path_steps, g.vid, afirst, rpos, rlen, soff, sid, sor);

	TravDevice d;
	d.q = q;
	d.R = R;
	d.n_al = n_al;
	d.n2 = n2;
	d.n_steps = n_steps;
	d.n_splits = n_splits;
	d.op = op, d.of = of, d.ol = ol, d.oa = oa, d.sid = sid, d.toff = toff, d.aoff = aoff, d.qstatus = qstatus;
	d.soff = soff, d.rq = rq, d.rlen = rlen, d.afirst = afirst, d.orv = orv, d.sor = sor, d.rpos = rpos;
	return d;
}
} // namespace povu_hip

extern "C" povu_hip_traversals *povu_hip_forest_traversals(povu_hip_ctx *ctx, povu_hip_forest *f, const povu_hip_trav_opts *opts,
							   char *err, size_t errlen)
{
	CallTimer timer;
	return guarded_call(ctx, err, errlen, (povu_hip_traversals *)nullptr, [&] {
		check_query_forest(ctx, f, "traversals");
		const TravDevice d = trav_pipeline(
			ctx, [&](CallTimer &tm, const QueryLayout &more) { return query_front(ctx, f, ctx->tr_ws, tm, more); }, opts, timer);
		hipStream_t s = ctx->stream;
		const uint32_t n = d.q.n, R = d.R, n_al = d.n_al;
		const uint64_t n_steps = d.n_steps;
		const size_t n1 = (size_t)n + 1;
		// ---- to the host
		auto o = std::make_unique<TraversalsOwner>();
		std::vector<uint32_t> h_toff(n1), h_aoff(n1), h_status(n1), h_soff((size_t)n_al + 1);
		hand_off(o->path, R, d.op, R, ctx);
		hand_off(o->first, R, d.of, R, ctx);
		hand_off(o->last, R, d.ol, R, ctx);
		hand_off(o->allele, R, d.oa, R, ctx);
		hand_off(o->reverse, R, d.orv, R, ctx);
		hand_off(o->step_id, n_steps, d.sid, n_steps, ctx);
		hand_off(o->step_or, n_steps, d.sor, n_steps, ctx);
		HIP_CHECK(copy_async(h_toff.data(), d.toff, n1 * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(h_aoff.data(), d.aoff, n1 * 4, hipMemcpyDeviceToHost, s));
		if (n)
			HIP_CHECK(copy_async(h_status.data(), d.qstatus, (size_t)n * 4, hipMemcpyDeviceToHost, s));
		if (n_al)
			HIP_CHECK(copy_async(h_soff.data(), d.soff, ((size_t)n_al + 1) * 4, hipMemcpyDeviceToHost, s));
		o->view.device_ms = timer.stop(s);
		o->trav_off.assign(h_toff.begin(), h_toff.end());
		o->allele_off.assign(h_aoff.begin(), h_aoff.end());
		o->status.resize(n);
		for (uint32_t q = 0; q < n; q++)
			o->status[q] = (uint8_t)h_status[q];
		o->step_off.assign(h_soff.begin(), h_soff.end());
		o->view.n_queries = n;
		o->view.n_traversals = R;
		o->view.n_alleles = n_al;
		o->view.n_steps = n_steps;
		o->view.trav_off = o->trav_off.data();
		o->view.allele_off = o->allele_off.data();
		o->view.status = o->status.data();
		o->view.path = o->path.data();
		o->view.first = o->first.data();
		o->view.last = o->last.data();
		o->view.allele = o->allele.data();
		o->view.reverse = o->reverse.data();
		o->view.step_off = o->step_off.data();
		o->view.step_id = o->step_id.data();
		o->view.step_or = o->step_or.data();
		o->view.n_tier2 = d.n2;
		o->view.n_hash_splits = d.n_splits;
		TraversalsOwner *raw = o.release();
		return &raw->view;
	});
}
extern "C" void povu_hip_traversals_free(povu_hip_traversals *t)
{
	delete reinterpret_cast<TraversalsOwner *>(t);
}
