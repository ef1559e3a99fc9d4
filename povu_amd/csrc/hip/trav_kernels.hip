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
#include "exact_groups.hpp"

namespace povu_hip
{

static constexpr uint32_t T_PER_LANE = 16;		 // steps per lane of the start-task passes
static constexpr uint32_t T_TILE = Q_TPB * T_PER_LANE; // steps per workgroup of the start-task passes
static constexpr uint32_t T1_STEPS = 64;		 // steps tier 1 looks at before it hands a scan over
static constexpr uint8_t TS_LONG = POVU_HIP_TRAV_LONG, TS_STRAY = POVU_HIP_TRAV_STRAY, TS_OPEN = POVU_HIP_TRAV_OPEN;

// ---- paths: segment ids -> step words (the ids were copied into `steps`, mapped in place); the lowest step whose id the
// graph does not have is kept in *bad
__global__ void k_tr_map_steps(uint64_t N, uint32_t *__restrict__ steps, const uint8_t *__restrict__ rev,
			       const uint32_t *__restrict__ vid, uint32_t V, unsigned long long *__restrict__ bad)
{
	for (uint64_t i = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; i < N; i += (uint64_t)gridDim.x * Q_TPB) {
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
	const uint32_t q = blockIdx.x * Q_TPB + threadIdx.x;
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

// ---- start tasks.  Lane t of a workgroup looks at steps base + k Q_TPB + t, k < T_PER_LANE (coalesced); the emit pass
// ranks them in step order with a workgroup scan per k.
__device__ __forceinline__ uint32_t wg_exclusive_scan(uint32_t v, uint32_t &total, uint32_t *lds /* [Q_TPB / 64 + 1] */)
{
	const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
	const uint32_t x = wave_inclusive_sum(v);
	if (lane == 63)
		lds[wv] = x;
	__syncthreads();
	uint32_t before = 0, all = 0;
	for (uint32_t w = 0; w < Q_TPB / 64; w++) {
		const uint32_t c = lds[w];
		before += w < wv ? c : 0;
		all += c;
	}
	__syncthreads();
	total = all;
	return before + x - v;
}

__global__ __launch_bounds__(Q_TPB) void k_tr_count(uint64_t N, const uint32_t *__restrict__ steps, const uint32_t *__restrict__ boff,
						    uint32_t *__restrict__ tile_cnt)
{
	__shared__ uint32_t lds[Q_TPB / 64 + 1];
	const uint64_t base = (uint64_t)blockIdx.x * T_TILE;
	uint32_t c = 0;
	for (uint32_t k = 0; k < T_PER_LANE; k++) {
		const uint64_t i = base + (uint64_t)k * Q_TPB + threadIdx.x;
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

__global__ __launch_bounds__(Q_TPB) void k_tr_emit(uint64_t N, const uint32_t *__restrict__ steps, const uint32_t *__restrict__ boff,
						   const uint32_t *__restrict__ bval, const uint32_t *__restrict__ tile_off,
						   uint64_t *__restrict__ tpos, uint32_t *__restrict__ tkey)
{
	__shared__ uint32_t lds[Q_TPB / 64 + 1];
	const uint64_t base = (uint64_t)blockIdx.x * T_TILE;
	uint32_t at = tile_off[blockIdx.x];
	for (uint32_t k = 0; k < T_PER_LANE; k++) {
		const uint64_t i = base + (uint64_t)k * Q_TPB + threadIdx.x;
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

// out[k] = in[perm[k]] (u64 / u32)
__global__ void k_tr_gather64(uint32_t n, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ in, uint64_t *__restrict__ out)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < n; k += gridDim.x * Q_TPB)
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
	const TravSpan sp = trav_span(tp, 0);
	t.rev = sp.rev;
	t.pos = sp.p;
	const uint32_t ys = A.ys[q], yz = A.yz[q];
	t.a = ys >> 1;
	t.z = yz >> 1;
	t.close = t.rev ? ys ^ 1u : yz;
	const uint64_t end = A.path_off[span_of(A.path_off, A.n_paths, t.pos) + 1];
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
__global__ __launch_bounds__(Q_TPB) void k_tr_t1(uint32_t T, ScanArgs A, const uint32_t *__restrict__ tq, const uint64_t *__restrict__ tpos,
						 uint32_t force2, ScanOut O, uint8_t *__restrict__ handover)
{
	const uint32_t k = blockIdx.x * Q_TPB + threadIdx.x;
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

// tier 2: one wave per task of `list`, every wave taking its next task from *next (zeroed before the launch); 64 steps a
// ballot to find the end, then 64 steps a pass to hash the sequence
__global__ __launch_bounds__(Q_TPB) void k_tr_t2(const uint32_t *__restrict__ list, uint32_t n2, uint32_t *__restrict__ next, ScanArgs A,
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
		h = wave_sum(h);
		if (lane == 0) {
			O.len[k] = len;
			O.hash[k] = keep_bits(A, h);
		}
	}
}

__global__ void k_tr_closed(uint32_t T, const uint32_t *__restrict__ len, uint8_t *__restrict__ closed)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < T; k += gridDim.x * Q_TPB)
		closed[k] = len[k] != 0;
}

// the traversals (closed tasks, `list` in sorted task order): their query, position (with role), length and hash
__global__ void k_tr_trav_fields(uint32_t R, const uint32_t *__restrict__ list, const uint32_t *__restrict__ tq,
				 const uint64_t *__restrict__ tpos, const uint32_t *__restrict__ len, const uint64_t *__restrict__ hash,
				 uint32_t *__restrict__ rq, uint64_t *__restrict__ rpos, uint32_t *__restrict__ rlen,
				 uint64_t *__restrict__ rhash)
{
	for (uint32_t t = blockIdx.x * Q_TPB + threadIdx.x; t < R; t += gridDim.x * Q_TPB) {
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
	const uint32_t q = blockIdx.x * Q_TPB + threadIdx.x;
	if (q > n)
		return;
	off[q] = lower_bound(rq, 0u, R, q);
}

__device__ __forceinline__ bool same_sequence(const uint32_t *__restrict__ steps, uint64_t pa, uint64_t pb, uint32_t len)
{
	const TravSpan a = trav_span(pa, len), b = trav_span(pb, len);
	for (uint32_t i = 0; i < len; i++)
		if (a.step(steps, i) != b.step(steps, i))
			return false;
	return true;
}

// traversals a and b (of one query and length) spell the same step sequence
struct SameTraversal {
	const uint32_t *steps;
	const uint64_t *rpos;
	const uint32_t *rlen;
	__device__ __forceinline__ bool operator()(uint32_t a, uint32_t b) const { return same_sequence(steps, rpos[a], rpos[b], rlen[a]); }
};

// allele of every traversal (global numbering: aidx of its group's first traversal); the first traversal of every allele
__global__ void k_tr_allele(uint32_t R, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ rep, const uint32_t *__restrict__ aidx,
			    const uint32_t *__restrict__ rlen, uint32_t *__restrict__ rallele, uint32_t *__restrict__ afirst,
			    uint32_t *__restrict__ alen)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < R; k += gridDim.x * Q_TPB) {
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
	for (uint32_t t = blockIdx.x * Q_TPB + threadIdx.x; t < R; t += gridDim.x * Q_TPB) {
		const TravSpan sp = trav_span(rpos, rlen, t);
		const uint32_t p = span_of(path_off, n_paths, sp.p);
		o_path[t] = p;
		o_first[t] = (uint32_t)(sp.first_pos() - path_off[p]);
		o_last[t] = (uint32_t)(sp.last_pos() - path_off[p]);
		o_rev[t] = sp.rev ? 1 : 0;
		o_allele[t] = rallele[t] - aidx[toff[rq[t]]];
	}
}

// allele_off[q] = aidx[trav_off[q]]
__global__ void k_tr_allele_off(uint32_t n, const uint32_t *__restrict__ toff, const uint32_t *__restrict__ aidx, uint32_t *__restrict__ aoff)
{
	const uint32_t q = blockIdx.x * Q_TPB + threadIdx.x;
	if (q <= n)
		aoff[q] = aidx[toff[q]];
}

// the steps of every allele (S -> Z), one wave per allele
__global__ __launch_bounds__(Q_TPB) void k_tr_allele_steps(uint32_t n_al, const uint32_t *__restrict__ steps, const uint32_t *__restrict__ vid,
							   const uint32_t *__restrict__ afirst, const uint64_t *__restrict__ rpos,
							   const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ soff,
							   uint32_t *__restrict__ o_id, uint8_t *__restrict__ o_or)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	for (uint32_t a = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); a < n_al; a += waves) {
		const uint32_t at = soff[a];
		const TravSpan sp = trav_span(rpos, rlen, afirst[a]);
		for (uint32_t i = lane; i < sp.len; i += 64) {
			const uint32_t x = sp.step(steps, i);
			o_id[at + i] = vid[x >> 1];
			o_or[at + i] = (uint8_t)(x & 1u);
		}
	}
}

static void check_32(uint64_t v, const char *what)
{
	refuse_2_32(v, "the traversals need ", what, " for now (the scans and sorts here are 32-bit)");
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
			KLAUNCH(k_tr_map_steps, dim3(stride_blocks(N)), dim3(Q_TPB), 0, s, N, ctx->path_steps, rev, g.vid, g.V, bad);
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
namespace
{
// what a call asks for and what is resident
struct TravParams {
	povu_hip_ctx *ctx;
	hipStream_t s;
	uint32_t max_steps, flags, hbits;
	uint64_t N, n_tiles; // path steps, their tiles of T_TILE in the start-task passes
	uint32_t P, nS;
};
// phase A (the front end's arena): the queries, the boundary table, the tile counts
struct TravBoundary {
	QueryFront q;
	size_t n1; // queries + 1
	uint32_t *qstatus, *boff, *bval, *tile_cnt, *tile_off; // bval: the table's (query, role) entries
	unsigned long long *tot;
	void *tmp;
	size_t tmp_bytes;
};
// phase B (tr_task): the tasks, sorted by query, and what their scans found
struct TravTasks {
	uint32_t T = 0, n2 = 0, R = 0; // tasks, those tier 2 took, those that closed (the traversals)
	uint32_t *sq, *tlen, *list;    // list: the tasks handed over, then the closed ones
	uint64_t *spos, *thash;
	uint8_t *handover, *closed;
	void *tmp;
	size_t tmp_bytes;
};
// phase C (tr_trav): the traversals, grouped into alleles
struct TravGroups {
	uint64_t *rpos;
	uint32_t *rq, *rlen, *toff, *aoff, *rep, *firstf, *aidx, *rallele, *afirst, *alen, *soff;
	const uint32_t *sp; // the traversals sorted by (query, length, hash)
	void *tmp;
	size_t tmp_bytes;
	uint32_t n_al = 0;
	uint64_t n_splits = 0, n_steps = 0;
};
} // namespace

static TravBoundary boundary_table(const TravParams &p, const QueryFrontFn &front, CallTimer &timer)
{
	hipStream_t s = p.s;
	TravBoundary b;
	uint32_t *bkey, *bval, *bkey2, *bcnt;
	b.q = front(timer, [&](Spans &take, uint32_t n) {
		const size_t n2q = 2 * (size_t)n + 1;
		b.tmp_bytes = std::max(prim_tmp_bytes(std::max<size_t>((size_t)p.nS + 1, p.n_tiles + 1), false), sort_tmp_bytes(n2q)) + 256;
		take((size_t)n + 1, b.qstatus);
		take(n2q, bkey, bval, bkey2, b.bval);
		take((size_t)p.nS + 1, bcnt, b.boff);
		take(p.n_tiles + 1, b.tile_cnt, b.tile_off);
		take(2, b.tot);
		take(b.tmp_bytes, b.tmp);
	});
	const uint32_t n = b.q.n;
	b.n1 = (size_t)n + 1;
	HIP_CHECK(hipMemsetAsync(b.qstatus, 0, b.n1 * 4, s));
	HIP_CHECK(hipMemsetAsync(bcnt, 0, ((size_t)p.nS + 1) * 4, s));
	uint32_t hw[8] = {0};
	HIP_CHECK(copy_async(hw, b.q.words, 32, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	query_refusals(hw[0], "traversals");
	if (n) {
		KLAUNCH(k_tr_keys, dim3(lane_blocks(n)), dim3(Q_TPB), 0, s, n, p.nS, b.q.ys, b.q.yz, bkey, bval, bcnt);
		sort_pairs_u32(bkey, bkey2, bval, b.bval, 2 * (size_t)n, bits_for(p.nS), b.tmp, b.tmp_bytes, s);
	}
	scan_exclusive_u32(bcnt, b.boff, (size_t)p.nS + 1, b.tmp, b.tmp_bytes, s);
	return b;
}

// count per tile, total, offsets, emit, sort by query
static TravTasks start_tasks(const TravParams &p, const TravBoundary &b)
{
	povu_hip_ctx *ctx = p.ctx;
	hipStream_t s = p.s;
	TravTasks t;
	if (p.n_tiles)
		KLAUNCH(k_tr_count, dim3((unsigned)p.n_tiles), dim3(Q_TPB), 0, s, p.N, ctx->path_steps, b.boff, b.tile_cnt);
	counts_to_offsets(b.tile_cnt, b.tile_off, nullptr, nullptr, p.n_tiles, b.tot, b.tmp, b.tmp_bytes, s, [&](const uint64_t *total) {
		check_32(total[0], "scan tasks");
		t.T = (uint32_t)total[0];
	});
	const uint32_t T = t.T;
	const size_t T1 = (size_t)T + 1;
	t.tmp_bytes = prim_tmp_bytes(T1, true) + 256;
	uint64_t *tpos;
	uint32_t *tkey, *tval, *perm;
	carve(ctx->tr_task, [&](Spans &take) {
		take(T1, tpos, t.spos, t.thash, tkey, tval, t.sq, perm, t.tlen, t.list, t.handover, t.closed);
		take(t.tmp_bytes, t.tmp);
	});
	if (T) {
		KLAUNCH(k_tr_emit, dim3((unsigned)p.n_tiles), dim3(Q_TPB), 0, s, p.N, ctx->path_steps, b.boff, b.bval, b.tile_off, tpos, tkey);
		launch_iota(T, tval, s);
		sort_pairs_u32(tkey, t.sq, tval, perm, T, bits_for(b.q.n), t.tmp, t.tmp_bytes, s);
		KLAUNCH(k_tr_gather64, dim3(stride_blocks(T)), dim3(Q_TPB), 0, s, T, perm, tpos, t.spos);
	}
	return t;
}

// tier 1, the hand-over, tier 2, the closed tasks
static void scan_tasks(const TravParams &p, const TravBoundary &b, TravTasks &t)
{
	hipStream_t s = p.s;
	const uint32_t T = t.T, hbits = p.hbits;
	uint32_t *words = b.q.words;
	if (!T)
		return;
	const ScanArgs SA{p.ctx->path_steps, p.ctx->path_off, p.P, b.q.ys, b.q.yz, p.max_steps,
			  hbits >= 64 ? 0xFFFFFFFFu : hbits > 32 ? (1u << (hbits - 32)) - 1 : 0u, hbits >= 32 ? 0xFFFFFFFFu : (1u << hbits) - 1};
	const ScanOut SO{t.tlen, t.thash, b.qstatus};
	KLAUNCH(k_tr_t1, dim3(lane_blocks(T)), dim3(Q_TPB), 0, s, T, SA, t.sq, t.spos, (p.flags & POVU_HIP_T_FORCE_TIER2) ? 1u : 0u, SO, t.handover);
	compact_flagged_u8(t.handover, T, t.list, words + 1, t.tmp, t.tmp_bytes, s);
	t.n2 = read_back(words + 1, s);
	if (t.n2) {
		const unsigned wg = (unsigned)std::min<uint64_t>(((uint64_t)t.n2 + Q_TPB / 64 - 1) / (Q_TPB / 64), 4096);
		KLAUNCH(k_tr_t2, dim3(wg), dim3(Q_TPB), 0, s, t.list, t.n2, words + 2, SA, t.sq, t.spos, SO);
	}
	KLAUNCH(k_tr_closed, dim3(stride_blocks(T)), dim3(Q_TPB), 0, s, T, t.tlen, t.closed);
	compact_flagged_u8(t.closed, T, t.list, words + 3, t.tmp, t.tmp_bytes, s);
	t.R = read_back(words + 3, s);
}

// the traversals' fields, the LSD sort by (query, length, hash), run heads, the check of every run, the exact regrouping of
// the runs with a mismatch.  g.n_splits is on its way to the host when this returns: alleles() waits for it.
static void dedup(const TravParams &p, const TravBoundary &b, const TravTasks &t, TravGroups &g)
{
	povu_hip_ctx *ctx = p.ctx;
	hipStream_t s = p.s;
	const uint32_t n = b.q.n, R = t.R, hbits = p.hbits;
	uint32_t *words = b.q.words;
	const size_t R1 = (size_t)R + 1, n1 = b.n1;
	g.tmp_bytes = std::max(prim_tmp_bytes(R1, true), prim_tmp_bytes(n1, false)) + 256;
	uint64_t *rhash;
	uint32_t *pa, *pb, *key, *kout, *mark, *hmax, *head, *blist;
	uint8_t *rbad;
	carve(ctx->tr_trav, [&](Spans &take) {
		take(R1, g.rpos, rhash, g.rq, g.rlen, pa, pb, key, kout, mark, hmax, head, g.rep);
		take(R1, g.firstf, g.aidx, g.rallele, g.afirst, g.alen, g.soff, blist);
		take(n1, g.toff, g.aoff);
		take(R1, rbad);
		take(g.tmp_bytes, g.tmp);
	});
	// (`list` of tr_task holds the traversals' task indices)
	if (R) {
		KLAUNCH(k_tr_trav_fields, dim3(stride_blocks(R)), dim3(Q_TPB), 0, s, R, t.list, t.sq, t.spos, t.tlen, t.thash, g.rq, g.rpos, g.rlen, rhash);
	}
	KLAUNCH(k_tr_query_off, dim3(lane_blocks(n1)), dim3(Q_TPB), 0, s, n, R, g.rq, g.toff);
	if (!R)
		return;
	GroupWs gw{pa, pb, key, kout, mark, hmax, head, g.rep, blist, rbad, g.tmp, g.tmp_bytes};
	g.sp = group_exact(R, g.rq, g.rlen, rhash, hbits, bits_for(p.max_steps), bits_for(n), SameTraversal{ctx->path_steps, g.rpos, g.rlen}, gw,
			   words + 4, b.tot + 1, &g.n_splits, s);
}

// an allele per group, numbered in traversal order; the alleles of every query; their step offsets
static void alleles(const TravParams &p, const TravBoundary &b, const TravTasks &t, TravGroups &g)
{
	hipStream_t s = p.s;
	const uint32_t n = b.q.n, R = t.R;
	if (R) {
		number_groups(R, g.sp, g.rep, g.firstf, g.aidx, nullptr, g.tmp, g.tmp_bytes, s);
		HIP_CHECK(copy_async(&g.n_al, g.aidx + R, 4, hipMemcpyDeviceToHost, s));
		KLAUNCH(k_tr_allele, dim3(stride_blocks(R)), dim3(Q_TPB), 0, s, R, g.sp, g.rep, g.aidx, g.rlen, g.rallele, g.afirst, g.alen);
		HIP_CHECK(hipStreamSynchronize(s));
	} else {
		HIP_CHECK(hipMemsetAsync(g.aidx, 0, 4, s));
	}
	KLAUNCH(k_tr_allele_off, dim3(lane_blocks(b.n1)), dim3(Q_TPB), 0, s, n, g.toff, g.aidx, g.aoff);
	if (g.n_al)
		counts_to_offsets(g.alen, g.soff, nullptr, nullptr, g.n_al, b.tot, g.tmp, g.tmp_bytes, s, [&](const uint64_t *total) {
			check_32(total[0], "allele steps");
			g.n_steps = total[0];
		});
}

// per traversal and allele steps, in tr_steps
static TravDevice outputs(const TravParams &p, const TravBoundary &b, const TravTasks &t, const TravGroups &g)
{
	povu_hip_ctx *ctx = p.ctx;
	hipStream_t s = p.s;
	const uint32_t R = t.R, n_al = g.n_al;
	TravDevice d;
	carve(ctx->tr_steps, [&](Spans &take) {
		take((size_t)R + 1, d.op, d.of, d.ol, d.oa, d.orv);
		take(g.n_steps + 1, d.sid, d.sor);
	});
	if (R)
		KLAUNCH(k_tr_out, dim3(stride_blocks(R)), dim3(Q_TPB), 0, s, R, ctx->path_off, p.P, g.rq, g.rpos, g.rlen, g.rallele, g.aidx, g.toff, d.op, d.of,
			d.ol, d.oa, d.orv);
	if (n_al)
		KLAUNCH(k_tr_allele_steps, dim3(wave_blocks(n_al)), dim3(Q_TPB), 0, s, n_al, ctx->path_steps, ctx->g.vid, g.afirst, g.rpos, g.rlen, g.soff,
			d.sid, d.sor);
	d.q = b.q;
	d.R = R;
	d.n_al = n_al;
	d.n2 = t.n2;
	d.n_steps = g.n_steps;
	d.n_splits = g.n_splits;
	d.toff = g.toff, d.aoff = g.aoff, d.qstatus = b.qstatus;
	d.soff = g.soff, d.rq = g.rq, d.rlen = g.rlen, d.afirst = g.afirst, d.rpos = g.rpos;
	return d;
}

TravDevice trav_pipeline(povu_hip_ctx *ctx, const QueryFrontFn &front, const povu_hip_trav_opts *opts, CallTimer &timer)
{
	if (!ctx->paths_valid || ctx->paths_gen != ctx->g.gen)
		throw HipError("no paths are resident for the graph now uploaded (povu_hip_paths_upload after povu_hip_graph_upload)");
	TravParams p{ctx, ctx->stream, 65536, 0, hash_bits_hook(), ctx->n_path_steps, 0, ctx->n_paths, 2 * ctx->g.V};
	if (opts) {
		if (opts->max_steps == 1)
			throw HipError("max_steps must be at least 2");
		if (opts->max_steps)
			p.max_steps = opts->max_steps;
		p.flags = opts->flags;
	}
	p.n_tiles = (p.N + T_TILE - 1) / T_TILE;
	check_32(p.n_tiles + 1, "start-task tiles");
	const TravBoundary b = boundary_table(p, front, timer);
	TravTasks t = start_tasks(p, b);
	scan_tasks(p, b, t);
	TravGroups g;
	dedup(p, b, t, g);
	alleles(p, b, t, g);
	return outputs(p, b, t, g);
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
