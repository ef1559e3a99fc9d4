// list_rank.hip -- the splitter-based list ranking behind list_rank.hpp (the contract with its callers stands there): the
// splitter rule, the walks up and down the levels, the pointer jumping of the top level, the planner and driver, the writer of
// the level-0 records, their statistics and the unit-test hook.
#include "list_rank.hpp"

#include <cstdlib>

#include <algorithm>
#include <vector>

namespace povu_hip
{

#ifndef NIL
#define NIL POVU_NIL
#endif

// ---- list-ranking words and splitters (section "work-efficient list ranking" below).
// Splitters cut every list into short segments.  The index space of a list level is cut into buckets of 2^b
// consecutive elements and every bucket names exactly ONE of its elements as a splitter, pseudo-randomly
// (multiplicative hash of the bucket idx).  So the splitter of bucket q is computed, not looked up; a splitter's id on
// the next level IS its bucket idx (dense, no flag array, no scan, no compaction), and lane q of a walk kernel works
// near element q * 2^b (the scattered rank stores of neighbouring lanes meet again in L2).
// b = 3 (1 in 8): short segments, whose walks are bound by their longest one; b = 4 is kept as an A/B switch.
unsigned rank_bucket_bits(const PassHooks &hooks) { return hooks.rank_bits; } // (tuning hook; the default and its measurement: pass_hooks.hpp)
// words of the levels above the list (their elements number an eighth of it), so that a walk step is ONE dependent load:
// bits 0..28 successor (PK_END = none), bit 31 = stop after this element (the successor is a splitter, or there is none).
// Their weights are words of their own (the sums of the level below).
static constexpr uint32_t PK_END = 0x1FFFFFFFu, PK_STOP = 0x80000000u;
__device__ __forceinline__ uint32_t bucket_splitter(uint32_t q, unsigned b) { return (q << b) | ((q * 0x9E3779B1u) >> (32u - b)); }
__device__ __forceinline__ bool is_splitter(uint32_t i, unsigned b) { return bucket_splitter(i >> b, b) == i; }
__device__ __forceinline__ bool rank_l0_stop(uint32_t nx, unsigned b) { return nx == P0_END || is_splitter(nx, b); }
// one launch = several rounds of pointer jumping with two accumulators (suffix sums along the list):
// HOPS = 3 covers two rounds (every pointer then spans 4x as far), HOPS = 7 three rounds (8x).  More
// hops per launch mean fewer launches but more loads in total, which pays only while the launches are
// dispatch-bound (short splitter lists).
template <int HOPS>
__global__ void k_wyllie(uint32_t n, const uint32_t *__restrict__ nxt_in, const uint32_t *__restrict__ a_in,
			 const uint32_t *__restrict__ b_in, uint32_t *__restrict__ nxt_out, uint32_t *__restrict__ a_out,
			 uint32_t *__restrict__ b_out, const uint32_t *__restrict__ n_dev)
{
	uint32_t i = BIDX * blockDim.x + threadIdx.x;
	if (i >= n || (n_dev && i >= *n_dev))
		return;
	uint32_t nx = nxt_in[i], a = a_in[i], b = b_in ? b_in[i] : 0;
#pragma unroll
	for (int hop = 0; hop < HOPS; hop++) {
		if (nx == NIL)
			break;
		a += a_in[nx];
		if (b_in)
			b += b_in[nx];
		nx = nxt_in[nx];
	}
	nxt_out[i] = nx;
	a_out[i] = a;
	if (b_out)
		b_out[i] = b;
}
// `bits` = bits_for(longest possible list); returns which buffer set (0 = A, 1 = B) holds the result
static int list_rank(uint32_t n, unsigned bits, uint32_t *nxtA, uint32_t *nxtB, uint32_t *aA, uint32_t *aB, uint32_t *bA,
		     uint32_t *bB, hipStream_t s, const uint32_t *n_dev = nullptr)
{
	int cur = 0;
	const bool small = n < (1u << 21);
	const unsigned launches = small ? (bits + 2) / 3 : (bits + 1) / 2;
	for (unsigned r = 0; r < launches; r++) {
		uint32_t *ni = cur ? nxtB : nxtA, *no = cur ? nxtA : nxtB, *ai = cur ? aB : aA, *ao = cur ? aA : aB;
		uint32_t *bi = cur ? bB : bA, *bo = cur ? bA : bB;
		if (small)
			LAUNCH(k_wyllie<7>, n, s, n, ni, ai, bi, no, ao, bo, n_dev);
		else
			LAUNCH(k_wyllie<3>, n, s, n, ni, ai, bi, no, ao, bo, n_dev);
		cur ^= 1;
	}
	return cur;
}

// ---- work-efficient list ranking, recursive.  Level 0 is the list itself (packed words, 0/1 weights).  One lane per
// splitter (= per bucket, plus one per list head) walks its segment and leaves {next splitter, segment sums} -- the
// element of the next level, whose index is the bucket idx.  Levels shrink by 2^b until one workgroup ranks the top in
// LDS (pointer jumping); then every level above the list hands its elements their suffix sums on the way back down.
// The list itself is walked once: its walk up leaves a record per element, from which the readers work out the rank
// (see k_rank_up).  A list of n elements costs about n(1 + 2^-b + ...) dependent loads up and n 2^-b(1 + ...) down.
// Heads: an element that heads a list is never reached through its bucket (its lane stays idle); head h of the caller's
// head array is element m + h of every level above 0 (m = buckets of the level below) and is walked by its own lane.
// EV (the pre-order events): two sums, and at level 0 the weights follow from the index (rank_l0_weights); the levels
// above carry the second sum as a second word per element (TWO).
static constexpr uint32_t RANK_TOP = 8192; // elements one workgroup ranks in LDS
struct RankLevelArgs {
	uint32_t n;	// elements of this level
	uint32_t m;	// buckets of this level = hash lanes of the walk
	uint32_t hbase; // first head element of this level (level 0: unused, heads come from the array)
	uint32_t M;	// lanes of the walk = elements of the next level = m + heads
};
// start element of lane `id`, NIL when the lane has nothing to walk
template <bool L0>
__device__ __forceinline__ uint32_t rank_lane_start(uint32_t id, const RankLevelArgs &A, unsigned b, const uint32_t *__restrict__ pk0,
						    const uint32_t *__restrict__ heads)
{
	if (id < A.m) {
		const uint32_t x = bucket_splitter(id, b);
		if (x >= A.n)
			return NIL;
		if (L0)
			return (pk0[x] & P0_HEAD) ? NIL : x;
		return x >= A.hbase ? NIL : x;
	}
	return L0 ? heads[id - A.m] : A.hbase + (id - A.m);
}
// the weights of level-0 element x with word p.  The tour (!EV): one, the weight bit.  EV: the elements are the events of
// the pre-order ranking, three per segment, and an element's two weights follow from its index: 3g = enter both sides of
// segment g (+2 entered, depth +2), 3g + 1 = leave the far side (depth -1, or -2 when the weight bit says the entered side
// is left with it), 3g + 2 = leave the entered side (depth -1).
template <bool EV>
__device__ __forceinline__ void rank_l0_weights(uint32_t x, uint32_t p, uint32_t &wa, uint32_t &wb)
{
	if constexpr (EV) {
		const uint32_t t = x % 3u;
		wa = t == 0 ? 2u : 0u;
		wb = t == 0 ? 2u : ((t == 1 && (p & P0_W)) ? 0u - 2u : 0u - 1u);
	} else {
		wa = (p & P0_W) ? 1u : 0u;
		wb = 0u; // (no second sum)
	}
}
struct RecPlanes {
	uint32_t *w0, *w1;
};
// plane 1 begins at a multiple of four words, so that 16-byte loads of either plane are aligned alike
static RecPlanes rec_planes(uint2 *rec, size_t n)
{
	uint32_t *w = reinterpret_cast<uint32_t *>(rec);
	return RecPlanes{w, w + ((n + 3) & ~(size_t)3)};
}
// (the record format: list_rank.hpp, above rec_decode) the record of element x, walked by lane `owner`, with second word y (the tour: the partial; the events: pa | pd << 16)
template <bool TWO>
__device__ __forceinline__ void rec_store(const RecPlanes &rec, uint32_t x, unsigned b, uint32_t owner, uint32_t y)
{
	constexpr unsigned PB = TWO ? REC_E_PBITS : REC_T_PBITS, DB = TWO ? REC_E_DBITS : REC_T_DBITS;
	constexpr uint32_t PMAX = (1u << PB) - 1u, HALF = 1u << (DB - 1);
	const uint32_t d = owner - (x >> b), pa = TWO ? (y & REC_MAX) : y, pd = TWO ? (y >> 16) : 0u;
	if (d + HALF < 2u * HALF && pa <= PMAX && pd <= PMAX) {
		rec.w0[x] = ((d & (2u * HALF - 1u)) << (31u - DB)) | pa | (pd << PB);
	} else {
		rec.w0[x] = REC_ESC | owner;
		rec.w1[x] = y;
	}
}
template <bool L0, bool EV>
__global__ void k_rank_up(RankLevelArgs A, unsigned b, const uint32_t *__restrict__ nx_in, const uint32_t *__restrict__ a_in,
			  const uint32_t *__restrict__ b_in, const uint32_t *__restrict__ heads, uint32_t *__restrict__ nx_out,
			  uint32_t *__restrict__ a_out, uint32_t *__restrict__ b_out, RecPlanes rec, uint32_t *__restrict__ ovf)
{
	const uint32_t id = BIDX * blockDim.x + threadIdx.x;
	if (id >= A.M)
		return;
	uint32_t x = rank_lane_start<L0>(id, A, b, nx_in, heads);
	uint32_t sa = 0, sb = 0, out = PK_END | PK_STOP;
	bool big = false;
	if (x != NIL) {
		uint32_t p;
		bool stop;
		do {
			p = nx_in[x];
			if constexpr (L0) {
				uint32_t wa, wb;
				rank_l0_weights<EV>(x, p, wa, wb);
				if constexpr (EV) {
					big |= sa > REC_MAX || sa - sb > REC_MAX;
					rec_store<true>(rec, x, b, id, sa | ((sa - sb) << 16));
				} else {
					rec_store<false>(rec, x, b, id, sa);
				}
				sa += wa;
				if constexpr (EV)
					sb += wb;
				x = p & P0_END;
				stop = rank_l0_stop(x, b);
			} else {
				sa += a_in[x];
				if constexpr (EV)
					sb += b_in[x];
				x = p & PK_END;
				stop = (p & PK_STOP) != 0;
			}
		} while (!stop);
		if (x != (L0 ? P0_END : PK_END)) { // the successor is the splitter of its bucket: that bucket is its idx one level up
			const uint32_t q = x >> b;
			out = q | (is_splitter(q, b) ? PK_STOP : 0u);
		}
	}
	nx_out[id] = out;
	a_out[id] = sa;
	if constexpr (EV)
		b_out[id] = sb;
	if (L0 && EV && big)
		*ovf = 1u;
}
// (the events; a pass whose level-0 walk raised *ovf: the old way back over the list, final ranks a, b into the two planes; a grid-stride loop
// over the lanes, so that the launch costs next to nothing when the flag is down)
__global__ void k_rank_l0_fallback(RankLevelArgs A, unsigned b, const uint32_t *__restrict__ pk, const uint32_t *__restrict__ heads,
				   const uint32_t *__restrict__ ra, const uint32_t *__restrict__ rb, RecPlanes rec,
				   const uint32_t *__restrict__ ovf)
{
	if (!*ovf)
		return;
	for (uint32_t id = BIDX * blockDim.x + threadIdx.x; id < A.M; id += gridDim.x * blockDim.x) {
		uint32_t x = rank_lane_start<true>(id, A, b, pk, heads);
		if (x == NIL)
			continue;
		uint32_t sa = ra[id], sb = rb[id];
		do {
			const uint32_t p = pk[x];
			uint32_t wa, wb;
			rank_l0_weights<true>(x, p, wa, wb);
			rec.w0[x] = sa;
			rec.w1[x] = sb;
			sa -= wa;
			sb -= wb;
			x = p & P0_END;
		} while (!rank_l0_stop(x, b));
	}
}
// the way back (levels >= 1): lane `id` knows the suffix sums at its splitter (ra / rb of the level above) and hands
// every element of its segment its own, in place of its weights.
template <bool TWO>
__global__ void k_rank_down(RankLevelArgs A, unsigned b, const uint32_t *__restrict__ nx_in, uint32_t *a_io, uint32_t *b_io,
			    const uint32_t *__restrict__ ra, const uint32_t *__restrict__ rb)
{
	const uint32_t id = BIDX * blockDim.x + threadIdx.x;
	if (id >= A.M)
		return;
	uint32_t x = rank_lane_start<false>(id, A, b, nx_in, nullptr);
	if (x == NIL)
		return;
	uint32_t sa = ra[id], sb = TWO ? rb[id] : 0, p;
	do {
		p = nx_in[x];
		const uint32_t wa = a_io[x];
		a_io[x] = sa;
		sa -= wa;
		if (TWO) {
			const uint32_t wb = b_io[x];
			b_io[x] = sb;
			sb -= wb;
		}
		x = p & PK_END;
	} while (!(p & PK_STOP));
}
// top level: inclusive suffix sums of at most RANK_TOP elements by pointer jumping in LDS, one workgroup
template <bool TWO>
__global__ void __launch_bounds__(1024) k_rank_top(uint32_t n, const uint32_t *__restrict__ nx_in, uint32_t *a_io, uint32_t *b_io)
{
	__shared__ uint32_t nx[RANK_TOP], sa[RANK_TOP], sb[TWO ? RANK_TOP : 1];
	for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
		const uint32_t p = nx_in[i] & PK_END;
		nx[i] = p == PK_END ? NIL : p;
		sa[i] = a_io[i];
		if (TWO)
			sb[i] = b_io[i];
	}
	__syncthreads();
	constexpr int PER = RANK_TOP / 1024;
	for (uint32_t span = 1; span < n; span <<= 1) {
		uint32_t tn[PER], ta[PER], tb[PER];
#pragma unroll
		for (int k = 0; k < PER; k++) {
			const uint32_t i = threadIdx.x + k * 1024;
			tn[k] = NIL, ta[k] = 0, tb[k] = 0;
			if (i < n && nx[i] != NIL) {
				const uint32_t j = nx[i];
				tn[k] = nx[j];
				ta[k] = sa[j];
				if (TWO)
					tb[k] = sb[j];
			}
		}
		__syncthreads();
#pragma unroll
		for (int k = 0; k < PER; k++) {
			const uint32_t i = threadIdx.x + k * 1024;
			if (i < n && nx[i] != NIL) {
				nx[i] = tn[k];
				sa[i] += ta[k];
				if (TWO)
					sb[i] += tb[k];
			}
		}
		__syncthreads();
	}
	for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
		a_io[i] = sa[i];
		if (TWO)
			b_io[i] = sb[i];
	}
}
// (top level too large for one workgroup -- graphs with very many tiny components: the old pointer jumping in global memory)
__global__ void k_rank_unpack_next(uint32_t n, const uint32_t *__restrict__ nx_in, uint32_t *__restrict__ out)
{
	uint32_t i = BIDX * blockDim.x + threadIdx.x;
	if (i < n) {
		const uint32_t p = nx_in[i] & PK_END;
		out[i] = p == PK_END ? NIL : p;
	}
}

static constexpr int RANK_MAX_LEVELS = 12;
// words every pool needs for lists of n elements in total with nh heads: the first level above the list has
// M = n / 2^b + nh elements (b >= 3), the following ones at least halve until the last, which may be as large as
// the one before it again -- < 3.2 M in all
size_t rank_pool_words(size_t n, size_t nh) { return n / 2 + 4 * nh + 64; }

// (debug hook povu_hip_debug_rank_escapes) What the level-0 walk left, counted after the fact by a walk of its own over the
// same segments: the elements it reaches, how many of their records carry REC_ESC, and the histogram of the widths their
// owner delta (zigzag) and partial sums need (RankRecStats).  out[0] = live, out[1] = escaped, out[2 + 33 d + p] = the histogram.
__device__ __forceinline__ uint32_t bit_width(uint32_t v) { return 32u - (uint32_t)__clz(v); }
template <bool EV>
__global__ void k_rank_rec_stats(RankLevelArgs A, unsigned b, const uint32_t *__restrict__ pk, const uint32_t *__restrict__ heads,
				 const uint32_t *__restrict__ w0, unsigned long long *__restrict__ out)
{
	__shared__ uint32_t h[2 + 33 * 33];
	for (uint32_t i = threadIdx.x; i < 2 + 33 * 33; i += blockDim.x)
		h[i] = 0;
	__syncthreads();
	for (uint32_t id = blockIdx.x * blockDim.x + threadIdx.x; id < A.M; id += gridDim.x * blockDim.x) {
		uint32_t x = rank_lane_start<true>(id, A, b, pk, heads);
		if (x == NIL)
			continue;
		uint32_t sa = 0, sb = 0;
		do {
			const uint32_t p = pk[x];
			uint32_t wa, wb;
			rank_l0_weights<EV>(x, p, wa, wb);
			const int32_t d = (int32_t)(id - (x >> b));
			const uint32_t zz = ((uint32_t)d << 1) ^ (uint32_t)(d >> 31);
			const uint32_t pw = EV ? max(bit_width(sa), bit_width(sa - sb)) : bit_width(sa);
			atomicAdd(&h[0], 1u);
			if (w0[x] & REC_ESC)
				atomicAdd(&h[1], 1u);
			atomicAdd(&h[2 + 33 * bit_width(zz) + pw], 1u);
			sa += wa;
			if constexpr (EV)
				sb += wb;
			x = p & P0_END;
		} while (!rank_l0_stop(x, b));
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < 2 + 33 * 33; i += blockDim.x)
		if (h[i])
			atomicAdd(&out[i], (unsigned long long)h[i]);
}
template <bool EV>
static void rank_rec_stats(const RankLevelArgs &A, unsigned b, const RankBufs &rb, const L0Ranks &R, RankRecStats &st, hipStream_t s)
{
	constexpr size_t W = 2 + 33 * 33;
	st = RankRecStats{};
	unsigned long long *d = nullptr;
	uint32_t fin = 0;
	std::vector<unsigned long long> hst(W);
	HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d), W * 8));
	try {
		HIP_CHECK(hipMemsetAsync(d, 0, W * 8, s));
		// (a block's LDS counters are 32 bits wide: at most 2048 blocks of 256 lanes, each lane over M / 2^19 segments)
		KLAUNCH((k_rank_rec_stats<EV>), dim3(std::min(nblk(A.M), 2048u)), dim3(TPB), 0, s, A, b, rb.pk, rb.heads, R.w0, d);
		HIP_CHECK(copy_async(hst.data(), d, W * 8, hipMemcpyDeviceToHost, s));
		if constexpr (EV)
			HIP_CHECK(copy_async(&fin, R.fin, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
	} catch (...) {
		(void)hipFree(d);
		throw;
	}
	HIP_CHECK(hipFree(d));
	st.valid = true;
	st.fin = fin;
	st.bits = b;
	st.delta_bits = EV ? REC_E_DBITS : REC_T_DBITS;
	st.part_bits[0] = EV ? REC_E_PBITS : REC_T_PBITS;
	st.part_bits[1] = EV ? REC_E_PBITS : 0u;
	st.live = hst[0];
	st.esc = fin ? hst[0] : hst[1];
	std::copy(hst.begin() + 2, hst.end(), st.hist);
}

// suffix sums (inclusive) along the lists packed in rb.pk, left as level-0 records rec[x] (k_rank_up) to be resolved
// by rank_l0 (the 0/1 weights) or rank_l0_pair (EV: the two sums of the events' weights; `ovf` = a device word for the
// overflow flag).  R stays valid until the pools are used again.
template <bool EV>
static L0Ranks list_rank_splitters(uint32_t n, unsigned b, uint2 *rec_arr, uint32_t *ovf, uint32_t nh, RankBufs &rb, hipStream_t s,
				   RankRecStats *st)
{
	const RecPlanes rec = rec_planes(rec_arr, n);
	if (n >= P0_END)
		throw HipError("list ranking: more than 2^30 elements (graph too large for the packed walk)");
	// plan: level L has lv[L].n elements; its walk has lv[L].M lanes = the elements of level L + 1
	RankLevelArgs lv[RANK_MAX_LEVELS];
	uint32_t *nxp[RANK_MAX_LEVELS + 1], *wap[RANK_MAX_LEVELS + 1], *wbp[RANK_MAX_LEVELS + 1];
	int levels = 0;
	size_t used = 0;
	const size_t pool = rank_pool_words(n, nh);
	nxp[0] = rb.pk, wap[0] = wbp[0] = nullptr;
	uint32_t cur_n = n, hbase = 0;
	for (;;) {
		RankLevelArgs &A = lv[levels];
		A.n = cur_n;
		A.m = (cur_n + (1u << b) - 1) >> b;
		A.hbase = hbase;
		A.M = A.m + nh;
		if (used + A.M > pool)
			throw HipError("list ranking: level pool exhausted (internal sizing bug)");
		nxp[levels + 1] = rb.nx + used, wap[levels + 1] = rb.wa + used, wbp[levels + 1] = rb.wb + used;
		used += A.M;
		levels++;
		hbase = A.m;
		const uint32_t next_n = A.M;
		// stop when one workgroup can finish, or when the heads keep the levels from shrinking
		if (next_n <= RANK_TOP || next_n > cur_n / 2 || levels == RANK_MAX_LEVELS) {
			cur_n = next_n;
			break;
		}
		cur_n = next_n;
	}
	if constexpr (EV)
		HIP_CHECK(hipMemsetAsync(ovf, 0, 4, s));
	for (int L = 0; L < levels; L++) {
		const RankLevelArgs &A = lv[L];
		if (L == 0)
			LAUNCH((k_rank_up<true, EV>), A.M, s, A, b, nxp[0], nullptr, nullptr, rb.heads, nxp[1], wap[1], wbp[1], rec, ovf);
		else
			LAUNCH((k_rank_up<false, EV>), A.M, s, A, b, nxp[L], wap[L], wbp[L], nullptr, nxp[L + 1], wap[L + 1], wbp[L + 1],
			       RecPlanes{nullptr, nullptr}, nullptr);
	}
	const uint32_t nt = cur_n; // elements of the top level
	if (nt <= RANK_TOP) {
		KLAUNCH((k_rank_top<EV>), dim3(1), dim3(1024), 0, s, nt, nxp[levels], wap[levels], wbp[levels]);
	} else {
		LAUNCH(k_rank_unpack_next, nt, s, nt, nxp[levels], rb.tA);
		HIP_CHECK(copy_async(rb.tB, wap[levels], (size_t)nt * 4, hipMemcpyDeviceToDevice, s));
		if constexpr (EV)
			HIP_CHECK(copy_async(rb.tC, wbp[levels], (size_t)nt * 4, hipMemcpyDeviceToDevice, s));
		// ping-pong partners: the level's own arrays (their contents were just copied out)
		uint32_t *nA = rb.tA, *nB = nxp[levels], *aA = rb.tB, *aB = wap[levels], *bA = rb.tC, *bB = wbp[levels];
		const int side = list_rank(nt, bits_for(nt) + 1, nA, nB, aA, aB, EV ? bA : nullptr, EV ? bB : nullptr, s);
		if (side == 0) { // result in the A set: bring it home
			HIP_CHECK(copy_async(wap[levels], aA, (size_t)nt * 4, hipMemcpyDeviceToDevice, s));
			if constexpr (EV)
				HIP_CHECK(copy_async(wbp[levels], bA, (size_t)nt * 4, hipMemcpyDeviceToDevice, s));
		}
	}
	// (level 0 has no way back: its records are resolved where they are read)
	for (int L = levels - 1; L >= 1; L--) {
		const RankLevelArgs &A = lv[L];
		LAUNCH((k_rank_down<EV>), A.M, s, A, b, nxp[L], wap[L], wbp[L], wap[L + 1], wbp[L + 1]);
	}
	if constexpr (EV)
		KLAUNCH((k_rank_l0_fallback), dim3(std::min(nblk(lv[0].M), 2048u)), dim3(TPB), 0, s, lv[0], b, rb.pk, rb.heads, wap[1],
			wbp[1], rec, ovf);
	const L0Ranks R{wap[1], EV ? wbp[1] : nullptr, EV ? ovf : nullptr, lv[0].M, rec.w0, rec.w1, b};
	if (st)
		rank_rec_stats<EV>(lv[0], b, rb, R, *st, s);
	return R;
}

L0Ranks rank_tour(uint32_t n, unsigned b, uint2 *rec, uint32_t nh, RankBufs &rb, hipStream_t s, RankRecStats *st)
{
	return list_rank_splitters<false>(n, b, rec, nullptr, nh, rb, s, st);
}
L0Ranks rank_events(uint32_t n, unsigned b, uint2 *rec, uint32_t *ovf, uint32_t nh, RankBufs &rb, hipStream_t s, RankRecStats *st)
{
	return list_rank_splitters<true>(n, b, rec, ovf, nh, rb, s, st);
}

// (unit-test hook, debug_list_rank) every element's rank resolved from its record, as the readers do
template <bool TWO>
__global__ void k_rank_resolve(uint32_t n, L0Ranks R, uint32_t *__restrict__ ra, uint32_t *__restrict__ rb)
{
	const uint32_t x = BIDX * blockDim.x + threadIdx.x;
	if (x >= n)
		return;
	if (TWO) {
		const uint2 r = rank_l0_pair_of(R, x, *R.fin != 0);
		ra[x] = r.x;
		rb[x] = r.y;
	} else {
		ra[x] = rank_l0_of(R, x);
	}
}
void debug_list_rank(uint32_t n, const uint32_t *next, const uint8_t *w, const uint32_t *heads, uint32_t nh, int mode,
		     unsigned bits, uint32_t *ra, uint32_t *rb, hipStream_t s, RankRecStats *st, std::vector<uint32_t> *plane0)
{
	if (n == 0 || n >= P0_END)
		throw HipError("debug_list_rank: n must be in [1, 2^30)");
	const unsigned b = bits ? std::min(6u, std::max(2u, bits)) : rank_bucket_bits(read_pass_hooks()); // (a debug hook outside any pass)
	std::vector<uint32_t> pk(n);
	for (uint32_t x = 0; x < n; x++) {
		if (next[x] != NIL && next[x] >= n)
			throw HipError("debug_list_rank: successor out of range");
		pk[x] = rank_pack(next[x], w[x] ? 1u : 0u);
	}
	for (uint32_t h = 0; h < nh; h++)
		if (heads[h] != NIL) {
			if (heads[h] >= n)
				throw HipError("debug_list_rank: head out of range");
			pk[heads[h]] |= P0_HEAD;
		}
	const size_t pool = rank_pool_words(n, nh);
	Arena ar;
	ar.reserve(Arena::padded(n + 16, 4) * 3 + Arena::padded(n + 16, 8) + Arena::padded(nh + 1, 4) + 6 * Arena::padded(pool, 4) + 8192, false);
	RankBufs rbf{};
	rbf.pk = ar.take<uint32_t>(n + 16);
	rbf.heads = ar.take<uint32_t>(nh + 1);
	for (uint32_t **q : {&rbf.nx, &rbf.wa, &rbf.wb, &rbf.tA, &rbf.tB, &rbf.tC})
		*q = ar.take<uint32_t>(pool);
	uint32_t *da = ar.take<uint32_t>(n + 16), *db = ar.take<uint32_t>(n + 16), *ovf = ar.take<uint32_t>(4);
	uint2 *rec = ar.take<uint2>(n + 16);
	HIP_CHECK(copy_async(rbf.pk, pk.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
	if (nh)
		HIP_CHECK(copy_async(rbf.heads, heads, (size_t)nh * 4, hipMemcpyHostToDevice, s));
	if (mode == 0) {
		const L0Ranks R = rank_tour(n, b, rec, nh, rbf, s, st);
		LAUNCH(k_rank_resolve<false>, n, s, n, R, da, nullptr);
	} else {
		const L0Ranks R = rank_events(n, b, rec, ovf, nh, rbf, s, st);
		LAUNCH(k_rank_resolve<true>, n, s, n, R, da, db);
	}
	if (plane0) {
		plane0->resize(n);
		HIP_CHECK(copy_async(plane0->data(), rec, (size_t)n * 4, hipMemcpyDeviceToHost, s));
	}
	HIP_CHECK(copy_async(ra, da, (size_t)n * 4, hipMemcpyDeviceToHost, s));
	if (mode != 0)
		HIP_CHECK(copy_async(rb, db, (size_t)n * 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
}

} // namespace povu_hip
