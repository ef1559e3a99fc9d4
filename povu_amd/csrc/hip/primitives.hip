// primitives.hip -- device-wide primitives between the decompose kernels: exclusive scans and the stable radix sort
// of (key, value) pairs, all hand-written.
//
// The u32 scans (sum / max / xor) share one description of their input and one way to read it.  A ScanSrc says whether a
// job's elements are words or single BYTES, and whether a word array `sub` -- or, under a byte job, a byte array `sub8` -- is
// subtracted element by element (sums only).
// sc_load<Q> loads Q sub-tiles of SC_ITEMS consecutive elements a lane: whole sub-tiles with 16-byte (words) or 8-byte
// (bytes) loads that are ALL issued before the first is used, anything else element by element with zeros behind the end;
// the byte unpack (sc_unpack4) and the `- sub` step exist there and nowhere else.  Q = 1 is a tile of the two-launch form
// (k_scan_chunks), Q = LB_SUB the tile of the one-launch form (k_scan_lookback); sc_store writes a sub-tile back.  The
// reduction k_scan_partials reads 16 bytes a lane and load instead and selects words / bytes / sub the same way.  A new
// input form is a line in ScanSrc, sc_load and k_scan_partials.  The scans inside a wave and a workgroup are the helpers
// of common.hpp, as in every other kernel of this file.
// Two output forms ride on the same loader, lane scan, store, kernels and host driver: an INCLUSIVE job (a flag of the job:
// the lane scan leaves the inclusive sums) and the count-record scan (template parameter REC, see ScLane: twelve byte
// counts a lane and sub-tile, the record of common.hpp's cntrec_prefix written instead of twelve words).
#include "common.hpp"

namespace povu_hip
{

// ---- exclusive scans (sum / max / xor) of u32, two launches: per-chunk partials, then every block adds the
// partials in front of it and scans its own chunk tile by tile (8 elements per lane, wave shuffles,
// one LDS exchange per tile).  The arrays here are 1-30 M elements; the second read of the input comes
// from L2 / Infinity Cache.
static constexpr int SC_TPB = 256, SC_WAVES = SC_TPB / 64, SC_ITEMS = 8, SC_TILE = SC_TPB * SC_ITEMS, SC_MAX_BLOCKS = 1024;
// What a lane holds of a sub-tile.  REC = false: SC_ITEMS elements, one a word, scanned in the lane and written back as
// words.  REC = true (the count-record scan, byte jobs only): the CNTREC_N = 12 count bytes of ONE record exactly as they
// were loaded (three words) -- the record takes them as they are and the sum in front of the lane, so nothing is unpacked
// and only the lane's total is worked out.
template <bool REC>
struct ScLane {
	static constexpr int ITEMS = REC ? (int)CNTREC_N : SC_ITEMS, REGS = REC ? 3 : SC_ITEMS, TILE = SC_TPB * ITEMS;
};
struct ScBytes12 {
	uint32_t x, y, z;
};

// what a job scans: words, or one BYTE per element (flags, small counts -- a quarter of the reads); with `sub` (sum scans)
// the element is in[i] - sub[i]
// (sub8: the subtrahend as BYTES, for a byte job only; the difference still wraps mod 2^32 as with words)
struct ScanSrc {
	const void *in;
	const uint32_t *sub;
	bool bytes;
	const uint8_t *sub8 = nullptr;
	static ScanSrc words(const uint32_t *p, const uint32_t *sub = nullptr) { return ScanSrc{p, sub, false}; }
	static ScanSrc of_bytes(const uint8_t *p, const uint32_t *sub = nullptr) { return ScanSrc{p, sub, true}; }
	static ScanSrc bytes_minus_bytes(const uint8_t *p, const uint8_t *sub8) { return ScanSrc{p, nullptr, true, sub8}; }
	__device__ __forceinline__ const uint32_t *w() const { return static_cast<const uint32_t *>(in); }
	__device__ __forceinline__ const uint8_t *b() const { return static_cast<const uint8_t *>(in); }
	__device__ __forceinline__ uint32_t operator[](size_t i) const
	{
		return (bytes ? (uint32_t)b()[i] : w()[i]) - (sub ? sub[i] : sub8 ? (uint32_t)sub8[i] : 0u);
	}
};
// One scan job; a launch carries one or two of them (blockIdx.y picks) so that independent scans that
// are due at the same point of the pass share their two launches.
struct ScanJob {
	ScanSrc src;
	uint32_t *out;
	size_t n, chunk;
	uint32_t blocks;
	uint32_t *partial;
	bool inclusive; // out[i] takes element i in as well (sc_lane_scan)
	// single-launch form (k_scan_lookback): tiles of LB_TILE elements, one status word a tile, handed out by a ticket
	uint32_t tiles;
	unsigned long long *status;
	uint32_t *ticket;
};
struct ScanJobs {
	ScanJob j[2];
};
// the four one-byte elements of a word
__device__ __forceinline__ void sc_unpack4(uint32_t w, uint32_t *v) { v[0] = w & 0xFFu, v[1] = (w >> 8) & 0xFFu, v[2] = (w >> 16) & 0xFFu, v[3] = w >> 24; }
__device__ __forceinline__ void sc_minus4(uint32_t *v, const uint4 c) { v[0] -= c.x, v[1] -= c.y, v[2] -= c.z, v[3] -= c.w; }
template <int OP>
__device__ __forceinline__ uint32_t sc_fold4(const uint32_t *v)
{
	const ScanOp<OP> op;
	return op(op(v[0], v[1]), op(v[2], v[3]));
}
template <int OP>
__global__ void __launch_bounds__(SC_TPB) k_scan_partials(const ScanJobs jobs)
{
	__shared__ uint32_t sh[SC_WAVES];
	const ScanJob &J = jobs.j[blockIdx.y];
	if (blockIdx.x >= J.blocks)
		return;
	const ScanOp<OP> op;
	const ScanSrc S = J.src;
	const uint32_t *__restrict__ sub = S.sub;
	const size_t n = J.n, chunk = J.chunk;
	const size_t b0 = (size_t)blockIdx.x * chunk, b1 = b0 + chunk < n ? b0 + chunk : n;
	uint32_t acc = 0;
	// chunks start on multiples of the tile and every operand is 16-byte aligned: sixteen bytes per load (four words, or
	// sixteen one-byte elements), the tail of the last chunk element by element
	size_t w1;
	if (S.bytes) {
		const uint8_t *__restrict__ in8 = S.b();
		w1 = b0 + ((b1 - b0) & ~size_t(15));
		for (size_t i = b0 + 16 * (size_t)threadIdx.x; i < w1; i += 16 * SC_TPB) {
			const uint4 a = *reinterpret_cast<const uint4 *>(in8 + i);
			const uint32_t w[4] = {a.x, a.y, a.z, a.w};
			uint32_t f[4];
#pragma unroll
			for (int q = 0; q < 4; q++) {
				uint32_t v[4];
				sc_unpack4(w[q], v);
				f[q] = sc_fold4<OP>(v);
			}
			acc = op(acc, sc_fold4<OP>(f));
			if (sub) { // (sums only: the total of the differences is the difference of the totals)
#pragma unroll
				for (int q = 0; q < 4; q++) {
					const uint4 c = *reinterpret_cast<const uint4 *>(sub + i + 4 * q);
					acc -= c.x + c.y + c.z + c.w;
				}
			} else if (S.sub8) {
				const uint4 c = *reinterpret_cast<const uint4 *>(S.sub8 + i);
				const uint32_t cw[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
				for (int q = 0; q < 4; q++) {
					uint32_t v[4];
					sc_unpack4(cw[q], v);
					acc -= sc_fold4<0>(v);
				}
			}
		}
	} else {
		const uint32_t *__restrict__ in = S.w();
		w1 = b0 + ((b1 - b0) & ~size_t(3));
		if (sub) {
			for (size_t i = b0 + 4 * (size_t)threadIdx.x; i < w1; i += 4 * SC_TPB) {
				const uint4 a = *reinterpret_cast<const uint4 *>(in + i);
				uint32_t v[4] = {a.x, a.y, a.z, a.w};
				sc_minus4(v, *reinterpret_cast<const uint4 *>(sub + i));
				acc = op(acc, sc_fold4<OP>(v));
			}
		} else {
			for (size_t i = b0 + 4 * (size_t)threadIdx.x; i < w1; i += 4 * SC_TPB) {
				const uint4 a = *reinterpret_cast<const uint4 *>(in + i);
				const uint32_t v[4] = {a.x, a.y, a.z, a.w};
				acc = op(acc, sc_fold4<OP>(v));
			}
		}
	}
	for (size_t i = w1 + threadIdx.x; i < b1; i += SC_TPB)
		acc = op(acc, S[i]);
	acc = block_reduce<SC_WAVES>(acc, sh, op);
	if (threadIdx.x == 0)
		J.partial[blockIdx.x] = acc;
}
// The lane's SC_ITEMS consecutive elements of each of the Q sub-tiles (SC_TILE elements each) that start at t0 (zeros behind
// b1).  Whole -- all Q sub-tiles of the workgroup (a uniform test), or for a single one the lane's own elements --: every load
// of the lane is issued before the first is needed
template <int Q, bool REC = false>
__device__ __forceinline__ void sc_load(const ScanSrc &S, size_t t0, size_t b1, uint32_t (*v)[ScLane<REC>::REGS])
{
	constexpr int SC_ITEMS = ScLane<REC>::ITEMS, SC_TILE = ScLane<REC>::TILE;
	const size_t e0 = t0 + (size_t)threadIdx.x * SC_ITEMS;
	if (Q > 1 ? t0 + (size_t)Q * SC_TILE <= b1 : e0 + SC_ITEMS <= b1) {
		if constexpr (REC) { // a record's twelve bytes in one three-word load (tile bases are multiples of 16, e0 of 4)
			const uint8_t *__restrict__ in8 = S.b() + e0;
			ScBytes12 a[Q];
#pragma unroll
			for (int q = 0; q < Q; q++)
				a[q] = *reinterpret_cast<const ScBytes12 *>(in8 + q * SC_TILE);
#pragma unroll
			for (int q = 0; q < Q; q++)
				v[q][0] = a[q].x, v[q][1] = a[q].y, v[q][2] = a[q].z;
			return;
		} else if (S.bytes) {
			const uint8_t *__restrict__ in8 = S.b() + e0;
			uint2 a[Q];
#pragma unroll
			for (int q = 0; q < Q; q++)
				a[q] = *reinterpret_cast<const uint2 *>(in8 + q * SC_TILE);
#pragma unroll
			for (int q = 0; q < Q; q++)
				sc_unpack4(a[q].x, v[q]), sc_unpack4(a[q].y, v[q] + 4);
		} else {
			const uint32_t *__restrict__ in = S.w() + e0;
			uint4 a[Q][2];
#pragma unroll
			for (int q = 0; q < Q; q++)
				a[q][0] = *reinterpret_cast<const uint4 *>(in + q * SC_TILE), a[q][1] = *reinterpret_cast<const uint4 *>(in + q * SC_TILE + 4);
#pragma unroll
			for (int q = 0; q < Q; q++) {
				v[q][0] = a[q][0].x, v[q][1] = a[q][0].y, v[q][2] = a[q][0].z, v[q][3] = a[q][0].w;
				v[q][4] = a[q][1].x, v[q][5] = a[q][1].y, v[q][6] = a[q][1].z, v[q][7] = a[q][1].w;
			}
		}
		if (S.sub) {
			const uint32_t *__restrict__ sub = S.sub + e0;
#pragma unroll
			for (int q = 0; q < Q; q++) {
				const uint4 c = *reinterpret_cast<const uint4 *>(sub + q * SC_TILE), d = *reinterpret_cast<const uint4 *>(sub + q * SC_TILE + 4);
				sc_minus4(v[q], c), sc_minus4(v[q] + 4, d);
			}
		} else if (S.sub8) {
			const uint8_t *__restrict__ sub8 = S.sub8 + e0;
			uint2 c[Q];
#pragma unroll
			for (int q = 0; q < Q; q++)
				c[q] = *reinterpret_cast<const uint2 *>(sub8 + q * SC_TILE);
#pragma unroll
			for (int q = 0; q < Q; q++) {
				uint32_t m[SC_ITEMS];
				sc_unpack4(c[q].x, m), sc_unpack4(c[q].y, m + 4);
				sc_minus4(v[q], make_uint4(m[0], m[1], m[2], m[3])), sc_minus4(v[q] + 4, make_uint4(m[4], m[5], m[6], m[7]));
			}
		}
	} else if constexpr (Q > 1) { // the job's last tile: sub-tile by sub-tile
#pragma unroll
		for (int q = 0; q < Q; q++)
			sc_load<1, REC>(S, t0 + (size_t)q * SC_TILE, b1, v + q);
	} else if constexpr (REC) { // (the count bytes behind the end of the array are zero)
		v[0][0] = v[0][1] = v[0][2] = 0u;
#pragma unroll
		for (int k = 0; k < SC_ITEMS; k++)
			v[0][k >> 2] |= (e0 + k < b1 ? (uint32_t)S.b()[e0 + k] : 0u) << (8 * (k & 3));
	} else {
		for (int k = 0; k < SC_ITEMS; k++)
			v[0][k] = e0 + k < b1 ? S[e0 + k] : 0u;
	}
}
// the lane's exclusive (incl: inclusive) scan of its own elements, in place; returns their total
// (REC: the total only, the count bytes stay as they are)
template <int OP, bool REC = false>
__device__ __forceinline__ uint32_t sc_lane_scan(uint32_t (&v)[ScLane<REC>::REGS], bool incl)
{
	if constexpr (REC) {
		return cntrec_bytesum(v[2], cntrec_bytesum(v[1], cntrec_bytesum(v[0], 0u)));
	} else {
		uint32_t tot = 0;
#pragma unroll
		for (int k = 0; k < SC_ITEMS; k++) {
			const uint32_t x = v[k], nt = ScanOp<OP>{}(tot, x);
			v[k] = incl ? nt : tot;
			tot = nt;
		}
		return tot;
	}
}
// a scanned sub-tile back: pre = everything in front of the lane, v = the lane's own exclusive scan
// (an inclusive job's v already holds the inclusive sums; REC: the lane's record = its count bytes and pre, out an array of
// records -- every record that holds an element of [0, b1) is written, whole)
template <int OP, bool REC = false>
__device__ __forceinline__ void sc_store(uint32_t *__restrict__ out, size_t e0, size_t b1, uint32_t pre, const uint32_t (&v)[ScLane<REC>::REGS])
{
	const ScanOp<OP> op;
	if constexpr (REC) {
		if (e0 < b1)
			reinterpret_cast<uint4 *>(out)[e0 / CNTREC_N] = make_uint4(v[0], v[1], v[2], pre);
	} else if (e0 + SC_ITEMS <= b1) {
		*reinterpret_cast<uint4 *>(out + e0) = make_uint4(op(pre, v[0]), op(pre, v[1]), op(pre, v[2]), op(pre, v[3]));
		*reinterpret_cast<uint4 *>(out + e0 + 4) = make_uint4(op(pre, v[4]), op(pre, v[5]), op(pre, v[6]), op(pre, v[7]));
	} else {
		for (int k = 0; k < SC_ITEMS; k++)
			if (e0 + k < b1)
				out[e0 + k] = op(pre, v[k]);
	}
}
template <int OP, bool REC>
__global__ void __launch_bounds__(SC_TPB) k_scan_chunks(const ScanJobs jobs)
{
	constexpr int SC_ITEMS = ScLane<REC>::ITEMS, SC_TILE = ScLane<REC>::TILE, REGS = ScLane<REC>::REGS;
	__shared__ uint32_t sh[SC_WAVES];
	__shared__ uint32_t wave_tot[SC_WAVES];
	const ScanJob &J = jobs.j[blockIdx.y];
	if (blockIdx.x >= J.blocks)
		return;
	const ScanOp<OP> op;
	uint32_t *__restrict__ out = J.out;
	const uint32_t *__restrict__ partial = J.partial;
	const size_t n = J.n, chunk = J.chunk;
	uint32_t base = 0;
	for (uint32_t k = threadIdx.x; k < blockIdx.x; k += SC_TPB)
		base = op(base, partial[k]);
	uint32_t carry = block_reduce<SC_WAVES>(base, sh, op);
	const size_t b0 = (size_t)blockIdx.x * chunk, b1 = b0 + chunk < n ? b0 + chunk : n;
	// the next tile's loads are issued before this tile's exchange through LDS: two tiles of a block are in flight
	uint32_t v[REGS], nx[REGS];
	const bool incl = J.inclusive;
	if (b0 < b1)
		sc_load<1, REC>(J.src, b0, b1, &v);
	for (size_t t0 = b0; t0 < b1; t0 += SC_TILE) {
		const size_t e0 = t0 + (size_t)threadIdx.x * SC_ITEMS;
		const bool more = t0 + SC_TILE < b1;
		if (more)
			sc_load<1, REC>(J.src, t0 + SC_TILE, b1, &nx);
		const uint32_t tot = sc_lane_scan<OP, REC>(v, incl);
		uint32_t tile_tot;
		const uint32_t pre = op(carry, block_exclusive_scan<SC_WAVES>(tot, wave_tot, tile_tot, op)); // carry, earlier waves, earlier lanes
		sc_store<OP, REC>(out, e0, b1, pre, v);
		carry = op(carry, tile_tot);
		__syncthreads();
		if (more)
			for (int k = 0; k < REGS; k++)
				v[k] = nx[k];
	}
}

// ---- the same scans in ONE launch and one read of the input (decoupled look-back).  A workgroup takes a ticket = its
// tile (LB_TILE elements, all loaded up front: 64 a lane), publishes the tile's aggregate, then its first wave looks back
// over the status words of the tiles in front of it, 64 at a time -- aggregates are added up until a tile is met that
// already knows its inclusive prefix --, publishes its own inclusive prefix and the workgroup writes the tile out.  A tile
// only ever waits for tiles with smaller tickets, i.e. for workgroups that are already running: no assumption about the
// order workgroups are dispatched in.  Value and state of a tile share one 64-bit word (read and written with
// agent-scope atomics: the L2 of another XCD never serves a stale one), so no fence orders anything.  The two-launch form
// above reads its input twice (4.3 GB of the 170 GB a whole-genome pass moved in round 5, and 1.05 ms for the partials).
// (Other tilings and ticket-free forms were measured and dropped: DESIGN.md section 4, "Scans ... in one launch".)
static constexpr unsigned long long LB_AGG = 1ull << 32, LB_PREFIX = 2ull << 32;
static constexpr int LB_SUB = 8, LB_TILE = SC_TILE * LB_SUB;
template <int OP, bool REC>
__global__ void __launch_bounds__(SC_TPB) k_scan_lookback(const ScanJobs jobs)
{
	constexpr int SC_ITEMS = ScLane<REC>::ITEMS, SC_TILE = ScLane<REC>::TILE, LB_TILE = SC_TILE * LB_SUB;
	__shared__ uint32_t wave_tot[LB_SUB][SC_WAVES];
	__shared__ uint32_t s_tile, s_carry;
	const ScanJob &J = jobs.j[blockIdx.y];
	if (blockIdx.x >= J.tiles)
		return;
	const ScanOp<OP> op;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t t = blockIdx.x;
	if (J.tiles > 1) { // (uniform: a one-tile job needs neither ticket nor status)
		if (threadIdx.x == 0)
			s_tile = atomicAdd(J.ticket, 1u);
		__syncthreads();
		t = s_tile;
	}
	const size_t b0 = (size_t)t * LB_TILE, b1 = b0 + LB_TILE < J.n ? b0 + LB_TILE : J.n;
	uint32_t v[LB_SUB][ScLane<REC>::REGS], before[LB_SUB];
	const bool incl = J.inclusive;
	sc_load<LB_SUB, REC>(J.src, b0, b1, v);
#pragma unroll
	for (int q = 0; q < LB_SUB; q++) {
		const uint32_t tot = sc_lane_scan<OP, REC>(v[q], incl);
		before[q] = op.before(wave_scan_publish(tot, wave_tot[q], op), tot); // the earlier lanes of the wave
	}
	__syncthreads();
	if (wave == 0) {
		uint32_t agg = 0;
#pragma unroll
		for (int q = 0; q < LB_SUB; q++)
#pragma unroll
			for (int w = 0; w < SC_WAVES; w++)
				agg = op(agg, wave_tot[q][w]);
		uint32_t carry = 0;
		if (t > 0) {
			if (lane == 0)
				__hip_atomic_store(J.status + t, LB_AGG | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			for (int64_t base = (int64_t)t - 1;;) {
				const int64_t idx = base - lane;
				// (in front of tile 0: an inclusive prefix of nothing)
				const unsigned long long w = idx >= 0 ? __hip_atomic_load(J.status + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : LB_PREFIX;
				const unsigned long long has_p = __ballot((w >> 32) == 2ull), unset = __ballot((w >> 32) == 0ull);
				const int stop = has_p ? __ffsll((long long)has_p) - 1 : 64; // nearest tile that knows its prefix
				const unsigned long long need = stop >= 63 ? ~0ull : ((2ull << stop) - 1ull);
				if (unset & need)
					continue; // some tile up to there has not published yet: its workgroup is running, read again
				const uint32_t x = wave_reduce(lane <= stop ? (uint32_t)w : 0u, op);
				carry = op(carry, __shfl(x, 0));
				if (has_p)
					break;
				base -= 64;
			}
		}
		if (lane == 0) {
			if (J.tiles > 1)
				__hip_atomic_store(J.status + t, LB_PREFIX | op(carry, agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			s_carry = carry;
		}
	}
	__syncthreads();
	uint32_t pre_sub = s_carry; // everything in front of the sub-tile
#pragma unroll
	for (int q = 0; q < LB_SUB; q++) {
		uint32_t sub_tot;
		const uint32_t pre = op(op(pre_sub, waves_before<SC_WAVES>(wave_tot[q], sub_tot, op)), before[q]);
		sc_store<OP, REC>(J.out, b0 + (size_t)q * SC_TILE + (size_t)threadIdx.x * SC_ITEMS, b1, pre, v[q]);
		pre_sub = op(pre_sub, sub_tot);
	}
}

static constexpr size_t SC_LEGACY_BYTES = SC_MAX_BLOCKS * 16 + 256; // (two u32 jobs of the two-launch form, or one job of 128-bit words)
// below this many elements the two-launch form is the faster one: its second read comes out of the Infinity Cache
// (10^7 words: 0.023 ms against 0.035) -- except when every job fits one tile (one launch instead of two, no fill)
static constexpr size_t LB_MIN = 48u << 20;
static size_t lb_tiles(size_t n, size_t tile = LB_TILE) { return (n + tile - 1) / tile; }
static size_t lb_job_bytes(size_t n) { return 16 + 8 * lb_tiles(n); } // ticket (+ padding), status words (a record job's larger tiles need fewer)
size_t scan_tmp_bytes(size_t n)
{
	return SC_LEGACY_BYTES + 2 * lb_job_bytes(n) + 64; // the partials of the two-launch form, then ticket + status words of two jobs
}
// one or two jobs in one launch; false: the temporary storage was sized for fewer elements (the caller takes two launches)
template <int OP, bool REC>
static bool scan_lookback(ScanJobs &jobs, int nj, void *tmp, size_t tmp_bytes, hipStream_t s)
{
	static const bool off = getenv("POVU_HIP_SCAN_TWO_LAUNCH") != nullptr; // (A/B hook)
	if (off)
		return false;
	size_t need = SC_LEGACY_BYTES, clear = 0;
	unsigned gx = 0;
	char *at = static_cast<char *>(tmp) + SC_LEGACY_BYTES;
	for (int j = 0; j < nj; j++) {
		ScanJob &J = jobs.j[j];
		const size_t tiles = lb_tiles(J.n, (size_t)ScLane<REC>::TILE * LB_SUB);
		if (tiles > 0xFFFFFFF0ull)
			return false;
		J.tiles = (uint32_t)tiles;
		J.ticket = reinterpret_cast<uint32_t *>(at);
		J.status = reinterpret_cast<unsigned long long *>(at + 16);
		at += lb_job_bytes(J.n);
		need += lb_job_bytes(J.n);
		if (tiles > 1)
			clear = need - SC_LEGACY_BYTES; // (the jobs lie back to back: one fill covers every job that needs one)
		gx = std::max<unsigned>(gx, J.tiles);
	}
	if (need > tmp_bytes)
		return false;
	size_t n_max = 0;
	for (int j = 0; j < nj; j++)
		n_max = std::max(n_max, jobs.j[j].n);
	if (clear && n_max < LB_MIN)
		return false;
	if (clear)
		HIP_CHECK(hipMemsetAsync(static_cast<char *>(tmp) + SC_LEGACY_BYTES, 0, clear, s));
	KLAUNCH((k_scan_lookback<OP, REC>), dim3(gx, nj), dim3(SC_TPB), 0, s, jobs);
	return true;
}

struct ScanReq {
	ScanSrc src;
	uint32_t *out;
	size_t n;
	bool inclusive = false;
};
static ScanJob make_scan_job(const ScanReq &r, uint32_t *partial, size_t SC_TILE)
{
	if ((reinterpret_cast<uintptr_t>(r.src.in) | reinterpret_cast<uintptr_t>(r.src.sub) | reinterpret_cast<uintptr_t>(r.out)) & 15)
		throw HipError("scan: operands must be 16-byte aligned");
	size_t blocks = (r.n + SC_TILE - 1) / SC_TILE;
	if (blocks > SC_MAX_BLOCKS)
		blocks = SC_MAX_BLOCKS;
	size_t chunk = (r.n + blocks - 1) / blocks;
	chunk = (chunk + SC_TILE - 1) / SC_TILE * SC_TILE; // whole tiles: every tile base stays 16-byte aligned
	blocks = (r.n + chunk - 1) / chunk;
	return ScanJob{r.src, r.out, r.n, chunk, (uint32_t)blocks, partial, r.inclusive, 0u, nullptr, nullptr};
}
// the host side of every u32 scan: one job, or two in the same launches.  An empty job is left out, so a pair with one
// is a single job; the one-launch form where it applies, else partials and chunks
// (REC: byte jobs whose outputs are count records, see ScLane)
template <int OP, bool REC = false>
static void scan_run(const ScanReq &r0, const ScanReq &r1, void *tmp, size_t tmp_bytes, hipStream_t s)
{
	ScanJobs jobs{};
	unsigned nj = 0, gx = 0;
	for (const ScanReq *r : {&r0, &r1})
		if (r->n) {
			if (tmp_bytes < (nj + 1) * SC_MAX_BLOCKS * sizeof(uint32_t))
				throw HipError("scan: temporary storage too small");
			jobs.j[nj] = make_scan_job(*r, static_cast<uint32_t *>(tmp) + nj * SC_MAX_BLOCKS, ScLane<REC>::TILE);
			gx = std::max(gx, jobs.j[nj++].blocks);
		}
	if (!nj || scan_lookback<OP, REC>(jobs, (int)nj, tmp, tmp_bytes, s))
		return;
	KLAUNCH(k_scan_partials<OP>, dim3(gx, nj), dim3(SC_TPB), 0, s, jobs);
	KLAUNCH((k_scan_chunks<OP, REC>), dim3(gx, nj), dim3(SC_TPB), 0, s, jobs);
}
static constexpr ScanReq SC_NONE{};

void scan_exclusive_u32(const uint32_t *in, uint32_t *out, size_t n, void *tmp, size_t tmp_bytes, hipStream_t s)
{
	scan_run<0>({ScanSrc::words(in), out, n}, SC_NONE, tmp, tmp_bytes, s);
}
void scan_inclusive_u32(const uint32_t *in, uint32_t *out, size_t n, void *tmp, size_t tmp_bytes, hipStream_t s)
{
	scan_run<0>({ScanSrc::words(in), out, n, true}, SC_NONE, tmp, tmp_bytes, s);
}
void scan_exclusive_max_u32(const uint32_t *in, uint32_t *out, size_t n, void *tmp, size_t tmp_bytes, hipStream_t s)
{
	scan_run<1>({ScanSrc::words(in), out, n}, SC_NONE, tmp, tmp_bytes, s);
}
void scan_exclusive_diff_u32(const uint32_t *in, const uint32_t *sub, uint32_t *out, size_t n, void *tmp, size_t tmp_bytes,
			     hipStream_t s)
{
	scan_run<0>({ScanSrc::words(in, sub), out, n}, SC_NONE, tmp, tmp_bytes, s);
}
void scan_exclusive_diff_u8_u32(const uint8_t *in8, const uint32_t *sub, uint32_t *out, size_t n, void *tmp, size_t tmp_bytes,
				hipStream_t s)
{
	scan_run<0>({ScanSrc::of_bytes(in8, sub), out, n}, SC_NONE, tmp, tmp_bytes, s);
}
void scan_exclusive_diff_u8_u8(const uint8_t *in8, const uint8_t *sub8, uint32_t *out, size_t n, void *tmp, size_t tmp_bytes,
			       hipStream_t s)
{
	scan_run<0>({ScanSrc::bytes_minus_bytes(in8, sub8), out, n}, SC_NONE, tmp, tmp_bytes, s);
}
// byte inputs: one or two independent jobs in the same launches (in1 may be null)
void scan_exclusive_u8(const uint8_t *in0, uint32_t *out0, size_t n0, const uint8_t *in1, uint32_t *out1, size_t n1, void *tmp,
		       size_t tmp_bytes, hipStream_t s)
{
	scan_run<0>({ScanSrc::of_bytes(in0), out0, n0}, {ScanSrc::of_bytes(in1), out1, in1 ? n1 : 0}, tmp, tmp_bytes, s);
}
void scan_count_records_u8(const uint8_t *in0, uint4 *rec0, size_t n0, const uint8_t *in1, uint4 *rec1, size_t n1, void *tmp,
			   size_t tmp_bytes, hipStream_t s)
{
	scan_run<0, true>({ScanSrc::of_bytes(in0), reinterpret_cast<uint32_t *>(rec0), n0},
			  {ScanSrc::of_bytes(in1), reinterpret_cast<uint32_t *>(rec1), in1 ? n1 : 0}, tmp, tmp_bytes, s);
}
void scan_count_records_tiles(size_t *chunk_tile, size_t *lookback_tile)
{
	*chunk_tile = ScLane<true>::TILE;
	*lookback_tile = (size_t)ScLane<true>::TILE * LB_SUB;
}
void scan_exclusive_u32_pair(const uint32_t *in0, uint32_t *out0, size_t n0, const uint32_t *in1, uint32_t *out1, size_t n1,
			     void *tmp, size_t tmp_bytes, hipStream_t s)
{
	scan_run<0>({ScanSrc::words(in0), out0, n0}, {ScanSrc::words(in1), out1, n1}, tmp, tmp_bytes, s);
}
void scan_exclusive_u32_u8_pair(const uint32_t *in0, uint32_t *out0, size_t n0, const uint8_t *in1, uint32_t *out1, size_t n1,
				void *tmp, size_t tmp_bytes, hipStream_t s)
{
	scan_run<0>({ScanSrc::words(in0), out0, n0}, {ScanSrc::of_bytes(in1), out1, n1}, tmp, tmp_bytes, s);
}
void scan_exclusive_xor_u32_pair(const uint32_t *in0, uint32_t *out0, const uint32_t *in1, uint32_t *out1, size_t n, void *tmp,
				 size_t tmp_bytes, hipStream_t s)
{
	scan_run<2>({ScanSrc::words(in0), out0, n}, {ScanSrc::words(in1), out1, n}, tmp, tmp_bytes, s);
}

// ---- 64-bit totals of u32 counts: one array, or two of the same length side by side
__global__ void __launch_bounds__(SC_TPB) k_totals_u32(uint64_t n, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
						      unsigned long long *__restrict__ tot)
{
	__shared__ unsigned long long sa, sb;
	if (threadIdx.x == 0)
		sa = sb = 0;
	__syncthreads();
	unsigned long long x = 0, y = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * SC_TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SC_TPB) {
		x += a[i];
		if (b)
			y += b[i];
	}
	atomicAdd(&sa, x);
	if (b)
		atomicAdd(&sb, y);
	__syncthreads();
	if (threadIdx.x == 0) {
		atomicAdd(&tot[0], sa);
		if (b)
			atomicAdd(&tot[1], sb);
	}
}

void totals_u32(const uint32_t *a, const uint32_t *b, uint64_t n, unsigned long long *tot, uint64_t *h, hipStream_t s)
{
	const size_t bytes = b ? 16 : 8;
	HIP_CHECK(hipMemsetAsync(tot, 0, bytes, s));
	if (n)
		KLAUNCH(k_totals_u32, dim3((unsigned)std::min<uint64_t>((n + SC_TPB - 1) / SC_TPB, 1024)), dim3(SC_TPB), 0, s, n, a, b, tot);
	HIP_CHECK(copy_async(h, tot, bytes, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
}

// ---- exclusive u64 scan: per block of S64_N an LDS scan, the block sums scanned recursively, then added
static constexpr int S64_E = 4, S64_N = SC_TPB * S64_E; // elements per thread / per block
__global__ __launch_bounds__(SC_TPB) void k_u64_scan(const uint64_t *in, uint64_t *out, size_t n, uint64_t *__restrict__ sums)
{
	__shared__ uint64_t sh[SC_TPB];
	const size_t base = (size_t)blockIdx.x * S64_N + (size_t)threadIdx.x * S64_E;
	uint64_t v[S64_E], t = 0;
	for (int k = 0; k < S64_E; k++) {
		v[k] = base + k < n ? in[base + k] : 0;
		t += v[k];
	}
	sh[threadIdx.x] = t;
	__syncthreads();
	for (int d = 1; d < SC_TPB; d <<= 1) {
		const uint64_t x = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
		__syncthreads();
		sh[threadIdx.x] += x;
		__syncthreads();
	}
	uint64_t run = sh[threadIdx.x] - t;
	for (int k = 0; k < S64_E; k++) {
		if (base + k < n)
			out[base + k] = run;
		run += v[k];
	}
	if (threadIdx.x == SC_TPB - 1)
		sums[blockIdx.x] = sh[SC_TPB - 1];
}
__global__ __launch_bounds__(SC_TPB) void k_u64_add(uint64_t *out, size_t n, const uint64_t *__restrict__ offs)
{
	const size_t base = (size_t)blockIdx.x * S64_N;
	const uint64_t o = offs[blockIdx.x];
	for (size_t i = base + threadIdx.x; i < n && i < base + S64_N; i += SC_TPB)
		out[i] += o;
}
size_t scan_exclusive_u64_tmp(size_t n)
{
	size_t t = 2;
	while (n > 1) {
		n = (n + S64_N - 1) / S64_N;
		t += n + 1;
	}
	return t;
}
void scan_exclusive_u64(const uint64_t *in, uint64_t *out, size_t n, uint64_t *tmp, hipStream_t s)
{
	if (!n)
		return;
	const size_t nb = (n + S64_N - 1) / S64_N;
	KLAUNCH(k_u64_scan, dim3((unsigned)nb), dim3(SC_TPB), 0, s, in, out, n, tmp);
	if (nb > 1) {
		scan_exclusive_u64(tmp, tmp, nb, tmp + nb + 1, s);
		KLAUNCH(k_u64_add, dim3((unsigned)nb), dim3(SC_TPB), 0, s, out, n, tmp);
	}
}

// ---- exclusive running xor of 128-bit words (the bridge test's two hashes): same two-launch scheme, 2 words per lane
static constexpr int X128_ITEMS = 2, X128_TILE = SC_TPB * X128_ITEMS;
struct Xor128Job {
	const ulonglong2 *in;
	ulonglong2 *out;
	size_t n, chunk;
	uint32_t blocks;
	ulonglong2 *partial;
	const uint32_t *n_dev; // optional: only the first *n_dev + 1 words exist (n is then the most there can be)
};
__device__ __forceinline__ size_t x128_len(const Xor128Job &J)
{
	if (!J.n_dev)
		return J.n;
	const size_t m = (size_t)*J.n_dev + 1;
	return m < J.n ? m : J.n;
}
__global__ void __launch_bounds__(SC_TPB) k_xor128_partials(const Xor128Job J)
{
	__shared__ ulonglong2 sh[SC_WAVES];
	const Xor128 x128;
	const size_t n = x128_len(J);
	const size_t b0 = (size_t)blockIdx.x * J.chunk, b1 = b0 + J.chunk < n ? b0 + J.chunk : n;
	ulonglong2 acc = make_ulonglong2(0ull, 0ull);
	for (size_t i = b0 + threadIdx.x; i < b1; i += SC_TPB)
		acc = x128(acc, J.in[i]);
	acc = block_reduce<SC_WAVES>(acc, sh, x128);
	if (threadIdx.x == 0)
		J.partial[blockIdx.x] = acc;
}
__global__ void __launch_bounds__(SC_TPB) k_xor128_chunks(const Xor128Job J)
{
	__shared__ ulonglong2 sh[SC_WAVES], wave_tot[SC_WAVES];
	const Xor128 x128;
	ulonglong2 base = make_ulonglong2(0ull, 0ull);
	for (uint32_t k = threadIdx.x; k < blockIdx.x; k += SC_TPB)
		base = x128(base, J.partial[k]);
	ulonglong2 carry = block_reduce<SC_WAVES>(base, sh, x128);
	const size_t n = x128_len(J);
	const size_t b0 = (size_t)blockIdx.x * J.chunk, b1 = b0 + J.chunk < n ? b0 + J.chunk : n;
	for (size_t t0 = b0; t0 < b1; t0 += X128_TILE) {
		const size_t e0 = t0 + (size_t)threadIdx.x * X128_ITEMS;
		ulonglong2 v[X128_ITEMS];
		for (int k = 0; k < X128_ITEMS; k++)
			v[k] = e0 + k < b1 ? J.in[e0 + k] : make_ulonglong2(0ull, 0ull);
		ulonglong2 tot = make_ulonglong2(0ull, 0ull);
		for (int k = 0; k < X128_ITEMS; k++) {
			const ulonglong2 x = v[k];
			v[k] = tot;
			tot = x128(tot, x);
		}
		ulonglong2 tile_tot;
		const ulonglong2 pre = x128(carry, block_exclusive_scan<SC_WAVES>(tot, wave_tot, tile_tot, x128));
		for (int k = 0; k < X128_ITEMS; k++)
			if (e0 + k < b1)
				J.out[e0 + k] = x128(pre, v[k]);
		carry = x128(carry, tile_tot);
		__syncthreads();
	}
}
void scan_exclusive_xor_u128(const ulonglong2 *in, ulonglong2 *out, size_t n, void *tmp, size_t tmp_bytes, hipStream_t s,
			     const uint32_t *n_dev)
{
	if (n == 0)
		return;
	if (tmp_bytes < SC_MAX_BLOCKS * sizeof(ulonglong2))
		throw HipError("scan: temporary storage too small");
	size_t blocks = (n + X128_TILE - 1) / X128_TILE;
	if (blocks > SC_MAX_BLOCKS)
		blocks = SC_MAX_BLOCKS;
	size_t chunk = (n + blocks - 1) / blocks;
	chunk = (chunk + X128_TILE - 1) / X128_TILE * X128_TILE;
	blocks = (n + chunk - 1) / chunk;
	const Xor128Job J{in, out, n, chunk, (uint32_t)blocks, static_cast<ulonglong2 *>(tmp), n_dev};
	KLAUNCH(k_xor128_partials, dim3((unsigned)blocks), dim3(SC_TPB), 0, s, J);
	KLAUNCH(k_xor128_chunks, dim3((unsigned)blocks), dim3(SC_TPB), 0, s, J);
}

// ---- indices of the set bytes of a flag array, in order (stream compaction without a prefix array): per-tile counts,
// one workgroup scans the counts, the tiles then rank their own flags again and write the indices.  The flags are read
// twice (a byte each); the 4-byte prefix array a scan would hand to a separate compaction kernel is never written.
static constexpr int CP_TPB = 256, CP_ITEMS = 16, CP_TILE = CP_TPB * CP_ITEMS;
__device__ __forceinline__ uint32_t cp_load16(const uint8_t *__restrict__ flag, size_t e0, size_t n, uint32_t &bits)
{
	bits = 0;
	if (e0 + CP_ITEMS <= n) {
		const uint4 a = *reinterpret_cast<const uint4 *>(flag + e0);
		const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
		for (int k = 0; k < 4; k++)
#pragma unroll
			for (int b = 0; b < 4; b++)
				if ((w[k] >> (8 * b)) & 0xFFu)
					bits |= 1u << (4 * k + b);
	} else {
		for (int k = 0; k < CP_ITEMS; k++)
			if (e0 + k < n && flag[e0 + k])
				bits |= 1u << k;
	}
	return (uint32_t)__popc(bits);
}
__global__ void __launch_bounds__(CP_TPB) k_cp_count(const uint8_t *__restrict__ flag, size_t n, uint32_t *__restrict__ tile_cnt)
{
	__shared__ uint32_t sh[CP_TPB / 64];
	uint32_t bits, total;
	const uint32_t bx = BIDX;
	const uint32_t c = cp_load16(flag, (size_t)bx * CP_TILE + (size_t)threadIdx.x * CP_ITEMS, n, bits);
	(void)block_exclusive_scan<CP_TPB / 64>(c, sh, total, ScanOp<0>{});
	if (threadIdx.x == 0)
		tile_cnt[bx] = total;
}
// exclusive scan of the tile counts in place, one workgroup (a few ten thousand tiles); *count_out = the grand total
__global__ void __launch_bounds__(1024) k_cp_scan_tiles(uint32_t *tile_cnt, uint32_t ntiles, uint32_t *__restrict__ count_out)
{
	__shared__ uint32_t sh[16];
	const uint32_t per = (ntiles + 1023) / 1024, lo = min(ntiles, threadIdx.x * per), hi = min(ntiles, lo + per);
	uint32_t sum = 0;
	for (uint32_t k = lo; k < hi; k++)
		sum += tile_cnt[k];
	uint32_t total;
	uint32_t before = block_exclusive_scan<16>(sum, sh, total, ScanOp<0>{});
	for (uint32_t k = lo; k < hi; k++) {
		const uint32_t c = tile_cnt[k];
		tile_cnt[k] = before;
		before += c;
	}
	if (threadIdx.x == 0)
		*count_out = total;
}
__global__ void __launch_bounds__(CP_TPB) k_cp_write(const uint8_t *__restrict__ flag, size_t n, const uint32_t *__restrict__ tile_base,
						      uint32_t *__restrict__ out)
{
	__shared__ uint32_t sh[CP_TPB / 64];
	const uint32_t bx = BIDX;
	const size_t e0 = (size_t)bx * CP_TILE + (size_t)threadIdx.x * CP_ITEMS;
	uint32_t bits, total;
	const uint32_t c = cp_load16(flag, e0, n, bits);
	uint32_t at = tile_base[bx] + block_exclusive_scan<CP_TPB / 64>(c, sh, total, ScanOp<0>{});
	while (bits) {
		const int k = __ffs((int)bits) - 1;
		bits &= bits - 1;
		out[at++] = (uint32_t)(e0 + k);
	}
}
__global__ void k_bitrank_counts(uint32_t W, uint4 *__restrict__ rec, uint32_t *__restrict__ cnt)
{
	const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
	if (w > W)
		return;
	if (w == W) { // the closing record: rank(n) reads it
		rec[W] = make_uint4(0u, 0u, 0u, 0u);
		cnt[W] = 0;
		return;
	}
	const uint4 r = rec[w];
	cnt[w] = (uint32_t)(__popc(r.x) + __popc(r.y));
}
__global__ void k_bitrank_ranks(uint32_t W, const uint32_t *__restrict__ ps, uint4 *__restrict__ rec)
{
	const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
	if (w <= W)
		rec[w].z = ps[w];
}
void bitrank_build(uint4 *rec, size_t n_rec, uint32_t *tmp_counts, void *scan_tmp, size_t scan_tmp_bytes, hipStream_t s)
{
	const uint32_t W = (uint32_t)n_rec;
	const unsigned blocks = (unsigned)((n_rec + 1 + 255) / 256);
	KLAUNCH(k_bitrank_counts, dim3(blocks), dim3(256), 0, s, W, rec, tmp_counts);
	scan_exclusive_u32(tmp_counts, tmp_counts, n_rec + 1, scan_tmp, scan_tmp_bytes, s);
	KLAUNCH(k_bitrank_ranks, dim3(blocks), dim3(256), 0, s, W, tmp_counts, rec);
}
__global__ void k_publish_words(WordSrc src, int n, uint32_t *__restrict__ dst)
{
	if (threadIdx.x < (unsigned)n)
		dst[threadIdx.x] = *src.p[threadIdx.x];
}
void publish_words(uint32_t *host_dst, const WordSrc &src, int n, hipStream_t s)
{
	if (n <= 0 || n > 8)
		throw HipError("publish_words: 1..8 words");
	uint32_t *dev = nullptr;
	HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void **>(&dev), host_dst, 0));
	count_kernel_d2h((size_t)n * 4);
	KLAUNCH(k_publish_words, dim3(1), dim3(64), 0, s, src, n, dev);
}
size_t compact_tmp_bytes(size_t n) { return ((n + CP_TILE - 1) / CP_TILE + 1) * 4 + 256; }
void compact_flagged_u8(const uint8_t *flag, size_t n, uint32_t *out, uint32_t *count_dev, void *tmp, size_t tmp_bytes, hipStream_t s)
{
	if (n == 0) {
		HIP_CHECK(hipMemsetAsync(count_dev, 0, 4, s));
		return;
	}
	if (reinterpret_cast<uintptr_t>(flag) & 15)
		throw HipError("compaction: the flags must be 16-byte aligned");
	if (tmp_bytes < compact_tmp_bytes(n))
		throw HipError("compaction: temporary storage too small");
	const uint32_t ntiles = (uint32_t)((n + CP_TILE - 1) / CP_TILE);
	uint32_t *tile_cnt = static_cast<uint32_t *>(tmp);
	KLAUNCH(k_cp_count, dim3(ntiles), dim3(CP_TPB), 0, s, flag, n, tile_cnt);
	KLAUNCH(k_cp_scan_tiles, dim3(1), dim3(1024), 0, s, tile_cnt, ntiles, count_dev);
	KLAUNCH(k_cp_write, dim3(ntiles), dim3(CP_TPB), 0, s, flag, n, tile_cnt, out);
}

// ---- stable LSD radix sort of (key, value) pairs, hand-written.  Per place of RB bits: a histogram per tile of RS_TILE
// consecutive pairs, an exclusive scan over the [digit][tile] table (the scans above), and a scatter kernel in which
// every wave ranks its stretch of the tile with ballots (the lanes that hold the same digit find each other by RB
// ballots: no atomics, the order of equal keys is the order of the input), the tile is sorted into LDS, and consecutive
// lanes then write consecutive pairs of one digit to consecutive addresses.  Pangenome keys cluster (brackets of one
// bubble, slots of one side): runs of one digit inside a tile are long, and the table says where each run goes.
static constexpr int RS_TPB = 256, RS_WAVES = RS_TPB / 64, RS_ITEMS = 16, RS_TILE = RS_TPB * RS_ITEMS, RS_MAX_BINS = 1024;

__global__ void __launch_bounds__(RS_TPB) k_rs_hist(const uint32_t *__restrict__ keys, uint32_t n, unsigned shift, unsigned rb,
						     uint32_t *__restrict__ hist, uint32_t ntiles)
{
	__shared__ uint32_t h[RS_MAX_BINS];
	const uint32_t bins = 1u << rb, mask = bins - 1u;
	for (uint32_t d = threadIdx.x; d < bins; d += RS_TPB)
		h[d] = 0;
	__syncthreads();
	const uint32_t bx = BIDX, base = bx * RS_TILE;
	// four consecutive keys a lane and load (a histogram does not care which lane counts which key): a quarter of the
	// memory instructions
#pragma unroll
	for (int r = 0; r < RS_ITEMS / 4; r++) {
		const uint32_t i0 = base + (r * RS_TPB + threadIdx.x) * 4u;
		if (__all(i0 + 4 <= n)) {
			const uint4 k = *reinterpret_cast<const uint4 *>(keys + i0);
			const uint32_t d[4] = {(k.x >> shift) & mask, (k.y >> shift) & mask, (k.z >> shift) & mask, (k.w >> shift) & mask};
			// a whole wave on one digit (clustered keys) adds once
			const uint32_t d0 = __builtin_amdgcn_readfirstlane(d[0]);
			if (__all(d[0] == d0 && d[1] == d0 && d[2] == d0 && d[3] == d0)) {
				if ((threadIdx.x & 63) == 0)
					atomicAdd(&h[d0], 256u);
			} else {
#pragma unroll
				for (int q = 0; q < 4; q++)
					atomicAdd(&h[d[q]], 1u);
			}
		} else {
			for (uint32_t i = i0; i < i0 + 4 && i < n; i++)
				atomicAdd(&h[(keys[i] >> shift) & mask], 1u);
		}
	}
	__syncthreads();
	for (uint32_t d = threadIdx.x; d < bins; d += RS_TPB)
		hist[(size_t)d * ntiles + bx] = h[d];
}

__global__ void __launch_bounds__(RS_TPB) k_rs_scatter(const uint32_t *__restrict__ kin, const uint32_t *__restrict__ vin,
							uint32_t *__restrict__ kout, uint32_t *__restrict__ vout, uint32_t n, unsigned shift,
							unsigned rb, const uint32_t *__restrict__ gofs, uint32_t ntiles)
{
	// the counters are dead once every pair knows its tile-local position: the staging area lies over them (36 KB of
	// LDS in all, four workgroups per CU)
	struct Counters {
		uint32_t wcnt[RS_WAVES][RS_MAX_BINS]; // per wave: pairs of a digit seen so far; later: pairs in the waves before
		uint32_t bbase[RS_MAX_BINS];	      // first tile-local position of a digit
	};
	union Overlay {
		Counters c;
		uint2 stage[RS_TILE];
	};
	__shared__ Overlay sh;
	__shared__ uint32_t gof[RS_MAX_BINS]; // where the digit's run of this tile starts in the output, less bbase
	__shared__ uint32_t wsum[RS_WAVES];
	const uint32_t bins = 1u << rb, mask = bins - 1u;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const unsigned long long lt = (1ull << lane) - 1ull;
	for (uint32_t k = 0; k < RS_WAVES; k++)
		for (uint32_t d = threadIdx.x; d < bins; d += RS_TPB)
			sh.c.wcnt[k][d] = 0;
	const uint32_t bx = BIDX, base = bx * RS_TILE, wbase = base + wave * (RS_ITEMS * 64);
	uint32_t key[RS_ITEMS], val[RS_ITEMS], pos[RS_ITEMS];
#pragma unroll
	for (int r = 0; r < RS_ITEMS; r++) {
		const uint32_t i = wbase + r * 64 + lane;
		key[r] = i < n ? kin[i] : 0xFFFFFFFFu;
		val[r] = i < n ? vin[i] : 0u;
	}
	__syncthreads();
	// ---- rank inside the wave's stretch
#pragma unroll
	for (int r = 0; r < RS_ITEMS; r++) {
		const bool live = wbase + r * 64 + lane < n;
		const uint32_t d = (key[r] >> shift) & mask;
		unsigned long long peers = __ballot(live);
		for (unsigned b = 0; b < rb; b++) {
			const unsigned long long m = __ballot((d >> b) & 1u);
			peers &= ((d >> b) & 1u) ? m : ~m;
		}
		uint32_t old = 0;
		if (live) {
			const int leader = __ffsll((long long)peers) - 1;
			if ((int)lane == leader) {
				old = sh.c.wcnt[wave][d];
				sh.c.wcnt[wave][d] = old + (uint32_t)__popcll(peers);
			}
			old = __shfl(old, leader);
		}
		pos[r] = old + (uint32_t)__popcll(peers & lt);
	}
	__syncthreads();
	// ---- per digit: the pairs of the waves before (exclusive over waves), the tile's count; then the tile-local bases
	uint32_t mine = 0; // pairs of the digits this thread owns: digits [t * per, (t + 1) * per)
	const uint32_t per = (bins + RS_TPB - 1) / RS_TPB;
	for (uint32_t k = 0; k < per; k++) {
		const uint32_t d = threadIdx.x * per + k;
		if (d < bins) {
			uint32_t run = 0;
			for (int w = 0; w < RS_WAVES; w++) {
				const uint32_t c = sh.c.wcnt[w][d];
				sh.c.wcnt[w][d] = run;
				run += c;
			}
			sh.c.bbase[d] = run; // (count for now)
			mine += run;
		}
	}
	uint32_t tile_pairs; // (= the tile's live pairs; not needed)
	uint32_t before = block_exclusive_scan<RS_WAVES>(mine, wsum, tile_pairs, ScanOp<0>{});
	for (uint32_t k = 0; k < per; k++) {
		const uint32_t d = threadIdx.x * per + k;
		if (d < bins) {
			const uint32_t c = sh.c.bbase[d];
			sh.c.bbase[d] = before;
			gof[d] = gofs[(size_t)d * ntiles + bx] - before;
			before += c;
		}
	}
	__syncthreads();
#pragma unroll
	for (int r = 0; r < RS_ITEMS; r++) {
		const uint32_t d = (key[r] >> shift) & mask;
		pos[r] += sh.c.bbase[d] + sh.c.wcnt[wave][d];
	}
	__syncthreads(); // the counters are dead: the tile, sorted by digit, goes over them
#pragma unroll
	for (int r = 0; r < RS_ITEMS; r++)
		if (wbase + r * 64 + lane < n)
			sh.stage[pos[r]] = make_uint2(key[r], val[r]);
	__syncthreads();
	const uint32_t cnt = min((uint32_t)RS_TILE, n - base);
	for (uint32_t j = threadIdx.x; j < cnt; j += RS_TPB) {
		const uint2 e = sh.stage[j];
		const uint32_t gp = gof[(e.x >> shift) & mask] + j;
		kout[gp] = e.x;
		vout[gp] = e.y;
	}
}

static unsigned rs_places(size_t n, unsigned bits, unsigned &rb)
{
	// 9-bit digits (three places for the 25..27 key bits of a whole-genome graph); small inputs, whose table stays small,
	// take 10 and save a place where that helps
	const unsigned widest = n <= (size_t(1) << 24) ? 10u : 9u;
	const unsigned places = (bits + widest - 1) / widest;
	rb = (bits + places - 1) / places;
	return places;
}
static size_t rs_table_words(size_t n) { return (size_t)RS_MAX_BINS / (n <= (size_t(1) << 24) ? 1 : 2) * ((n + RS_TILE - 1) / RS_TILE) + 64; }

size_t sort_tmp_bytes(size_t n)
{
	// ping-pong buffer for keys and values + the [digit][tile] table (scanned in place) + the scan's own scratch
	return 2 * ((n * 4 + 255) & ~size_t(255)) + ((rs_table_words(n) * 4 + 255) & ~size_t(255)) + scan_tmp_bytes(rs_table_words(n)) + 1024;
}

size_t prim_tmp_bytes(size_t n, bool with_sort)
{
	return std::max({scan_tmp_bytes(n), compact_tmp_bytes(n), with_sort ? sort_tmp_bytes(n) : size_t(0)});
}

void sort_pairs_u32(const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout, size_t n, unsigned bits,
		    void *tmp, size_t tmp_bytes, hipStream_t s)
{
	if (n == 0)
		return;
	if (n >= (size_t(1) << 32) - RS_TILE)
		throw HipError("sort: too many pairs");
	if (tmp_bytes < sort_tmp_bytes(n))
		throw HipError("sort: temporary storage too small");
	if (bits == 0)
		bits = 1;
	char *q = static_cast<char *>(tmp);
	uint32_t *kt = reinterpret_cast<uint32_t *>(q);
	q += (n * 4 + 255) & ~size_t(255);
	uint32_t *vt = reinterpret_cast<uint32_t *>(q);
	q += (n * 4 + 255) & ~size_t(255);
	uint32_t *table = reinterpret_cast<uint32_t *>(q);
	q += (rs_table_words(n) * 4 + 255) & ~size_t(255);
	void *stmp = q;
	const size_t stmp_bytes = scan_tmp_bytes(rs_table_words(n));
	unsigned rb = 0;
	const unsigned places = rs_places(n, bits, rb);
	const uint32_t ntiles = (uint32_t)((n + RS_TILE - 1) / RS_TILE);
	// the last place writes kout / vout: in -> [tmp ->] out for an even / odd number of places
	const uint32_t *ki = kin, *vi = vin;
	for (unsigned p = 0; p < places; p++) {
		const bool to_out = ((places - 1 - p) & 1u) == 0;
		uint32_t *ko = to_out ? kout : kt, *vo = to_out ? vout : vt;
		const unsigned shift = p * rb, w = std::min(rb, bits - std::min(bits, shift));
		const unsigned prb = w ? w : 1u;
		const size_t words = ((size_t)1 << prb) * ntiles;
		KLAUNCH(k_rs_hist, dim3(ntiles), dim3(RS_TPB), 0, s, ki, (uint32_t)n, shift, prb, table, ntiles);
		scan_exclusive_u32(table, table, words, stmp, stmp_bytes, s);
		KLAUNCH(k_rs_scatter, dim3(ntiles), dim3(RS_TPB), 0, s, ki, vi, ko, vo, (uint32_t)n, shift, prb, table, ntiles);
		ki = ko, vi = vo;
	}
}

} // namespace povu_hip
