// debug_hooks.hip -- the C ABI's unit-test and parity hooks (include/povu_hip.h, povu_hip_debug_*): the device-wide
// primitives and look-up structures called directly, and the state of the last pass stage by stage.  Not the library.
#include "context.hpp"
#include "list_rank.hpp"
#include "segtree.hpp"

#include <algorithm>
#include <numeric>

using namespace povu_hip;

// ---- unit-test hooks for the device-wide primitives (primitives.hip).  Each call carves an arena of its own and touches
// nothing of the context but its stream.  Two things hold for all of them: the primitive's scratch is filled with a
// non-zero byte before the call (nothing may rely on scratch that happens to be zero: the look-back's status words and
// ticket, the compaction's tile counts, the sort's table), and every device output lies between two guard bands of a
// fixed byte, at least 64 words each, which are read back afterwards -- a changed guard byte is return code 5.
// A hook declares its buffers once, each with its size, and dbg_carve lays them out in an arena of the hook's own: as
// a list for carve (common.hpp), in which every buffer names its span and, in the run that hands out the pointers, fills it.
namespace
{
constexpr size_t DBG_GUARD = 256; // bytes in front of an output; behind it: as many, plus the padding of its span
constexpr int DBG_GUARD_BYTE = 0xC5, DBG_POISON_BYTE = 0xA7;
constexpr int DBG_RC_GUARD = 5;
// a guarded output of `bytes`, 256-byte aligned; the guards hold the guard byte and the payload holds `fill` until the
// primitive writes.  !on: the call has no such output, nothing is taken
struct DbgOut {
	size_t bytes = 0;
	int fill = DBG_GUARD_BYTE;
	bool on = true;
	char *base = nullptr;
	size_t span = 0; // the whole stretch with both guards
	template <class T>
	T *data() const { return reinterpret_cast<T *>(base + DBG_GUARD); }
	void declare(Spans &take, hipStream_t s)
	{
		if (!on)
			return;
		span = DBG_GUARD + Arena::padded(bytes, 1) + DBG_GUARD;
		take(span, base);
		if (take.ar)
			HIP_CHECK(hipMemsetAsync(base, DBG_GUARD_BYTE, span, s));
		if (take.ar && bytes && fill != DBG_GUARD_BYTE)
			HIP_CHECK(hipMemsetAsync(base + DBG_GUARD, fill, bytes, s));
	}
};
// scratch of exactly `bytes`, filled with the poison byte
struct DbgScratch {
	size_t bytes = 0;
	void *p = nullptr;
	void declare(Spans &take, hipStream_t s)
	{
		take(bytes, p);
		if (take.ar && bytes)
			HIP_CHECK(hipMemsetAsync(p, DBG_POISON_BYTE, bytes, s));
	}
};
// device copy of a host input, 256-byte aligned, with a little slack behind it.  !on: nothing is taken
template <class T>
struct DbgIn {
	const T *host = nullptr;
	size_t n = 0;
	bool on = true;
	const T *dev = nullptr;
	void declare(Spans &take, hipStream_t s)
	{
		T *d = nullptr;
		if (on)
			take(n + 16, d);
		if (take.ar && on && n)
			HIP_CHECK(copy_async(d, host, n * sizeof(T), hipMemcpyHostToDevice, s));
		dev = d;
	}
};
template <class... B>
void dbg_carve(Arena &ar, hipStream_t s, B &...buf)
{
	carve(ar, [&](Spans &take) { (buf.declare(take, s), ...); });
}
bool dbg_all_guard(const void *host, size_t from, size_t to)
{
	const unsigned char *p = static_cast<const unsigned char *>(host);
	for (size_t i = from; i < to; i++)
		if (p[i] != (unsigned char)DBG_GUARD_BYTE)
			return false;
	return true;
}
// both guard bands still hold the pattern (waits for the stream)
bool dbg_guards_intact(const DbgOut &o, hipStream_t s)
{
	if (!o.base)
		return true;
	const size_t back = o.span - DBG_GUARD - o.bytes;
	std::vector<unsigned char> h(DBG_GUARD + back);
	HIP_CHECK(copy_async(h.data(), o.base, DBG_GUARD, hipMemcpyDeviceToHost, s));
	HIP_CHECK(copy_async(h.data() + DBG_GUARD, o.base + DBG_GUARD + o.bytes, back, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	return dbg_all_guard(h.data(), 0, h.size());
}
// what povu_hip_debug_scan's arguments mean for each POVU_HIP_SCAN_* op (the row's index)
enum DbgSecond { DBG_NONE, DBG_PAIR, DBG_SUB }; // in2 is: unused / a job of its own, with out2 / what is subtracted from `in`
struct DbgScanOp {
	size_t e_in, e_in2, e_out; // bytes per element of in, in2 and the outputs
	DbgSecond second;
	bool need2;	// in2 must be there
	bool len_n2;	// in2 has n2 elements (else n)
	bool in_place;	// POVU_HIP_SCAN_IN_PLACE allowed
	bool n_dev;	// POVU_HIP_SCAN_N_DEV allowed
	bool nullable;	// an empty array may be a null pointer
};
const DbgScanOp DBG_SCAN_OPS[] = {
	{4, 4, 4, DBG_PAIR, false, true, true, false, false},	  // POVU_HIP_SCAN_SUM
	{4, 4, 4, DBG_NONE, false, false, true, false, false},	  // POVU_HIP_SCAN_MAX
	{8, 8, 8, DBG_NONE, false, false, true, false, false},	  // POVU_HIP_SCAN_U64
	{1, 1, 4, DBG_PAIR, false, true, false, false, true},	  // POVU_HIP_SCAN_U8
	{4, 4, 4, DBG_SUB, true, false, false, false, false},	  // POVU_HIP_SCAN_DIFF
	{4, 4, 4, DBG_PAIR, true, false, false, false, false},	  // POVU_HIP_SCAN_XOR_PAIR
	{16, 16, 16, DBG_NONE, false, false, false, true, false}, // POVU_HIP_SCAN_XOR_U128
	{1, 4, 4, DBG_SUB, true, false, false, false, false},	  // POVU_HIP_SCAN_DIFF_U8
	{4, 1, 4, DBG_PAIR, true, true, false, false, false},	  // POVU_HIP_SCAN_MIXED_PAIR
	{1, 1, 4, DBG_SUB, true, false, false, false, false},	  // POVU_HIP_SCAN_DIFF_U8_U8
	{4, 4, 4, DBG_NONE, false, false, true, false, false},	  // POVU_HIP_SCAN_INCLUSIVE
};
static_assert(sizeof(DBG_SCAN_OPS) / sizeof(DBG_SCAN_OPS[0]) == POVU_HIP_SCAN_INCLUSIVE + 1, "one row per op");
} // namespace

extern "C" int povu_hip_debug_scan(povu_hip_ctx *ctx, int op, const uint32_t *in, uint32_t *out, size_t n, const uint32_t *in2,
				   uint32_t *out2, size_t n2)
{
	const int kind = op & 0xFF;
	const bool in_place = (op & POVU_HIP_SCAN_IN_PLACE) != 0, with_len = (op & POVU_HIP_SCAN_N_DEV) != 0;
	if (!ctx || kind > POVU_HIP_SCAN_INCLUSIVE || (op & ~(0xFF | POVU_HIP_SCAN_IN_PLACE | POVU_HIP_SCAN_N_DEV)))
		return 1;
	const DbgScanOp &T = DBG_SCAN_OPS[kind];
	if (T.nullable ? ((n && (!in || !out)) || (in2 && n2 && !out2)) : (!in || !out || (in2 && !out2 && T.second != DBG_SUB)))
		return 1;
	if ((in_place && (!T.in_place || in2)) || (with_len && !T.n_dev) || (T.need2 && !in2))
		return 1;
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		hipStream_t s = ctx->stream;
		// element sizes, the length of the second input and whether it has an output of its own
		const size_t e_in = T.e_in, e_in2 = T.e_in2, e_out = T.e_out;
		const bool pair = in2 && T.second == DBG_PAIR, second_in = in2 && T.second != DBG_NONE;
		const size_t m = !second_in ? 0 : T.len_n2 ? n2 : n;
		const size_t tb = kind == POVU_HIP_SCAN_U64 ? scan_exclusive_u64_tmp(n) * 8 : scan_tmp_bytes(std::max(n, m));
		const uint32_t len = (uint32_t)n2;
		Arena ar;
		DbgOut o1{n * e_out}, o2{m * e_out, DBG_GUARD_BYTE, pair};
		DbgScratch scr{tb};
		DbgIn<char> i1{reinterpret_cast<const char *>(in), n * e_in, !in_place}, i2{reinterpret_cast<const char *>(in2), m * e_in2, second_in};
		DbgIn<uint32_t> ilen{&len, 1, with_len};
		dbg_carve(ar, s, o1, o2, scr, i1, i2, ilen);
		if (in_place)
			HIP_CHECK(copy_async(o1.data<char>(), in, n * e_in, hipMemcpyHostToDevice, s));
		if (with_len)
			HIP_CHECK(hipStreamSynchronize(s)); // (`len` has been read whatever happens below)
		const char *di = in_place ? o1.data<char>() : i1.dev, *di2 = i2.dev;
		const uint32_t *w1 = reinterpret_cast<const uint32_t *>(di), *w2 = reinterpret_cast<const uint32_t *>(di2);
		void *tmp = scr.p;
		switch (kind) {
		case POVU_HIP_SCAN_SUM:
			if (pair)
				scan_exclusive_u32_pair(w1, o1.data<uint32_t>(), n, w2, o2.data<uint32_t>(), m, tmp, tb, s);
			else
				scan_exclusive_u32(w1, o1.data<uint32_t>(), n, tmp, tb, s);
			break;
		case POVU_HIP_SCAN_MAX: scan_exclusive_max_u32(w1, o1.data<uint32_t>(), n, tmp, tb, s); break;
		case POVU_HIP_SCAN_INCLUSIVE: scan_inclusive_u32(w1, o1.data<uint32_t>(), n, tmp, tb, s); break;
		case POVU_HIP_SCAN_U64: // n u64 values, each a pair of words
			scan_exclusive_u64(reinterpret_cast<const uint64_t *>(di), o1.data<uint64_t>(), n, static_cast<uint64_t *>(tmp), s);
			break;
		case POVU_HIP_SCAN_U8:
			scan_exclusive_u8(reinterpret_cast<const uint8_t *>(di), o1.data<uint32_t>(), n,
					  pair ? reinterpret_cast<const uint8_t *>(di2) : nullptr, pair ? o2.data<uint32_t>() : nullptr, m, tmp, tb, s);
			break;
		case POVU_HIP_SCAN_DIFF: scan_exclusive_diff_u32(w1, w2, o1.data<uint32_t>(), n, tmp, tb, s); break;
		case POVU_HIP_SCAN_DIFF_U8:
			scan_exclusive_diff_u8_u32(reinterpret_cast<const uint8_t *>(di), w2, o1.data<uint32_t>(), n, tmp, tb, s);
			break;
		case POVU_HIP_SCAN_DIFF_U8_U8:
			scan_exclusive_diff_u8_u8(reinterpret_cast<const uint8_t *>(di), reinterpret_cast<const uint8_t *>(di2), o1.data<uint32_t>(), n, tmp, tb, s);
			break;
		case POVU_HIP_SCAN_MIXED_PAIR:
			scan_exclusive_u32_u8_pair(w1, o1.data<uint32_t>(), n, reinterpret_cast<const uint8_t *>(di2), o2.data<uint32_t>(), m, tmp, tb, s);
			break;
		case POVU_HIP_SCAN_XOR_PAIR: scan_exclusive_xor_u32_pair(w1, o1.data<uint32_t>(), w2, o2.data<uint32_t>(), n, tmp, tb, s); break;
		default:
			scan_exclusive_xor_u128(reinterpret_cast<const ulonglong2 *>(di), o1.data<ulonglong2>(), n, tmp, tb, s, ilen.dev);
			break;
		}
		if (n)
			HIP_CHECK(copy_async(out, o1.data<char>(), n * e_out, hipMemcpyDeviceToHost, s));
		if (pair && m)
			HIP_CHECK(copy_async(out2, o2.data<char>(), m * e_out, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		if (!dbg_guards_intact(o1, s) || !dbg_guards_intact(o2, s))
			return DBG_RC_GUARD;
		// (only the first n2 + 1 words exist: what lies behind them is a guard as well)
		if (with_len && !dbg_all_guard(out, std::min<size_t>(n2 + 1, n) * 16, n * 16))
			return DBG_RC_GUARD;
		return 0;
	} catch (const std::exception &) {
		return 2;
	}
}

extern "C" int povu_hip_debug_sort(povu_hip_ctx *ctx, const uint32_t *keys, const uint32_t *vals, size_t n, unsigned bits,
				   uint32_t *keys_out, uint32_t *vals_out)
{
	if (!ctx || bits > 32 || (n && (!keys || !vals || !keys_out || !vals_out)))
		return 1;
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		hipStream_t s = ctx->stream;
		const size_t tb = sort_tmp_bytes(n);
		Arena ar;
		DbgOut ko{n * 4}, vo{n * 4};
		DbgScratch tmp{tb};
		DbgIn<uint32_t> dk{keys, n}, dv{vals, n};
		dbg_carve(ar, s, ko, vo, tmp, dk, dv);
		sort_pairs_u32(dk.dev, ko.data<uint32_t>(), dv.dev, vo.data<uint32_t>(), n, bits, tmp.p, tb, s);
		if (n) {
			HIP_CHECK(copy_async(keys_out, ko.data<char>(), n * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(copy_async(vals_out, vo.data<char>(), n * 4, hipMemcpyDeviceToHost, s));
		}
		HIP_CHECK(hipStreamSynchronize(s));
		return dbg_guards_intact(ko, s) && dbg_guards_intact(vo, s) ? 0 : DBG_RC_GUARD;
	} catch (const std::exception &) {
		return 2;
	}
}

extern "C" int povu_hip_debug_compact(povu_hip_ctx *ctx, const uint8_t *flags, size_t n, uint32_t *out, uint32_t *count)
{
	if (!ctx || !count || n >= (size_t(1) << 32) || (n && (!flags || !out)))
		return 1;
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		hipStream_t s = ctx->stream;
		const size_t tb = compact_tmp_bytes(n);
		Arena ar;
		DbgOut oo{n * 4}, oc{4};
		DbgScratch tmp{tb};
		DbgIn<uint8_t> df{flags, n};
		dbg_carve(ar, s, oo, oc, tmp, df);
		compact_flagged_u8(df.dev, n, oo.data<uint32_t>(), oc.data<uint32_t>(), tmp.p, tb, s);
		if (n)
			HIP_CHECK(copy_async(out, oo.data<char>(), n * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(count, oc.data<char>(), 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		if (!dbg_guards_intact(oo, s) || !dbg_guards_intact(oc, s))
			return DBG_RC_GUARD;
		// (`count` indices were due: what lies behind them is a guard as well)
		return dbg_all_guard(out, std::min<size_t>(*count, n) * 4, n * 4) ? 0 : DBG_RC_GUARD;
	} catch (const std::exception &) {
		return 2;
	}
}

extern "C" int povu_hip_debug_totals(povu_hip_ctx *ctx, const uint32_t *a, const uint32_t *b, size_t n, uint64_t tot[2])
{
	if (!ctx || !tot || (n && !a))
		return 1;
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		hipStream_t s = ctx->stream;
		Arena ar;
		DbgOut ot{b ? size_t(16) : size_t(8)}; // (one array: the second total's word is a guard)
		DbgIn<uint32_t> da{a, n}, db{b, n, b != nullptr};
		dbg_carve(ar, s, ot, da, db);
		tot[0] = tot[1] = 0;
		totals_u32(da.dev, db.dev, n, ot.data<unsigned long long>(), tot, s);
		return dbg_guards_intact(ot, s) ? 0 : DBG_RC_GUARD;
	} catch (const std::exception &) {
		return 2;
	}
}

// ---- unit-test hooks for the look-up structures one layer above the primitives: the coarse min segment tree (segtree.hpp),
// the bit-rank directory and append_in_order (common.hpp).  Same conventions as above.  The kernels here only bring the
// inputs into the shape the real producers and consumers have; the structures themselves are the real functions.
namespace
{
constexpr uint32_t DBG_SEG_MIN = POVU_HIP_SEG_MIN, DBG_SEG_FIRST = POVU_HIP_SEG_FIRST_LESS, DBG_SEG_LAST = POVU_HIP_SEG_LAST_LESS;
// one query (kind, l, r, x) a lane, grid-stride: neighbouring lanes hold different queries, as in the real consumers
__global__ void __launch_bounds__(256) k_dbg_seg_query(SegTree st, uint32_t nq, const uint4 *__restrict__ q, uint32_t *__restrict__ out)
{
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += gridDim.x * blockDim.x) {
		const uint4 a = q[i];
		out[i] = a.x == DBG_SEG_MIN ? seg_min(st, a.y, a.z) : a.x == DBG_SEG_FIRST ? seg_first_less(st, a.y, a.z, a.w) : seg_last_less(st, a.y, a.z, a.w);
	}
}
// the shape of k_bridge_flags (par_kernels.hip): 256 lanes, four consecutive flags a lane, whole waves over [0, n]
__global__ void __launch_bounds__(256) k_dbg_bitrank_flags(uint32_t n, const uint8_t *__restrict__ flags, uint4 *__restrict__ rec)
{
	const uint32_t t0 = (BIDX * blockDim.x + threadIdx.x) * 4u;
	uint32_t f = 0;
	for (uint32_t j = 0; j < 4 && t0 + j < n; j++)
		f |= (flags[t0 + j] ? 1u : 0u) << j;
	const uint32_t w0 = (BIDX * blockDim.x + (threadIdx.x & ~63u)) / 16u; // first record of this wave's 256 positions
	bitrank_store_wave(rec + w0, f, w0 + (threadIdx.x & 63u) <= n / 64u);
}
// rank[i] = bitrank(x[i]) (x[i] <= n), test[i] = bitrank_test(x[i]) where x[i] < n (left alone elsewhere)
__global__ void __launch_bounds__(256) k_dbg_bitrank_query(uint32_t n, const uint4 *__restrict__ rec, uint32_t nq, const uint32_t *__restrict__ x,
							   uint32_t *__restrict__ rank, uint32_t *__restrict__ test)
{
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += gridDim.x * blockDim.x) {
		const uint32_t p = x[i];
		rank[i] = bitrank(rec, p);
		if (p < n)
			test[i] = bitrank_test(rec, p) ? 1u : 0u;
	}
}
__global__ void __launch_bounds__(256) k_dbg_cntrec_query(const uint4 *__restrict__ rec, uint32_t nq, const uint32_t *__restrict__ x,
							  uint32_t *__restrict__ prefix, uint32_t *__restrict__ count)
{
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += gridDim.x * blockDim.x) {
		prefix[i] = cntrec_prefix(rec, x[i]);
		count[i] = cntrec_count(rec, x[i]);
	}
}
// the shape of k_entry_list (tree_kernels.hip): a workgroup of LIST_TPB lanes over LIST_SPAN positions, bit 4 it + j of fw =
// position B0 + 1024 it + 4 tid + j
__global__ void __launch_bounds__(LIST_TPB) k_dbg_append(uint32_t n, const uint8_t *__restrict__ flags, uint32_t *__restrict__ list,
							  uint32_t *__restrict__ n_list)
{
	const uint32_t B0 = BIDX * LIST_SPAN;
	unsigned long long fw = 0;
#pragma unroll
	for (uint32_t it = 0; it < LIST_ITER; it++) {
		const uint32_t p0 = B0 + it * (LIST_TPB * 4u) + threadIdx.x * 4u;
		uint32_t f = 0;
		for (uint32_t j = 0; j < 4 && p0 + j < n; j++)
			f |= (flags[p0 + j] ? 1u : 0u) << j;
		fw |= (unsigned long long)f << (4 * it);
	}
	append_in_order(fw, B0, list, n_list);
}
constexpr size_t DBG_LOOKUP_MAX_N = (size_t(1) << 32) - (size_t(1) << 16); // (positions and their block / span arithmetic stay in 32 bits)
unsigned dbg_query_blocks(size_t nq) { return (unsigned)std::min<size_t>(std::max<size_t>((nq + 255) / 256, 1), 4096); }
} // namespace

extern "C" int povu_hip_debug_segtree(povu_hip_ctx *ctx, const uint32_t *val, size_t n, const uint32_t *queries, size_t nq, uint32_t *out,
				      uint32_t *tree, uint32_t *P)
{
	if (!ctx || n > DBG_LOOKUP_MAX_N || nq >= (size_t(1) << 32) || (n && !val) || (nq && (!queries || !out)))
		return 1;
	for (size_t i = 0; i < nq; i++) // (kind, l, r, x): no call site asks beyond the values; l > r is an empty range
		if (queries[4 * i] > DBG_SEG_LAST || queries[4 * i + 2] > n)
			return 1;
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		hipStream_t s = ctx->stream;
		const size_t padded = (n + SEG_BLK - 1) / SEG_BLK * SEG_BLK, tw = SegTree::tree_words(n);
		Arena ar;
		DbgOut ot{tw * 4, DBG_POISON_BYTE}, oq{nq * 4};
		DbgScratch vals{(padded + SEG_BLK) * 4};
		DbgIn<uint32_t> dq{queries, 4 * nq};
		dbg_carve(ar, s, ot, oq, vals, dq);
		// the values, 16-byte aligned; the tail of the last block holds ZEROS (below every useful threshold and every
		// minimum: a build or a query that lets a tail value through gives a wrong answer), the block behind it poison
		uint32_t *dv = static_cast<uint32_t *>(vals.p);
		if (n)
			HIP_CHECK(copy_async(dv, val, n * 4, hipMemcpyHostToDevice, s));
		if (padded > n)
			HIP_CHECK(hipMemsetAsync(dv + n, 0, (padded - n) * 4, s));
		SegTree st;
		st.tree = ot.data<uint32_t>();
		seg_build(st, dv, n, s); // (2 P <= tree_words(n): pow2 is monotone)
		if (nq)
			KLAUNCH(k_dbg_seg_query, dim3(dbg_query_blocks(nq)), dim3(256), 0, s, st, (uint32_t)nq, reinterpret_cast<const uint4 *>(dq.dev), oq.data<uint32_t>());
		std::vector<uint32_t> ht(tw);
		HIP_CHECK(copy_async(ht.data(), ot.data<char>(), tw * 4, hipMemcpyDeviceToHost, s));
		if (nq)
			HIP_CHECK(copy_async(out, oq.data<char>(), nq * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		if (P)
			*P = st.P;
		if (tree)
			std::copy(ht.begin(), ht.begin() + 2 * (size_t)st.P, tree);
		if (!dbg_guards_intact(ot, s) || !dbg_guards_intact(oq, s))
			return DBG_RC_GUARD;
		// (the tree has 2 P nodes: the words of the buffer behind them belong to nobody)
		const unsigned char *hb = reinterpret_cast<const unsigned char *>(ht.data());
		for (size_t i = 2 * (size_t)st.P * 4; i < tw * 4; i++)
			if (hb[i] != (unsigned char)DBG_POISON_BYTE)
				return DBG_RC_GUARD;
		return 0;
	} catch (const std::exception &) {
		return 2;
	}
}

extern "C" int povu_hip_debug_bitrank(povu_hip_ctx *ctx, const uint8_t *flags, size_t n, const uint32_t *pos, size_t nq, uint32_t *rank,
				      uint32_t *test, uint32_t *records)
{
	if (!ctx || n > DBG_LOOKUP_MAX_N || nq >= (size_t(1) << 32) || (n && !flags) || (nq && (!pos || !rank || !test)))
		return 1;
	for (size_t i = 0; i < nq; i++)
		if (pos[i] > n)
			return 1;
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		hipStream_t s = ctx->stream;
		const size_t n_rec = n / 64 + 1, tb = scan_tmp_bytes(n_rec + 1); // records of [0, n]; one more closes the array
		Arena ar;
		DbgOut orec{(n_rec + 1) * 16, DBG_POISON_BYTE}, ocnt{(n_rec + 1) * 4, DBG_POISON_BYTE}, ork{nq * 4}, ots{nq * 4};
		DbgScratch tmp{tb};
		DbgIn<uint8_t> df{flags, n};
		DbgIn<uint32_t> dp{pos, nq};
		dbg_carve(ar, s, orec, ocnt, ork, ots, tmp, df, dp);
		uint4 *rec = orec.data<uint4>();
		const size_t waves = n / 256 + 1; // whole waves: every record of [0, n] is written
		KLAUNCH(k_dbg_bitrank_flags, dim3((unsigned)((waves * 64 + 255) / 256)), dim3(256), 0, s, (uint32_t)n, df.dev, rec);
		bitrank_build(rec, n_rec, ocnt.data<uint32_t>(), tmp.p, tb, s);
		if (nq) {
			KLAUNCH(k_dbg_bitrank_query, dim3(dbg_query_blocks(nq)), dim3(256), 0, s, (uint32_t)n, rec, (uint32_t)nq, dp.dev, ork.data<uint32_t>(),
				ots.data<uint32_t>());
			HIP_CHECK(copy_async(rank, ork.data<char>(), nq * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(copy_async(test, ots.data<char>(), nq * 4, hipMemcpyDeviceToHost, s));
		}
		if (records)
			HIP_CHECK(copy_async(records, orec.data<char>(), (n_rec + 1) * 16, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		return dbg_guards_intact(orec, s) && dbg_guards_intact(ocnt, s) && dbg_guards_intact(ork, s) && dbg_guards_intact(ots, s) ? 0 : DBG_RC_GUARD;
	} catch (const std::exception &) {
		return 2;
	}
}

extern "C" int povu_hip_debug_count_records(povu_hip_ctx *ctx, const uint8_t *in0, size_t n0, const uint32_t *pos0, size_t nq0, uint32_t *rec0,
					    uint32_t *prefix0, uint32_t *count0, const uint8_t *in1, size_t n1, const uint32_t *pos1, size_t nq1,
					    uint32_t *rec1, uint32_t *prefix1, uint32_t *count1, uint64_t tile[2])
{
	if (tile) {
		size_t a = 0, b = 0;
		scan_count_records_tiles(&a, &b);
		tile[0] = a, tile[1] = b;
	}
	const uint8_t *in[2] = {in0, in1};
	const size_t n[2] = {n0, in1 ? n1 : 0}, nq[2] = {nq0, in1 ? nq1 : 0};
	const uint32_t *pos[2] = {pos0, pos1};
	uint32_t *rec[2] = {rec0, rec1}, *prefix[2] = {prefix0, prefix1}, *count[2] = {count0, count1};
	if (!ctx)
		return 1;
	for (int j = 0; j < 2; j++) {
		if (n[j] > DBG_LOOKUP_MAX_N || nq[j] >= (size_t(1) << 32) || (n[j] && !in[j]) || (nq[j] && (!pos[j] || !prefix[j] || !count[j])))
			return 1;
		for (size_t i = 0; i < nq[j]; i++) // (what the word form can be asked for: [0, n))
			if (pos[j][i] >= n[j])
				return 1;
	}
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		hipStream_t s = ctx->stream;
		// the records that hold an element; the slack record behind them stays as it was (poison)
		const size_t nr[2] = {cntrec_records(n[0]) - 1, cntrec_records(n[1]) - 1}, tb = scan_tmp_bytes(std::max(n[0], n[1]));
		Arena ar;
		DbgOut orec[2] = {{(nr[0] + 1) * 16, DBG_POISON_BYTE}, {(nr[1] + 1) * 16, DBG_POISON_BYTE}};
		DbgOut opre[2] = {{nq[0] * 4}, {nq[1] * 4}}, ocnt[2] = {{nq[0] * 4}, {nq[1] * 4}};
		DbgScratch tmp{tb};
		DbgIn<uint8_t> di[2] = {{in[0], n[0]}, {in[1], n[1]}};
		DbgIn<uint32_t> dp[2] = {{pos[0], nq[0]}, {pos[1], nq[1]}};
		dbg_carve(ar, s, orec[0], orec[1], opre[0], opre[1], ocnt[0], ocnt[1], tmp, di[0], di[1], dp[0], dp[1]);
		scan_count_records_u8(di[0].dev, orec[0].data<uint4>(), n[0], in1 ? di[1].dev : nullptr, orec[1].data<uint4>(), n[1], tmp.p, tb, s);
		for (int j = 0; j < 2; j++) {
			if (nq[j]) {
				KLAUNCH(k_dbg_cntrec_query, dim3(dbg_query_blocks(nq[j])), dim3(256), 0, s, orec[j].data<uint4>(), (uint32_t)nq[j], dp[j].dev,
					opre[j].data<uint32_t>(), ocnt[j].data<uint32_t>());
				HIP_CHECK(copy_async(prefix[j], opre[j].data<char>(), nq[j] * 4, hipMemcpyDeviceToHost, s));
				HIP_CHECK(copy_async(count[j], ocnt[j].data<char>(), nq[j] * 4, hipMemcpyDeviceToHost, s));
			}
			if (rec[j] && nr[j])
				HIP_CHECK(copy_async(rec[j], orec[j].data<char>(), nr[j] * 16, hipMemcpyDeviceToHost, s));
		}
		std::vector<unsigned char> slack(32);
		for (int j = 0; j < 2; j++)
			HIP_CHECK(copy_async(slack.data() + 16 * j, orec[j].data<char>() + nr[j] * 16, 16, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		for (unsigned char c : slack) // (nothing is written behind the last record that holds an element)
			if (c != (unsigned char)DBG_POISON_BYTE)
				return DBG_RC_GUARD;
		for (int j = 0; j < 2; j++)
			if (!dbg_guards_intact(orec[j], s) || !dbg_guards_intact(opre[j], s) || !dbg_guards_intact(ocnt[j], s))
				return DBG_RC_GUARD;
		return 0;
	} catch (const std::exception &) {
		return 2;
	}
}

extern "C" int povu_hip_debug_append(povu_hip_ctx *ctx, const uint8_t *flags, size_t n, uint32_t *list, uint32_t *count)
{
	if (!ctx || !count || n > DBG_LOOKUP_MAX_N || (n && (!flags || !list)))
		return 1;
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		hipStream_t s = ctx->stream;
		Arena ar;
		DbgOut ol{n * 4}, oc{4};
		DbgIn<uint8_t> df{flags, n};
		dbg_carve(ar, s, ol, oc, df);
		HIP_CHECK(hipMemsetAsync(oc.data<char>(), 0, 4, s)); // the list is empty
		if (n)
			KLAUNCH(k_dbg_append, dim3((unsigned)((n + LIST_SPAN - 1) / LIST_SPAN)), dim3(LIST_TPB), 0, s, (uint32_t)n, df.dev, ol.data<uint32_t>(),
				oc.data<uint32_t>());
		if (n)
			HIP_CHECK(copy_async(list, ol.data<char>(), n * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(count, oc.data<char>(), 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		if (!dbg_guards_intact(ol, s) || !dbg_guards_intact(oc, s))
			return DBG_RC_GUARD;
		// (`count` entries were due: what lies behind them is a guard as well)
		return dbg_all_guard(list, std::min<size_t>(*count, n) * 4, n * 4) ? 0 : DBG_RC_GUARD;
	} catch (const std::exception &) {
		return 2;
	}
}

// ---- unit-test hook for the list ranking (list_rank.hip, debug_list_rank)
extern "C" int povu_hip_debug_list_rank(povu_hip_ctx *ctx, uint32_t n, const uint32_t *next, const uint8_t *w, const uint32_t *heads,
					uint32_t nh, int mode, uint32_t bits, uint32_t *ra, uint32_t *rb)
{
	if (!ctx || !next || !w || (nh && !heads) || !ra || (mode != 0 && !rb) || mode < 0 || mode > 1)
		return 1;
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		ctx->dbg_rank_stats.valid = false;
		debug_list_rank(n, next, w, heads, nh, mode, bits, ra, rb, ctx->stream, &ctx->dbg_rank_stats, &ctx->dbg_rank_plane0);
		return 0;
	} catch (const std::exception &) {
		return 2;
	}
}

// ---- what the level-0 walks left in their records (list_rank.hip, k_rank_rec_stats): read-only, no launch.  The numbers
// were counted by a kernel of its own behind the ranking -- in a pass only when POVU_HIP_RANK_STATS was set while it ran
extern "C" int povu_hip_debug_rank_escapes(povu_hip_ctx *ctx, int which, povu_hip_rank_records *out, uint8_t *esc, size_t n_esc)
{
	if (!ctx || !out || which < 0 || which > 2 || (esc && which != 2))
		return 1;
	if (which < 2 && !ctx->last.valid)
		return 1;
	const RankRecStats &st = which == 2 ? ctx->dbg_rank_stats : ctx->tw.rec_stats[which];
	if (!st.valid)
		return 3; // nothing was collected
	if (esc && n_esc != ctx->dbg_rank_plane0.size())
		return 1;
	out->live = st.live;
	out->escaped = st.esc;
	out->final_ranks = st.fin;
	out->bucket_bits = st.bits;
	out->delta_bits = st.delta_bits;
	out->partial_bits[0] = st.part_bits[0];
	out->partial_bits[1] = st.part_bits[1];
	std::copy(st.hist, st.hist + 33 * 33, out->hist);
	if (esc)
		for (size_t x = 0; x < n_esc; x++)
			esc[x] = st.fin ? 1 : (uint8_t)((ctx->dbg_rank_plane0[x] & REC_ESC) != 0);
	return 0;
}

// ---- timing hook for the scans: `reps` exclusive sum scans of n words (device resident, all ones), ms per scan by HIP events
extern "C" double povu_hip_debug_scan_time(povu_hip_ctx *ctx, size_t n, int reps, int op)
{
	if (!ctx || !n || reps <= 0)
		return -1.0;
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		hipStream_t s = ctx->stream;
		Arena ar;
		const size_t tb = scan_tmp_bytes(n);
		uint32_t *di = nullptr, *dout = nullptr;
		void *tmp = nullptr;
		carve(ar, [&](Spans &take) {
			take(n + 16, di, dout);
			take(tb, tmp);
		});
		HIP_CHECK(hipMemsetAsync(di, 1, n * 4, s));
		hipEvent_t e0, e1;
		HIP_CHECK(hipEventCreate(&e0));
		HIP_CHECK(hipEventCreate(&e1));
		for (int w = 0; w < 2; w++)
			op ? scan_exclusive_max_u32(di, dout, n, tmp, tb, s) : scan_exclusive_u32(di, dout, n, tmp, tb, s);
		HIP_CHECK(hipEventRecord(e0, s));
		for (int r = 0; r < reps; r++)
			op ? scan_exclusive_max_u32(di, dout, n, tmp, tb, s) : scan_exclusive_u32(di, dout, n, tmp, tb, s);
		HIP_CHECK(hipEventRecord(e1, s));
		HIP_CHECK(hipEventSynchronize(e1));
		float ms = 0;
		HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
		(void)hipEventDestroy(e0);
		(void)hipEventDestroy(e1);
		return (double)ms / reps;
	} catch (const std::exception &) {
		return -2.0;
	}
}

// ---- stage-level parity hooks
extern "C" int povu_hip_debug_components(povu_hip_ctx *ctx, uint32_t *comp_of, uint32_t *local_idx)
{
	if (!ctx || !ctx->last.valid)
		return 1;
	ctx->quiesce();
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		const uint32_t V = ctx->g.V, C = ctx->last.C;
		std::vector<uint32_t> pos(V), voff(C + 1);
		HIP_CHECK(hipMemcpy(comp_of, ctx->cs.comp_of, (size_t)V * 4, hipMemcpyDeviceToHost));
		if (ctx->cs.lean_identity)
			std::iota(pos.begin(), pos.end(), 0u);
		else
			HIP_CHECK(hipMemcpy(pos.data(), ctx->cs.pos, (size_t)V * 4, hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(voff.data(), ctx->cs.voff, (size_t)(C + 1) * 4, hipMemcpyDeviceToHost));
		for (uint32_t v = 0; v < V; v++)
			local_idx[v] = pos[v] - voff[comp_of[v]];
		return 0;
	} catch (const std::exception &) {
		return 2;
	}
}

// ---- rows A and B alone.  Both hooks read arrays the context owns (the resident graph, the row-B workspace): there is no
// buffer of their own to put between guard bands.
extern "C" int povu_hip_debug_csr(povu_hip_ctx *ctx, uint32_t *off, uint32_t *adj, uint32_t *aoth, uint32_t *atwin, uint8_t *tip,
				  uint32_t words[4])
{
	if (!ctx || !ctx->g.block || !off || !adj || !aoth || !atwin || !tip || !words)
		return 1;
	ctx->quiesce();
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		const ResidentGraph &g = ctx->g;
		const size_t V = g.V, n = g.n_slots;
		HIP_CHECK(hipMemcpy(off, g.off, (2 * V + 1) * 4, hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(tip, g.tip, V, hipMemcpyDeviceToHost));
		if (n) {
			HIP_CHECK(hipMemcpy(adj, g.adj, n * 4, hipMemcpyDeviceToHost));
			HIP_CHECK(hipMemcpy(aoth, g.aoth, n * 4, hipMemcpyDeviceToHost));
			HIP_CHECK(hipMemcpy(atwin, g.atwin, n * 4, hipMemcpyDeviceToHost));
		}
		words[0] = g.n_slots, words[1] = g.max_vdeg, words[2] = g.n_empty_sides, words[3] = g.slot_fill ? 1u : 0u;
		return 0;
	} catch (const std::exception &) {
		return 2;
	}
}

extern "C" int povu_hip_debug_row_b(povu_hip_ctx *ctx, uint32_t flags, povu_hip_rowb *out)
{
	if (!ctx || !ctx->g.block || !out || !out->voff || !out->eoff || !out->comp || !out->pos || !out->loff || !out->ladj || !out->lle ||
	    !out->start_key)
		return 1;
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		ctx->wait_tail();
		const povu_hip_opts o{0, 1, flags};
		const PassPlan p = plan_pass(&o);
		const Sizes z = rowb_begin(ctx, p); // (forgets the pass before: ctx->last)
		const RowB rb = row_b(ctx, p, z, ctx->timer);
		ctx->host.wait(rb.sizes);
		hipStream_t s = ctx->stream;
		HIP_CHECK(hipStreamSynchronize(s));
		const ResidentGraph &g = ctx->g;
		const CompState &cs = ctx->cs;
		const size_t V = g.V, C = rb.C, nS = 2 * V;
		out->n_components = rb.C;
		out->stats0 = rb.gstats[0];
		out->n_cross = cs.n_cross;
		const bool identity = rb.C == 1 || cs.comp_sorted;
		out->path_bits = (identity ? POVU_HIP_ROWB_IDENTITY : 0u) | (sort_free_adjacency(g, p.sorted_adj) ? POVU_HIP_ROWB_SORT_FREE : 0u) |
				 (cs.lean_identity ? POVU_HIP_ROWB_LEAN_IDENTITY : 0u) | (cs.has_self_loops ? POVU_HIP_ROWB_SELF_LOOPS : 0u) |
				 (cs.dense_edges ? POVU_HIP_ROWB_DENSE_EDGES : 0u) | (cs.spec_adj_kept ? POVU_HIP_ROWB_SPEC_KEPT : 0u);
		std::copy(rb.voff, rb.voff + C + 1, out->voff); // (as the pass reads them: published into page-locked memory)
		std::copy(rb.eoff, rb.eoff + C + 1, out->eoff);
		HIP_CHECK(hipMemcpy(out->comp, cs.comp_of, V * 4, hipMemcpyDeviceToHost));
		if (cs.lean_identity)
			std::iota(out->pos, out->pos + V, 0u);
		else
			HIP_CHECK(hipMemcpy(out->pos, cs.pos, V * 4, hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(out->loff, cs.loff, (nS + 1) * 4, hipMemcpyDeviceToHost));
		const size_t n = out->loff[nS];
		out->n_local_slots = (uint32_t)n;
		if (n > 2 * (size_t)g.E)
			return 2; // (more local slots than two a link: the caller's arrays would not hold them)
		if (n) {
			HIP_CHECK(hipMemcpy(out->ladj, cs.ladj, n * 4, hipMemcpyDeviceToHost));
			HIP_CHECK(hipMemcpy(out->lle, cs.lle, n * 4, hipMemcpyDeviceToHost));
		}
		if (C)
			HIP_CHECK(hipMemcpy(out->start_key, cs.start_key, C * 8, hipMemcpyDeviceToHost));
		return 0;
	} catch (const std::exception &) {
		if (ctx->stream)
			(void)hipStreamSynchronize(ctx->stream);
		return 2;
	}
}

extern "C" int povu_hip_debug_tree(povu_hip_ctx *ctx, uint32_t comp, uint32_t *n_tree, uint32_t *gid, uint8_t *typ,
				   uint32_t *par, uint32_t *cls)
{
	if (!ctx || !ctx->last.valid || comp >= ctx->last.C || !n_tree)
		return 1;
	if (cls && ctx->last.mixed)
		return 4; // classes of a mixed pass sit in two layouts (parallel stage / one-lane kernels): not exported
	ctx->quiesce();
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		uint32_t voff = 0, N = 0;
		HIP_CHECK(hipMemcpy(&voff, ctx->cs.voff + comp, 4, hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(&N, ctx->sw.c_ntree + comp, 4, hipMemcpyDeviceToHost));
		*n_tree = N;
		const size_t tb = 2 * (size_t)voff + comp;
		if (gid)
			HIP_CHECK(hipMemcpy(gid, ctx->sw.t_gid + tb, (size_t)N * 4, hipMemcpyDeviceToHost));
		if (par)
			HIP_CHECK(hipMemcpy(par, ctx->sw.t_par + tb, (size_t)N * 4, hipMemcpyDeviceToHost));
		const bool par_cls = !ctx->last.plan.all_seq && (ctx->last.seq_redo == 0 || ctx->last.redo_pvst_only);
		if (cls && par_cls) {
			classes_to_tree_space(ctx->pw, ctx->stream);
			HIP_CHECK(hipStreamSynchronize(ctx->stream));
		}
		if (cls) // the parallel class stage keeps the classes in its own T-space array
			HIP_CHECK(hipMemcpy(cls, (par_cls ? ctx->pw.gcls : ctx->sw.t_cls) + tb, (size_t)N * 4, hipMemcpyDeviceToHost));
		if (typ)
			HIP_CHECK(hipMemcpy(typ, ctx->sw.t_flags + tb, N, hipMemcpyDeviceToHost));
		return 0;
	} catch (const std::exception &) {
		return 2;
	}
}

extern "C" int povu_hip_debug_edge_ids(povu_hip_ctx *ctx, uint32_t comp, uint32_t *n_tree, uint32_t *tree_edge_id)
{
	if (!ctx || !ctx->last.valid || comp >= ctx->last.C || !n_tree)
		return 1;
	if (!ctx->last.plan.par_tree)
		return 3; // the one-lane tree kernels keep no per-side scan state
	if (ctx->last.mixed)
		return 4; // (see povu_hip_debug_tree)
	uint32_t *dw = nullptr;
	ctx->quiesce();
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		uint32_t voff = 0, N = 0;
		HIP_CHECK(hipMemcpy(&voff, ctx->cs.voff + comp, 4, hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(&N, ctx->sw.c_ntree + comp, 4, hipMemcpyDeviceToHost));
		*n_tree = N;
		if (!tree_edge_id || N == 0)
			return 0;
		const size_t T = 2 * (size_t)ctx->sw.V + ctx->last.C, tb = 2 * (size_t)voff + comp;
		HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&dw), 2 * T * 4));
		HIP_CHECK(hipMemsetAsync(dw, 0, 2 * T * 4, ctx->stream));
		edge_id_weights(ctx->cs, ctx->sw, ctx->tw, dw, dw + T, ctx->stream);
		std::vector<uint32_t> w(N), tail(N), size(N);
		HIP_CHECK(copy_async(w.data(), dw + tb, (size_t)N * 4, hipMemcpyDeviceToHost, ctx->stream));
		HIP_CHECK(copy_async(tail.data(), dw + T + tb, (size_t)N * 4, hipMemcpyDeviceToHost, ctx->stream));
		HIP_CHECK(copy_async(size.data(), ctx->sw.t_size + tb, (size_t)N * 4, hipMemcpyDeviceToHost, ctx->stream));
		HIP_CHECK(hipStreamSynchronize(ctx->stream));
		HIP_CHECK(hipFree(dw));
		dw = nullptr;
		// back edges created before vertex t is discovered: those in front of every vertex up to t, and the tails of
		// the vertices whose subtree closed before t
		std::vector<uint32_t> closed((size_t)N + 1, 0);
		for (uint32_t t = 0; t < N; t++)
			closed[std::min<size_t>((size_t)t + size[t], N)] += tail[t];
		uint32_t before = 0;
		tree_edge_id[0] = POVU_NIL;
		for (uint32_t t = 0; t < N; t++) {
			before += w[t] + closed[t];
			if (t > 0)
				tree_edge_id[t] = t - 1 + before;
		}
		return 0;
	} catch (const std::exception &) {
		if (dw)
			(void)hipFree(dw);
		return 2;
	}
}

// the class walks' counter words of the last pass (cleared ahead of the tree stage, written by it alone): read-only, no launch
extern "C" int povu_hip_debug_walk_words(povu_hip_ctx *ctx, uint32_t out[3])
{
	if (!ctx || !ctx->last.valid || !out)
		return 1;
	if (!ctx->last.plan.par_tree)
		return 3; // the one-lane tree kernels walk no classes
	if (ctx->last.mixed)
		return 4; // (see povu_hip_debug_tree)
	ctx->quiesce();
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		const int words[3] = {PW_N_ENTRY, PW_N_OVER, PW_POOL_TOP};
		for (int i = 0; i < 3; i++)
			HIP_CHECK(hipMemcpy(out + i, ctx->pw.err + words[i], 4, hipMemcpyDeviceToHost));
		return 0;
	} catch (const std::exception &) {
		return 2;
	}
}

// how full the splice of the last -s pass left component comp's stretch of the children-vector pool: out[0] = slots taken
// (ptop - poff), out[1] = slots it had (layout_splice's budget).  Read-only, no launch; the pass itself records two pointers.
extern "C" int povu_hip_debug_splice_pool(povu_hip_ctx *ctx, uint32_t comp, uint32_t out[2])
{
	if (!ctx || !ctx->last.valid || !out)
		return 1;
	if (!ctx->last.plan.all_sub || !ctx->ws_sub.pool_off)
		return 3; // the last pass ran no inserting passes
	if (comp >= ctx->last.C || comp >= ctx->ws_sub.pool_comps)
		return 5; // no such component
	ctx->quiesce();
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		uint32_t off[2] = {0, 0}, top = 0;
		HIP_CHECK(hipMemcpy(off, ctx->ws_sub.pool_off + comp, 8, hipMemcpyDeviceToHost));
		top = off[0];
		if (ctx->ws_sub.pool_top)
			HIP_CHECK(hipMemcpy(&top, ctx->ws_sub.pool_top + comp, 4, hipMemcpyDeviceToHost));
		out[0] = top - off[0];
		out[1] = off[1] - off[0];
		return 0;
	} catch (const std::exception &) {
		return 2;
	}
}

extern "C" int povu_hip_debug_stack(povu_hip_ctx *ctx, uint32_t comp, uint32_t *n, uint32_t *tree_vtx, uint32_t *cls,
				    uint32_t *next_seen)
{
	if (!ctx || !ctx->last.valid || comp >= ctx->last.C || !n)
		return 1;
	if (ctx->last.mixed)
		return 4; // the candidate stacks of a mixed pass sit in two layouts: not exported (see povu_hip_debug_tree)
	ctx->quiesce();
	try {
		HIP_CHECK(hipSetDevice(ctx->device));
		if (ctx->last.stack_export_pending && ctx->last.seq_redo == 0) {
			export_parallel_stack(ctx->cs, ctx->sw, ctx->pw, ctx->stream);
			HIP_CHECK(hipStreamSynchronize(ctx->stream));
			ctx->last.stack_export_pending = false;
		}
		uint32_t voff = 0, ns = 0;
		HIP_CHECK(hipMemcpy(&voff, ctx->cs.voff + comp, 4, hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(&ns, ctx->sw.c_nstack + comp, 4, hipMemcpyDeviceToHost));
		*n = ns;
		if (tree_vtx)
			HIP_CHECK(hipMemcpy(tree_vtx, ctx->sw.s_vtx + voff, (size_t)ns * 4, hipMemcpyDeviceToHost));
		if (cls)
			HIP_CHECK(hipMemcpy(cls, ctx->sw.s_cls + voff, (size_t)ns * 4, hipMemcpyDeviceToHost));
		if (next_seen)
			HIP_CHECK(hipMemcpy(next_seen, ctx->sw.next_seen + voff, (size_t)ns * 4, hipMemcpyDeviceToHost));
		return 0;
	} catch (const std::exception &) {
		return 2;
	}
}
