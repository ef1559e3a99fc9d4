// query_common.hpp -- what the four query pipelines share (walks: walk_kernels.hip, traversals: trav_kernels.hip, flubble
// calls: call_kernels.hip, inversion calls: inv_kernels.hip).  Device side: the launch shapes, the step of a traversal, the
// binary searches, the wave reductions.  Host side: the queries of a forest (every PVST vertex but the roots, tree order then
// vertex order), the refusals of forests they cannot read, the resolution of a query's boundary steps to entered sides on the
// device (segment ids must ascend with the vertex index), the steps every pipeline repeats (a one-word read-back, counts to
// offsets with the 2^32 refusal, a sort by several keys), and the C ABI side of a call: its timing, its errors and the
// hand-off of its results to the host.  Defined in query_common.hip.
#pragma once
#include "context.hpp"

#include <functional>

namespace povu_hip
{

static constexpr uint32_t NO_QUERY = 0xFFFFFFFFu;
static constexpr int Q_TPB = 256;		 // lanes of a workgroup, every kernel of the four pipelines
static constexpr uint64_t ROLE_BIT = 1ull << 63; // role of a task, kept in the top bit of its position: reverse traversals carry it in rpos

// ---- launch shapes: workgroups of Q_TPB lanes with a lane per item, the same capped for kernels that stride over their
// grid, and workgroups with a wave per item (such kernels stride)
static inline unsigned lane_blocks(size_t n) { return (unsigned)std::max<size_t>(1, (n + Q_TPB - 1) / Q_TPB); }
static inline unsigned stride_blocks(size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n + Q_TPB - 1) / Q_TPB, 65536)); }
static inline unsigned wave_blocks(size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n + Q_TPB / 64 - 1) / (Q_TPB / 64), 65536)); }

// step k (S -> Z) of the traversal that occupies path words [pos, pos + len), read backwards and flipped when reverse
__device__ __forceinline__ uint32_t trav_step(const uint32_t *__restrict__ steps, uint64_t pos, uint32_t len, bool rev, uint32_t k)
{
	return rev ? steps[pos + len - 1 - k] ^ 1u : steps[pos + k];
}
// a traversal as rpos / rlen keep it, unpacked: the path words [p, p + len), reverse when rpos carries ROLE_BIT
struct TravSpan {
	uint64_t p;
	uint32_t len;
	bool rev;
	__device__ __forceinline__ uint32_t step(const uint32_t *__restrict__ steps, uint32_t k) const { return trav_step(steps, p, len, rev, k); }
	__device__ __forceinline__ uint64_t first_pos() const { return p; }
	__device__ __forceinline__ uint64_t last_pos() const { return p + len - 1; }
};
__device__ __forceinline__ TravSpan trav_span(uint64_t packed, uint32_t len) { return {packed & ~ROLE_BIT, len, (packed & ROLE_BIT) != 0}; }
__device__ __forceinline__ TravSpan trav_span(const uint64_t *__restrict__ rpos, const uint32_t *__restrict__ rlen, uint32_t t) { return trav_span(rpos[t], rlen[t]); }
// the position alone, for those that need no more
__device__ __forceinline__ uint64_t trav_first_pos(const uint64_t *__restrict__ rpos, uint32_t t) { return trav_span(rpos[t], 0).p; }

// what the kernels read of the resident paths, segments and sequences (paths_view: from the context)
struct PathsView {
	uint32_t n_paths;
	const uint64_t *path_off; // [n_paths + 1] first path word of every path, the paths concatenated
	const uint32_t *steps;	  // the path words
	const uint64_t *seq_off;  // [V + 1]
	const char *seq;
	const uint32_t *vid; // [V] segment ids, ascending
};
static inline PathsView paths_view(const povu_hip_ctx *ctx)
{
	return PathsView{ctx->n_paths, ctx->path_off, ctx->path_steps, ctx->seq_off, ctx->seq, ctx->g.vid};
}

// (the span a position lies in -- the path of a global step, the reference of a reference step, the block of a spelled
// allele: span_of, search_rules.hpp)

// sum over the wave, in every lane
template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
	return wave_all_reduce(v, ScanOp<0>{});
}
// (inclusive prefix sum over the wave: wave_inclusive_sum, common.hpp)

// vertex index of segment `id` in the ascending `vid`, NO_QUERY when the graph has no such segment
__device__ __forceinline__ uint32_t find_vertex(const uint32_t *__restrict__ vid, uint32_t V, uint32_t id)
{
	const uint32_t lo = lower_bound(vid, 0u, V, id);
	return (lo < V && vid[lo] == id) ? lo : NO_QUERY;
}

// throws unless `f` was made by povu_hip_decompose on `ctx` from the graph now resident there (no shard, merge or attach);
// `what` names the caller in the message ("walks", "traversals")
void check_query_forest(const povu_hip_ctx *ctx, const povu_hip_forest *f, const char *what);
// bit 0 of *bad when vid does not ascend
void launch_vid_ascending(uint32_t V, const uint32_t *vid, uint32_t *bad, hipStream_t s);
// a[i] = i, i < n
void launch_iota(uint32_t n, uint32_t *a, hipStream_t s);

// one value of device memory, through the stream and waited for
template <class T>
T read_back(const T *dev, hipStream_t s)
{
	T h{};
	HIP_CHECK(copy_async(&h, dev, sizeof(T), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	return h;
}

// throws "<who><v> <what>: 2^32 or more are refused<why>" when v does not fit the 32-bit indices, scans and sorts
void refuse_2_32(uint64_t v, const char *who, const char *what, const char *why = "");

// Counts to offsets: the 64-bit totals of cnt[0 .. n) (and cnt2, optional, of the same length) go to `refuse`, which throws
// in the caller's words when they do not fit; then element n is cleared and off[0 .. n] (off2) are the exclusive sums.
// tot: two words of device memory.  Waits for the stream (totals_u32).
template <class Refuse>
void counts_to_offsets(uint32_t *cnt, uint32_t *off, uint32_t *cnt2, uint32_t *off2, size_t n, unsigned long long *tot, void *tmp,
		       size_t tmp_bytes, hipStream_t s, Refuse &&refuse)
{
	uint64_t total[2] = {0, 0};
	totals_u32(cnt, cnt2, n, tot, total, s);
	refuse(total);
	HIP_CHECK(hipMemsetAsync(cnt + n, 0, 4, s));
	if (!cnt2) {
		scan_exclusive_u32(cnt, off, n + 1, tmp, tmp_bytes, s);
		return;
	}
	HIP_CHECK(hipMemsetAsync(cnt2 + n, 0, 4, s));
	scan_exclusive_u32_pair(cnt, off, n + 1, cnt2, off2, n + 1, tmp, tmp_bytes, s);
}

// A stable sort of an index list by several keys, least significant first: per key a pass -- `write_key(which, perm, key)`
// launches the caller's kernel that writes key `which` of entry perm[k] to key[k], then one radix sort of `bits` bits moves
// the list to its other buffer.  `cur` holds the list, before the first pass and after the last.
struct LsdSort {
	uint32_t *cur, *nxt; // the index list and its ping-pong buffer
	uint32_t *key, *kout;
	size_t n;
	void *tmp; // sort_tmp_bytes(n)
	size_t tmp_bytes;
	hipStream_t s;
	template <class WriteKey>
	void pass(int which, unsigned bits, WriteKey &&write_key)
	{
		write_key(which, static_cast<const uint32_t *>(cur), key);
		sort_pairs_u32(key, kout, cur, nxt, n, bits, tmp, tmp_bytes, s);
		std::swap(cur, nxt);
	}
};

// HIP-event time of a call's device work, from start() to stop(); the events go with the scope on every exit
class CallTimer
{
public:
	CallTimer() = default;
	CallTimer(const CallTimer &) = delete;
	CallTimer &operator=(const CallTimer &) = delete;
	~CallTimer()
	{
		if (e0_)
			(void)hipEventDestroy(e0_);
		if (e1_)
			(void)hipEventDestroy(e1_);
	}
	void start(hipStream_t s)
	{
		HIP_CHECK(hipEventCreate(&e0_));
		HIP_CHECK(hipEventCreate(&e1_));
		HIP_CHECK(hipEventRecord(e0_, s));
	}
	// records the end, waits for the stream and gives the milliseconds since start()
	float stop(hipStream_t s)
	{
		HIP_CHECK(hipEventRecord(e1_, s));
		HIP_CHECK(hipStreamSynchronize(s));
		float ms = 0;
		(void)hipEventElapsedTime(&ms, e0_, e1_);
		return ms;
	}

private:
	hipEvent_t e0_ = nullptr, e1_ = nullptr;
};

// The device side of a forest's queries (query_front)
struct QueryFront {
	uint32_t n = 0;			      // queries
	const uint32_t *qa = nullptr, *qz = nullptr; // [n + 1] segment ids of both boundaries
	const uint32_t *ys = nullptr, *yz = nullptr; // [n + 1] entered sides of both boundaries, NO_QUERY for a query whose
						      // boundaries are one segment
	uint32_t *words = nullptr;		      // [8] cleared: word 0 takes the checks' bits (query_refusals), 1..7 are the caller's
};
// the caller's arrays, sized by the number of queries
using QueryLayout = std::function<void(Spans &take, uint32_t n)>;
// The front end of a query call, behind the caller's refusals of its options: the device made current and idle, the queries
// of `f` built, their arrays carved from `A` together with the caller's (`more`), `timer` started, the queries uploaded and
// both checks enqueued.  Nothing is waited for: the caller reads `words` back with what it enqueues behind them and hands
// word 0 to query_refusals.
QueryFront query_front(povu_hip_ctx *ctx, povu_hip_forest *f, Arena &A, CallTimer &timer, const QueryLayout &more);
// ... of explicit queries: per query the S id, the Z id and or1 | or2 << 1 (povu_hip_call's sites)
QueryFront query_front(povu_hip_ctx *ctx, std::vector<uint32_t> qa, std::vector<uint32_t> qz, std::vector<uint8_t> qor, Arena &A,
		       CallTimer &timer, const QueryLayout &more);
// the refusals of the checks, from bits of word 0 (bit 0: vid does not ascend, bit 1: a boundary is no segment of the graph);
// `what` names the caller in the first ("walks", "traversals", "paths")
void query_refusals(uint32_t word0, const char *what);

// A C ABI call: `body` under the context's transfer tally; an exception waits for the stream (nothing of the call may still
// run when its arena is used again), goes to `err` and makes the call return `failed`
template <class R, class Body>
R guarded_call(povu_hip_ctx *ctx, char *err, size_t errlen, R failed, Body &&body)
{
	XferScope xfer(ctx);
	try {
		return body();
	} catch (const std::exception &e) {
		if (ctx && ctx->stream)
			(void)hipStreamSynchronize(ctx->stream);
		set_err(err, errlen, e.what());
		return failed;
	}
}

// a result to the host: `v` sized `size` from the context's pool, its first n elements copied from `dev` when n > 0
template <typename T>
void hand_off(PinnedVec<T> &v, size_t size, const T *dev, size_t n, povu_hip_ctx *ctx)
{
	v.resize(size, ctx->pool);
	if (n)
		HIP_CHECK(copy_async(v.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
}

// The traversal pipeline of povu_hip_forest_traversals behind a query front end (`front` carves the queries from the
// traversals' first arena): its refusals of the options and of missing paths, its kernels, and its results left on the
// device in the context's traversal arenas (valid until the next traversal call on the context).  Per query: toff, aoff
// (u32 offsets), qstatus; per traversal (in (query, path, first) order): rq (query), op (path), of / ol (first / last step),
// oa (allele within the query), orv (reverse), rpos (global position of its first step | ROLE_BIT when reverse), rlen
// (steps); per allele: afirst (its first traversal), soff (u32 step offsets); per allele step: sid (segment id), sor.
using QueryFrontFn = std::function<QueryFront(CallTimer &timer, const QueryLayout &more)>;
struct TravDevice {
	QueryFront q;
	uint32_t R = 0, n_al = 0, n2 = 0;
	uint64_t n_steps = 0, n_splits = 0;
	uint32_t *op, *of, *ol, *oa, *sid, *toff, *aoff, *qstatus, *soff, *rq, *rlen, *afirst;
	uint8_t *orv, *sor;
	uint64_t *rpos;
};
TravDevice trav_pipeline(povu_hip_ctx *ctx, const QueryFrontFn &front, const povu_hip_trav_opts *opts, CallTimer &timer);

} // namespace povu_hip
