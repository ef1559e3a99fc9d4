// query_common.hpp -- what the walks (walk_kernels.hip) and the traversals (trav_kernels.hip) share: the queries of a forest
// (every PVST vertex but the roots, tree order then vertex order), the refusals of forests they cannot read, the resolution
// of a query's boundary steps to entered sides on the device (segment ids must ascend with the vertex index), and the C ABI
// side of a call: its timing, its errors and the hand-off of its results to the host.  Defined in query_common.hip.
#pragma once
#include "context.hpp"

#include <functional>

namespace povu_hip
{

static constexpr uint32_t NO_QUERY = 0xFFFFFFFFu;

// vertex index of segment `id` in the ascending `vid`, NO_QUERY when the graph has no such segment
__device__ __forceinline__ uint32_t find_vertex(const uint32_t *__restrict__ vid, uint32_t V, uint32_t id)
{
	uint32_t lo = 0, hi = V;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (vid[mid] < id)
			lo = mid + 1;
		else
			hi = mid;
	}
	return (lo < V && vid[lo] == id) ? lo : NO_QUERY;
}

// throws unless `f` was made by povu_hip_decompose on `ctx` from the graph now resident there (no shard, merge or attach);
// `what` names the caller in the message ("walks", "traversals")
void check_query_forest(const povu_hip_ctx *ctx, const povu_hip_forest *f, const char *what);
// bit 0 of *bad when vid does not ascend
void launch_vid_ascending(uint32_t V, const uint32_t *vid, uint32_t *bad, hipStream_t s);

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
