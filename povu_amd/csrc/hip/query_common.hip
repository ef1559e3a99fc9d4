// query_common.hip -- the front end the query pipelines share: the queries of a forest, their upload and the two checks that
// resolve them to entered sides; the iota and the 2^32 refusal (query_common.hpp).
#include "query_common.hpp"

namespace povu_hip
{

// segment ids must ascend with the vertex index (binary search; successor order = side order)
__global__ void k_wk_vid_ascending(uint32_t V, const uint32_t *__restrict__ vid, uint32_t *__restrict__ bad)
{
	const uint32_t i = blockIdx.x * Q_TPB + threadIdx.x;
	if (i + 1 < V && vid[i] >= vid[i + 1])
		atomicOr(bad, 1u);
}

// (id, orientation) of both boundaries -> entered sides; a query whose two boundaries are one segment has no walk (NO_QUERY)
__global__ void k_wk_resolve(uint32_t n, const uint32_t *__restrict__ qa, const uint32_t *__restrict__ qz,
			       const uint8_t *__restrict__ qor, const uint32_t *__restrict__ vid, uint32_t V, uint32_t *__restrict__ ys,
			       uint32_t *__restrict__ yz, uint32_t *__restrict__ bad)
{
	const uint32_t q = blockIdx.x * Q_TPB + threadIdx.x;
	if (q >= n)
		return;
	const uint32_t a = find_vertex(vid, V, qa[q]), z = find_vertex(vid, V, qz[q]);
	if (a == NO_QUERY || z == NO_QUERY) {
		atomicOr(bad, 2u);
		ys[q] = yz[q] = NO_QUERY;
		return;
	}
	const uint8_t o = qor[q];
	ys[q] = a == z ? NO_QUERY : 2 * a + (o & 1u);
	yz[q] = a == z ? NO_QUERY : 2 * z + ((o >> 1) & 1u);
}

__global__ void k_q_iota(uint32_t n, uint32_t *__restrict__ a)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < n; i += gridDim.x * Q_TPB)
		a[i] = i;
}

void launch_iota(uint32_t n, uint32_t *a, hipStream_t s)
{
	KLAUNCH(k_q_iota, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, a);
}

void refuse_2_32(uint64_t v, const char *who, const char *what, const char *why)
{
	if (v >= 0xFFFFFFFFull)
		throw HipError(std::string(who) + std::to_string(v) + " " + what + ": 2^32 or more are refused" + why);
}

void launch_vid_ascending(uint32_t V, const uint32_t *vid, uint32_t *bad, hipStream_t s)
{
	KLAUNCH(k_wk_vid_ascending, dim3(lane_blocks(V)), dim3(Q_TPB), 0, s, V, vid, bad);
}

void check_query_forest(const povu_hip_ctx *ctx, const povu_hip_forest *f, const char *what)
{
	if (!ctx || !f)
		throw HipError("null context or forest");
	if (!f->walk_ctx)
		throw HipError(std::string(what) +
			       " need a forest made by povu_hip_decompose of a whole resident graph (not a sharded, merged or attached forest)");
	if (f->walk_ctx != ctx || !ctx->g.block || f->walk_gen != ctx->g.gen)
		throw HipError("the forest was not decomposed from the graph now resident on this context (it was uploaded again, or the forest belongs to another context)");
}

// (S id, Z id, or1 | or2 << 1) of every query of `f`
static void forest_queries(povu_hip_forest *f, std::vector<uint32_t> &qa, std::vector<uint32_t> &qz, std::vector<uint8_t> &qor)
{
	const uint32_t n_trees = (uint32_t)f->trees.size();
	for (uint32_t i = 0; i < n_trees; i++) {
		povu_hip_subtree st;
		if (povu_hip_forest_get_subtree(f, i, &st) == 0) {
			for (uint32_t v = 1; v < st.n_total; v++) {
				qa.push_back(st.id1[v]);
				qz.push_back(st.id2[v]);
				qor.push_back((uint8_t)((st.or1[v] & 1u) | ((st.or2[v] & 1u) << 1)));
			}
			continue;
		}
		povu_hip_tree t;
		if (povu_hip_forest_get(f, i, &t) != 0)
			throw HipError("forest tree " + std::to_string(i) + " unreadable");
		for (uint32_t v = 1; v < t.n_pvst; v++) {
			qa.push_back(t.a_id[v]);
			qz.push_back(t.z_id[v]);
			qor.push_back((uint8_t)((t.a_or[v] & 1u) | ((t.z_or[v] & 1u) << 1)));
		}
	}
	if (qa.size() >= 0xFFFFFFFFull)
		throw HipError("too many queries for 32-bit indices");
}

QueryFront query_front(povu_hip_ctx *ctx, povu_hip_forest *f, Arena &A, CallTimer &timer, const QueryLayout &more)
{
	HIP_CHECK(hipSetDevice(ctx->device));
	ctx->wait_tail();
	f->ready();
	std::vector<uint32_t> qa, qz;
	std::vector<uint8_t> qor;
	forest_queries(f, qa, qz, qor);
	return query_front(ctx, std::move(qa), std::move(qz), std::move(qor), A, timer, more);
}

QueryFront query_front(povu_hip_ctx *ctx, std::vector<uint32_t> qa, std::vector<uint32_t> qz, std::vector<uint8_t> qor, Arena &A,
		       CallTimer &timer, const QueryLayout &more)
{
	HIP_CHECK(hipSetDevice(ctx->device));
	ctx->wait_tail();
	if (qa.size() >= 0xFFFFFFFFull)
		throw HipError("too many queries for 32-bit indices");
	const ResidentGraph &g = ctx->g;
	const hipStream_t s = ctx->stream;
	QueryFront q;
	q.n = (uint32_t)qa.size();
	const size_t n1 = (size_t)q.n + 1;
	uint32_t *d_qa, *d_qz, *ys, *yz;
	uint8_t *d_qor;
	carve(A, [&](Spans &take) {
		take(n1, d_qa, d_qz, d_qor, ys, yz);
		take(8, q.words);
		more(take, q.n);
	});
	q.qa = d_qa;
	q.qz = d_qz;
	q.ys = ys;
	q.yz = yz;

	timer.start(s);
	HIP_CHECK(hipMemsetAsync(q.words, 0, 8 * 4, s));
	if (q.n) {
		HIP_CHECK(copy_async(d_qa, qa.data(), (size_t)q.n * 4, hipMemcpyHostToDevice, s));
		HIP_CHECK(copy_async(d_qz, qz.data(), (size_t)q.n * 4, hipMemcpyHostToDevice, s));
		HIP_CHECK(copy_async(d_qor, qor.data(), q.n, hipMemcpyHostToDevice, s));
	}
	launch_vid_ascending(g.V, g.vid, q.words, s);
	if (q.n)
		KLAUNCH(k_wk_resolve, dim3(lane_blocks(q.n)), dim3(Q_TPB), 0, s, q.n, d_qa, d_qz, d_qor, g.vid, g.V, ys, yz, q.words);
	return q;
}

void query_refusals(uint32_t word0, const char *what)
{
	if (word0 & 1u)
		throw HipError(std::string(what) + " need segment ids that ascend with the vertex index (the order the GFA loader gives)");
	if (word0 & 2u)
		throw HipError("a flubble boundary of the forest is no segment of the resident graph");
}

} // namespace povu_hip
