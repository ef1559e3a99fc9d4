// povu_hip.hip -- C ABI (include/povu_hip.h) and host orchestration of the gfx950
// decompose path.  Mirrors povu::subcommands::decompose::do_decompose
// (app/subcommand/decompose.cpp:94-160) from "graph built" to "PVST ready to write".
#include "context.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <numeric>

#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

using namespace povu_hip;

// ---- page-locked result blocks (context.hpp)
PinnedPool::~PinnedPool()
{
	for (auto &b : free_blocks)
		if (b.seg < 0)
			(void)hipHostFree(b.p);
	for (auto &sg : segments) {
		(void)hipHostUnregister(sg.p);
		(void)munmap(sg.p, sg.cap);
		(void)shm_unlink(segment_name(shared_tag, sg.seg).c_str());
	}
}

void *PinnedPool::get(size_t bytes, size_t &cap, int *seg)
{
	const bool shared = !shared_tag.empty();
	{
		// best fit: a pass with -s takes two blocks of different sizes (the PVST arrays, the extended trees); first fit let the
		// smaller request walk off with the larger block, and the larger one page-locked a fresh 0.7 GB every call (60 ms)
		std::lock_guard<std::mutex> g(m);
		size_t best = free_blocks.size();
		for (size_t i = 0; i < free_blocks.size(); i++)
			if (free_blocks[i].cap >= bytes && (free_blocks[i].seg >= 0) == shared &&
			    (best == free_blocks.size() || free_blocks[i].cap < free_blocks[best].cap))
				best = i;
		if (best != free_blocks.size()) {
			const Block b = free_blocks[best];
			free_blocks.erase(free_blocks.begin() + best);
			cap = b.cap;
			if (seg)
				*seg = b.seg;
			return b.p;
		}
	}
	void *p = nullptr;
	cap = bytes + bytes / 4 + 4096;
	if (!shared) {
		if (hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess)
			throw HipError("hipHostMalloc failed for the PVST result block");
		if (seg)
			*seg = -1;
		return p;
	}
	// a named segment, page-locked and mapped for the device where it is
	cap = (cap + 4095) & ~size_t(4095);
	int k;
	{
		std::lock_guard<std::mutex> g(m);
		k = next_seg++;
	}
	const std::string name = segment_name(shared_tag, k);
	(void)shm_unlink(name.c_str()); // (a stale segment of a crashed job with the same tag)
	const int fd = shm_open(name.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
	if (fd < 0)
		throw HipError("shm_open failed for the shared PVST result block " + name);
	if (ftruncate(fd, (off_t)cap) != 0) {
		(void)close(fd);
		(void)shm_unlink(name.c_str());
		throw HipError("not enough shared memory for the PVST result block " + name + " (" + std::to_string(cap >> 20) + " MiB)");
	}
	p = mmap(nullptr, cap, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_POPULATE, fd, 0);
	(void)close(fd);
	if (p == MAP_FAILED) {
		(void)shm_unlink(name.c_str());
		throw HipError("mmap failed for the shared PVST result block " + name);
	}
	if (hipHostRegister(p, cap, hipHostRegisterMapped | hipHostRegisterPortable) != hipSuccess) {
		(void)hipGetLastError();
		(void)munmap(p, cap);
		(void)shm_unlink(name.c_str());
		throw HipError("hipHostRegister failed for the shared PVST result block " + name);
	}
	{
		std::lock_guard<std::mutex> g(m);
		segments.push_back(Block{p, cap, k});
	}
	if (seg)
		*seg = k;
	return p;
}

extern "C" int povu_hip_share_results(povu_hip_ctx *ctx, const char *tag, char *err, size_t errlen)
{
	if (!ctx || !tag || !*tag || strlen(tag) > 96 || strchr(tag, '/')) {
		set_err(err, errlen, "share_results: bad tag");
		return 1;
	}
	// a fresh pool: blocks of the old one go back to it as their forests are freed
	auto pool = std::make_shared<PinnedPool>();
	pool->shared_tag = tag;
	ctx->pool = pool;
	return 0;
}

extern "C" int povu_hip_transfer_bytes(const povu_hip_ctx *ctx, uint64_t out[4])
{
	if (!ctx || !out)
		return 1;
	out[0] = ctx->xfer_h2d, out[1] = ctx->xfer_d2h, out[2] = ctx->xfer_peer_out, out[3] = ctx->xfer_peer_in;
	return 0;
}

void set_err(char *err, size_t errlen, const std::string &msg)
{
	if (err && errlen) {
		snprintf(err, errlen, "%s", msg.c_str());
	}
}

extern "C" const char *povu_hip_version(void) { return "povu-hip 0.1.0 (gfx950)"; }

extern "C" int povu_hip_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

extern "C" povu_hip_ctx *povu_hip_create(int device, char *err, size_t errlen)
{
	try {
		int n = 0;
		if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
			throw HipError("no HIP device available: the decompose path has no CPU fallback");
		if (device < 0 || device >= n)
			throw HipError("HIP device index out of range");
		HIP_CHECK(hipSetDevice(device));
		auto ctx = std::make_unique<povu_hip_ctx>();
		ctx->device = device;
		HIP_CHECK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
		HIP_CHECK(hipStreamCreateWithFlags(&ctx->side.stream, hipStreamNonBlocking));
		HIP_CHECK(hipEventCreateWithFlags(&ctx->side.fork, hipEventDisableTiming));
		HIP_CHECK(hipEventCreateWithFlags(&ctx->side.join, hipEventDisableTiming));
		HIP_CHECK(hipEventCreateWithFlags(&ctx->side.fork2, hipEventDisableTiming));
		HIP_CHECK(hipStreamCreateWithFlags(&ctx->walk_side.stream, hipStreamNonBlocking));
		HIP_CHECK(hipEventCreateWithFlags(&ctx->walk_side.fork, hipEventDisableTiming));
		HIP_CHECK(hipEventCreateWithFlags(&ctx->walk_side.join, hipEventDisableTiming));
		HIP_CHECK(hipEventCreateWithFlags(&ctx->tail_done, hipEventDisableTiming));
		ctx->timer.stream = ctx->stream;
		return ctx.release();
	} catch (const std::exception &e) {
		set_err(err, errlen, e.what());
		return nullptr;
	}
}

void free_resident_graph(ResidentGraph &g)
{
	g = ResidentGraph{}; // the block belongs to the context's graph arena, which keeps it for the next graph
}

extern "C" int povu_hip_release_workspace(povu_hip_ctx *ctx)
{
	if (!ctx)
		return 1;
	(void)hipSetDevice(ctx->device);
	ctx->quiesce();
	ctx->wait_tail();
	(void)hipStreamSynchronize(ctx->stream);
	ctx->last.valid = false; // (the debug exports read the stage workspace)
	// The two other streams need no call of their own.  The wave walks' stream is joined into the main stream inside the
	// tree stage (walk_large_classes), so the synchronisation above covers it.  The side stream either joins the main
	// stream before the pass ends or, in a POVU_HIP_F_ASYNC pass, carries tail_done behind its last copy: wait_tail.
	ctx->for_each_arena([](const char *, Arena &a, ArenaKind kind) {
		if (kind == ARENA_WORKSPACE)
			a.release();
	});
	ctx->ws_sub.release(); // (its arenas went above; this drops what it remembers of their contents)
	return 0;
}

extern "C" int povu_hip_arena_report(const povu_hip_ctx *ctx, povu_hip_arena_info *out, int max)
{
	if (!ctx)
		return 0;
	int n = 0;
	ctx->for_each_arena([&](const char *name, const Arena &a, ArenaKind kind) {
		if (out && n < max) {
			snprintf(out[n].name, sizeof out[n].name, "%s", name);
			out[n].resident = kind == ARENA_RESIDENT;
			out[n].bytes = a.capacity();
		}
		n++;
	});
	return n;
}

extern "C" void povu_hip_destroy(povu_hip_ctx *ctx)
{
	if (!ctx)
		return;
	(void)hipSetDevice(ctx->device);
	ctx->wait_tail();
	free_resident_graph(ctx->g);
	// every arena goes before the streams and events do (hipFree waits for the device, so nothing still reads one)
	ctx->for_each_arena([](const char *, Arena &a, ArenaKind) { a.release(); });
	for (auto &kv : ctx->attached)
		(void)munmap(kv.second.p, kv.second.bytes);
	if (ctx->stream)
		(void)hipStreamDestroy(ctx->stream);
	if (ctx->side.stream)
		(void)hipStreamDestroy(ctx->side.stream);
	if (ctx->side.fork)
		(void)hipEventDestroy(ctx->side.fork);
	if (ctx->side.join)
		(void)hipEventDestroy(ctx->side.join);
	if (ctx->side.fork2)
		(void)hipEventDestroy(ctx->side.fork2);
	if (ctx->walk_side.stream)
		(void)hipStreamDestroy(ctx->walk_side.stream);
	if (ctx->walk_side.fork)
		(void)hipEventDestroy(ctx->walk_side.fork);
	if (ctx->walk_side.join)
		(void)hipEventDestroy(ctx->walk_side.join);
	if (ctx->tail_done)
		(void)hipEventDestroy(ctx->tail_done);
	delete ctx;
}

// device block of a resident graph: the link arrays + CSR (off / adj / aoth / atwin), carved from the context's graph
// arena (which only reallocates when a graph is larger than every one before it; the previous graph is gone afterwards)
void alloc_resident_graph(Arena &arena, ResidentGraph &g, uint32_t n_vtx, uint32_t n_links, bool tips_given)
{
	static std::atomic<uint64_t> next_gen{1};
	g.V = n_vtx;
	g.E = n_links;
	g.tips_given = tips_given;
	g.gen = next_gen.fetch_add(1);
	const size_t V = n_vtx, E = n_links;
	const size_t bytes = Arena::padded(V, 4) + 2 * Arena::padded(E + 1, 4) + 2 * Arena::padded(E + 1, 1) + Arena::padded(V, 1) +
			     Arena::padded(2 * V + 2, 4) + 3 * Arena::padded(2 * E + 8, 4) + 16 * 256;
	arena.reserve(bytes);
	g.vid = arena.take<uint32_t>(V);
	g.block = g.vid;
	g.v1 = arena.take<uint32_t>(E + 1);
	g.v2 = arena.take<uint32_t>(E + 1);
	g.s1 = arena.take<uint8_t>(E + 1);
	g.s2 = arena.take<uint8_t>(E + 1);
	g.tip = arena.take<uint8_t>(V);
	g.off = arena.take<uint32_t>(2 * V + 2);
	g.adj = arena.take<uint32_t>(2 * E + 8); // (+8: kernels read a side's slots four at a time)
	g.aoth = arena.take<uint32_t>(2 * E + 8);
	g.atwin = arena.take<uint32_t>(2 * E + 8);
}

void check_graph_size(uint32_t n_vtx, uint32_t n_links)
{
	if (n_vtx == 0)
		throw HipError("graph has no vertices");
	// 32-bit index spaces: the packed list-ranking words hold 30-bit successors -- 3 events per segment and 2 adjacency
	// slots per link must stay below 2^30 (round 3: 2^29).  The reference's own limit is 2V+1 < 2^32 (core.hpp:20-21); at
	// ~54 GB of HBM per 10^8 segments the card's 288 GB run out near 5 * 10^8, just above this limit.
	if (3ull * n_vtx >= (1u << 30) || 2ull * n_links >= (1u << 30))
		throw HipError("graph too large for this build: at most 357 913 941 segments and 536 870 911 links");
}

extern "C" int povu_hip_graph_upload(povu_hip_ctx *ctx, uint32_t n_vtx, const uint32_t *vid, uint32_t n_links,
				     const uint32_t *v1, const uint8_t *s1, const uint32_t *v2, const uint8_t *s2,
				     const uint8_t *tips, char *err, size_t errlen)
{
	ResidentGraph g;
	XferScope xfer(ctx);
	try {
		if (!ctx)
			throw HipError("null context");
		ctx->wait_tail(); // (an overlapped pass may still be reading its workspace)
		// the old graph (or shard) goes first, whatever happens next: a failed upload leaves the context without a graph
		free_resident_graph(ctx->g);
		ctx->last.valid = false;
		ctx->shard_comp_ids.clear();
		ctx->shard_total_components = 0;
		check_graph_size(n_vtx, n_links);
		HIP_CHECK(hipSetDevice(ctx->device));
		alloc_resident_graph(ctx->graph_arena, g, n_vtx, n_links, tips != nullptr);
		const size_t V = n_vtx, E = n_links;
		hipStream_t s = ctx->stream;
		hipEvent_t e0, e1;
		HIP_CHECK(hipEventCreate(&e0));
		HIP_CHECK(hipEventCreate(&e1));
		HIP_CHECK(hipEventRecord(e0, s));
		HIP_CHECK(copy_async(g.vid, vid, V * 4, hipMemcpyHostToDevice, s));
		if (E) {
			HIP_CHECK(copy_async(g.v1, v1, E * 4, hipMemcpyHostToDevice, s));
			HIP_CHECK(copy_async(g.v2, v2, E * 4, hipMemcpyHostToDevice, s));
			HIP_CHECK(copy_async(g.s1, s1, E, hipMemcpyHostToDevice, s));
			HIP_CHECK(copy_async(g.s2, s2, E, hipMemcpyHostToDevice, s));
		}
		if (tips)
			HIP_CHECK(copy_async(g.tip, tips, V, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipEventRecord(e1, s));
		HIP_CHECK(hipStreamSynchronize(s));
		(void)hipEventElapsedTime(&g.h2d_ms, e0, e1);
		(void)hipEventDestroy(e0);
		(void)hipEventDestroy(e1);
		build_global_csr(g, ctx->upload_tmp, s); // validates the operands on the device
		ctx->g = g;
		return 0;
	} catch (const std::exception &e) {
		if (ctx)
			(void)hipStreamSynchronize(ctx->stream);
		set_err(err, errlen, e.what());
		return 1;
	}
}

extern "C" int povu_hip_last_upload_times(const povu_hip_ctx *ctx, double out_ms[3])
{
	if (!ctx || !out_ms || !ctx->g.block)
		return 1;
	out_ms[0] = ctx->g.h2d_ms;
	out_ms[1] = ctx->g.csr_ms;
	out_ms[2] = ctx->g.twin_ms;
	return 0;
}


// Workspace carving (or just measuring when `ar` is null), in three parts with different life times:
//   part 0  rows A/B state (CompState), sized before the component count is known (C <= V)
//   part 1  tree / result arrays every execution mode shares, sized with the real component count
//   part 2  the one-lane kernels' own lists (back edges, brackets, stacks): only reserved when the
//           sequential kernels actually run (POVU_HIP_F_SEQUENTIAL / _SEQ_TREE, or a redo)
size_t carve_workspace(Arena *ar, int part, const Sizes &z, CompState &cs, SeqWs &sw, bool hairpins)
{
	Spans take{ar};
	const size_t V = z.V, E = z.E, C = z.Cmax, T = z.T, B = z.B, nS = z.nS;
	if (part == 0) {
		take(V + 1, cs.label);
		take(std::max(V, z.slots) + 2, cs.flag);
		take(V + 2, cs.crank);
		take(V + 1, cs.comp_of, cs.tmp_a, cs.ckey, cs.perm, cs.pos);
		take(C + 2, cs.voff, cs.eoff);
		take(V + 2, cs.vdeg, cs.sbase);
		take(E + 1, cs.first);
		take(z.slots + 2, cs.erank);
		take(nS + 2, cs.ldeg, cs.loff);
		take(2 * E + 8, cs.ladj); // (+8: the class walk reads a side's list words four at a time)
		take(2 * E + 2, cs.keys, cs.vals, cs.keys2, cs.vals2);
		take(2 * E + 32, cs.hook);
		take(E + 2, cs.la, cs.lb);
		take(2 * E + 8, cs.lle); // (+8: the tour kernel reads a segment's slot words four at a time)
		take(E + 32, cs.tgray);
		take(16, cs.stats);
		take(V + 1, cs.gid_s, cs.tip_s);
		take(C + 2, cs.start_key);
		cs.scan_tmp_bytes = scan_tmp_bytes(std::max<size_t>(nS, z.slots) + 2);
		cs.sort_tmp_bytes = sort_tmp_bytes(std::max<size_t>(2 * E, V) + 2);
		take(cs.scan_tmp_bytes, cs.scan_tmp);
		take(cs.sort_tmp_bytes, cs.sort_tmp);
	} else if (part == 1) {
		// host-built per-component tables, one upload: order | owner | processed-before | processed | stack entries before
		uint32_t *tables = nullptr;
		take(5 * (C + 1), tables);
		sw.order = tables;
		sw.owner = tables + (C + 1);
		sw.tables = tables;
		take(T, sw.t_gid, sw.t_par, sw.t_cls);
		take(T + 8, sw.t_size); // (+8: the class stage reads sizes eight words at a time)
		take(T, sw.t_depth, sw.t_flags);
		take(nS + 1, sw.cur);
		take(V + 1, sw.s_vtx, sw.s_cls, sw.next_seen);
		if (hairpins)
			take(2 * (V + C + 1), sw.hairpins);
		else
			sw.hairpins = nullptr;
		take(C + 1, sw.c_ntree, sw.c_nbe0, sw.c_nbe, sw.c_nstack, sw.c_npvst, sw.c_nclass, sw.c_nbry, sw.c_status);
	} else {
		take(T, sw.t_hi, sw.first_child, sw.next_sib, sw.last_child);
		take(nS + 1, sw.ctr);
		take(T, sw.stk);
		take(V + 1, sw.selfloop);
		take(B, sw.be_src, sw.be_tgt, sw.o_next, sw.i_next, sw.b_prev, sw.b_next, sw.b_rsize, sw.b_rclass);
		take(B, sw.be_type, sw.b_in, sw.be_cdef);
		take(T, sw.o_head, sw.o_tail, sw.i_head, sw.i_tail, sw.l_head, sw.l_tail, sw.l_size, sw.bl);
		take(T, sw.nxt, sw.st_head, sw.st_tail);
		take(B + T, sw.last);
		take(V + C + 1, sw.p_parent, sw.p_a, sw.p_z, sw.p_or, sw.aux);
		take(B + T, sw.in_s);
	}
	return take.bytes + (1 << 20);
}

size_t rowb_carve_label(Arena *ar, const Sizes &z, CompState &cs)
{
	Spans take{ar};
	const size_t V = z.V, E = z.E;
	take(V + 1, cs.label);
	take(V / 4 + 16, cs.flag); // (one byte per vertex: is-root flags)
	take(V + 2, cs.crank);
	take(V + 1, cs.comp_of);
	take(2 * E + 2, cs.keys); // the cross list of the union-find tiles: [E] pairs
	take(2 * E + 32, cs.hook);
	take(16, cs.stats);
	cs.scan_tmp_bytes = scan_tmp_bytes(std::max<size_t>(z.nS, z.slots) + 2);
	take(cs.scan_tmp_bytes, cs.scan_tmp);
	if (ar) { // (what rowb_carve_reindex adds; null until then so that a use before it is a clean failure, not a stale pointer)
		cs.tmp_a = cs.ckey = cs.perm = cs.pos = cs.voff = cs.eoff = cs.vdeg = cs.sbase = cs.first = cs.erank = cs.ldeg = cs.loff =
			cs.ladj = cs.vals = cs.keys2 = cs.vals2 = cs.la = cs.lb = cs.lle = cs.gid_s = nullptr;
		cs.tgray = cs.tip_s = nullptr;
		cs.start_key = nullptr;
		cs.sort_tmp = nullptr;
		cs.sort_tmp_bytes = 0;
	}
	return take.bytes + (1 << 16);
}

// what the re-index arena must hold already for the adjacency kernel to be started ahead of the component count
size_t rowb_speculative_adj_bytes(const Sizes &z) { return 2 * (Arena::padded(2 * z.E + 8, 4) + 256) + 4096; }

size_t rowb_carve_reindex(Arena *ar, const Sizes &z, size_t C, const RowBNeeds &need, CompState &cs)
{
	Spans take{ar};
	const size_t V = z.V, E = z.E, nS = z.nS;
	const bool lean = need.identity && need.sort_free; // sorted space = global vertex space, nothing is renumbered
	// (ladj and lle FIRST: their place in the arena does not depend on the component count -- povu_hip_decompose starts the
	// kernel that fills them before the count has reached the host, rowb_speculative_adj_bytes)
	take(2 * E + 8, cs.ladj); // (+8: the class walk reads a side's list words four at a time)
	take(2 * E + 8, cs.lle);  // (+8: the tour kernel reads a segment's slot words four at a time)
	take(C + 2, cs.voff, cs.eoff, cs.start_key);
	if (!lean) { // the vertices are renumbered (or the sorting builder wants the tables anyway)
		take(V + 1, cs.tmp_a, cs.ckey, cs.perm, cs.pos);
		take(V + 2, cs.vdeg, cs.sbase);
		take(V + 1, cs.gid_s, cs.tip_s);
	}
	if (!(lean && !need.self_loops)) // local degrees and offsets of the sides (else the CSR's own)
		take(nS + 2, cs.ldeg, cs.loff);
	if (!need.sort_free) { // the builder that numbers the local edges densely (hub vertices; povu_hip_componetize takes the full set)
		take(std::max(V, z.slots) + 2, cs.flag);
		take(E + 1, cs.first);
		take(z.slots + 2, cs.erank);
		take(2 * E + 2, cs.vals, cs.keys2, cs.vals2);
		take(E + 2, cs.la, cs.lb);
		take(E + 32, cs.tgray);
	}
	if (!need.identity || !need.sort_free) {
		cs.sort_tmp_bytes = sort_tmp_bytes(std::max<size_t>(2 * E, V) + 2);
		take(cs.sort_tmp_bytes, cs.sort_tmp);
	}
	return take.bytes + (1 << 16);
}

namespace
{
struct ComponentsOwner {
	povu_hip_components view{};
	std::vector<uint32_t> voff, eoff, vid, v1, v2;
	std::vector<uint8_t> tip, s1, s2;
};
} // namespace

extern "C" povu_hip_components *povu_hip_componetize(povu_hip_ctx *ctx, char *err, size_t errlen)
{
	try {
		if (!ctx || !ctx->g.block)
			throw HipError("no graph resident: call povu_hip_graph_upload first");
		HIP_CHECK(hipSetDevice(ctx->device));
		ctx->wait_tail();
		const ResidentGraph &g = ctx->g;
		hipStream_t s = ctx->stream;
		const Sizes z{g.V, g.E, g.V, 0, 0, 2 * (size_t)g.V, g.n_slots};
		CompState &cs = ctx->cs;
		SeqWs &sw = ctx->sw;
		ctx->last.valid = false;
		ctx->host.reset();
		cs.host = &ctx->host;
		cs.host_pub = nullptr;
		ctx->ws.reserve(carve_workspace(nullptr, 0, z, cs, sw, false));
		carve_workspace(&ctx->ws, 0, z, cs, sw, false);
		StageTimer &tm = ctx->timer;
		tm.reset();
		tm.enabled = true;
		const uint32_t C = label_components(g, cs, tm, s);
		reindex_components(g, cs, C, tm, s, true); // (the builder that numbers the local edges: la / lb in local edge order)
		if (!cs.dense_edges)
			throw HipError("componetize: local edges were not numbered (internal)");
		auto o = std::make_unique<ComponentsOwner>();
		const size_t V = g.V, E = g.E;
		o->voff.resize(C + 1);
		o->eoff.resize(C + 1);
		o->vid.resize(V);
		o->tip.resize(V);
		std::vector<uint32_t> la(E), lb(E);
		HIP_CHECK(copy_async(o->voff.data(), cs.voff, (size_t)(C + 1) * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(o->eoff.data(), cs.eoff, (size_t)(C + 1) * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(o->vid.data(), cs.gid_s, V * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(o->tip.data(), cs.tip_s, V, hipMemcpyDeviceToHost, s));
		if (E) {
			HIP_CHECK(copy_async(la.data(), cs.la, E * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(copy_async(lb.data(), cs.lb, E * 4, hipMemcpyDeviceToHost, s));
		}
		HIP_CHECK(hipStreamSynchronize(s));
		o->v1.resize(E);
		o->v2.resize(E);
		o->s1.resize(E);
		o->s2.resize(E);
		for (uint32_t c = 0; c < C; c++)
			for (uint32_t e = o->eoff[c]; e < o->eoff[c + 1]; e++) { // sorted side id = 2 * position + end
				o->v1[e] = (la[e] >> 1) - o->voff[c];
				o->s1[e] = (uint8_t)(la[e] & 1);
				o->v2[e] = (lb[e] >> 1) - o->voff[c];
				o->s2[e] = (uint8_t)(lb[e] & 1);
			}
		o->view = povu_hip_components{C, g.V, g.E, o->voff.data(), o->eoff.data(), o->vid.data(), o->tip.data(),
					      o->v1.data(), o->v2.data(), o->s1.data(), o->s2.data()};
		ComponentsOwner *raw = o.release();
		return &raw->view; // view is the first member: the owner is recovered from it in _free
	} catch (const std::exception &e) {
		set_err(err, errlen, e.what());
		return nullptr;
	}
}

extern "C" void povu_hip_components_free(povu_hip_components *c)
{
	delete reinterpret_cast<ComponentsOwner *>(c);
}

// What the stage workspace of a pass has to hold (par_kernels.hpp: StageWsOpts).  The plain all-parallel pass needs neither
// the per-vertex tables of a sequential tree stage, nor the keys of its bracket sort, nor the hairpin report's arrays, and
// takes the wave walk's arrays only when it meets large classes.  Brackets: every link outside the spanning forest of
// the segments starts at most one back edge (E - (V - C) of them), every side without links at most one to the root
// (spanning_tree.cpp:433-438), and the class stage adds at most one capping or simplifying edge per tree vertex.
static StageWsOpts stage_opts(size_t V, size_t E, size_t C, size_t empty_sides, bool seq_tree, bool hairpins)
{
	StageWsOpts o;
	const size_t T = 2 * V + C;
	o.nb_cap = std::min(E + V + T, (E + C > V ? E + C - V : 0) + empty_sides + T + 64);
	o.full_t = seq_tree || hairpins;
	o.sorted_brackets = seq_tree;
	o.hairpins = hairpins;
	o.walk_inline = false;
	return o;
}

extern "C" uint64_t povu_hip_workspace_estimate(uint32_t n_vtx, uint32_t n_links, uint32_t n_components)
{
	try {
		Sizes z{n_vtx, n_links, n_vtx, 0, 0, 2 * (size_t)n_vtx, 2 * (size_t)n_links};
		CompState cs{};
		SeqWs sw{};
		// (rows A/B of a graph whose vertices come grouped by component, without hub vertices or self loops: the pangenome
		// case; povu_hip_workspace_breakdown's out[6] has the general case)
		const RowBNeeds lean{true, true, false};
		uint64_t total = rowb_carve_label(nullptr, z, cs) + rowb_carve_reindex(nullptr, z, n_components ? n_components : n_vtx, lean, cs);
		z.set_components(n_components ? n_components : n_vtx);
		// (sides without links: two per component and a few more -- an estimate; a graph full of tips reserves more)
		total += carve_workspace(nullptr, 1, z, cs, sw, false) +
			 stage_workspace_bytes(z.V, z.E, z.Cmax, stage_opts(z.V, z.E, z.Cmax, 2 * z.Cmax + z.V / 64, false, false));
		return total;
	} catch (...) {
		return 0;
	}
}

extern "C" int povu_hip_workspace_breakdown(uint32_t n_vtx, uint32_t n_links, uint32_t n_components, uint64_t out[7])
{
	try {
		Sizes z{n_vtx, n_links, n_vtx, 0, 0, 2 * (size_t)n_vtx, 2 * (size_t)n_links};
		CompState cs{};
		SeqWs sw{};
		const RowBNeeds lean{true, true, false}, general{false, false, true};
		const size_t Cn = n_components ? n_components : n_vtx;
		out[0] = rowb_carve_label(nullptr, z, cs) + rowb_carve_reindex(nullptr, z, Cn, lean, cs);
		out[6] = rowb_carve_label(nullptr, z, cs) + rowb_carve_reindex(nullptr, z, Cn, general, cs);
		z.set_components(Cn);
		out[1] = carve_workspace(nullptr, 1, z, cs, sw, false);
		const StageWsOpts so = stage_opts(z.V, z.E, z.Cmax, 2 * z.Cmax + z.V / 64, false, false);
		out[2] = par_workspace_bytes(z.V, z.E, z.Cmax, 1, so);
		out[3] = par_workspace_bytes(z.V, z.E, z.Cmax, 2, so);
		out[4] = tree_workspace_bytes(z.V, z.E, z.Cmax, 1, so);
		out[5] = tree_workspace_bytes(z.V, z.E, z.Cmax, 2, so);
		return 0;
	} catch (...) {
		return 1;
	}
}

// Reserve, ahead of time, the device arenas a graph of this size will need (the resident graph, the CSR build's scratch and
// the decompose workspace for a graph of few components): the first upload + decompose on a fresh context otherwise
// pay for ~1 KB of device memory per segment being mapped (0.3 s and more for a whole-genome graph).  The CLI calls this on
// the thread that brought HIP up, as soon as the tokenizer knows the counts and while the rest of the parse runs.
// Best effort: when that does not fit, the arenas are left alone and the real calls allocate exactly.
extern "C" int povu_hip_prewarm(povu_hip_ctx *ctx, uint32_t n_vtx, uint32_t n_links, char *err, size_t errlen)
{
	try {
		if (!ctx)
			throw HipError("null context");
		ctx->wait_tail();
		if (ctx->g.block || ctx->last.valid)
			return 0; // (only for a context that holds nothing yet: a reserve invalidates what an arena holds)
		check_graph_size(n_vtx, n_links);
		HIP_CHECK(hipSetDevice(ctx->device));
		const size_t V = n_vtx, E = n_links, nS = 2 * V;
		size_t free_b = 0, total_b = 0;
		HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
		const size_t graph_b = Arena::padded(V, 4) + 2 * Arena::padded(E + 1, 4) + 2 * Arena::padded(E + 1, 1) + Arena::padded(V, 1) +
				       Arena::padded(2 * V + 2, 4) + 3 * Arena::padded(2 * E + 8, 4) + 16 * 256;
		const size_t tmp_b = Arena::padded(2 * E + 2, 4) * 4 + Arena::padded(nS + 2, 4) + sort_tmp_bytes(2 * E) +
				     scan_tmp_bytes(std::max<size_t>(nS, E) + 2) + (1 << 16);
		Sizes z;
		// (components: a guess -- a pangenome graph has few, and a larger count only means that the decompose call grows
		// its arena after all; reserving for V components took three times as long as the exact size)
		z.V = V, z.E = E, z.nS = nS, z.slots = 2 * E, z.Cmax = V, z.T = z.B = 0; // (rows A/B are sized before the count is known)
		CompState cs{};
		SeqWs sw{};
		z.Cmax = std::min<size_t>(V, std::max<size_t>(1024, V / 64));
		const size_t ws_b = rowb_carve_label(nullptr, z, cs), ws_b2 = rowb_carve_reindex(nullptr, z, z.Cmax, RowBNeeds{true, true, false}, cs);
		z.set_components(z.Cmax);
		const size_t ws2_b = carve_workspace(nullptr, 1, z, cs, sw, false) +
				     stage_workspace_bytes(V, E, z.Cmax, stage_opts(V, E, z.Cmax, 2 * z.Cmax + V / 64, false, false));
		const size_t need = graph_b + tmp_b + ws_b + ws_b2 + ws2_b;
		if (need + need / 8 + (size_t(64) << 20) > free_b)
			return 0; // the worst case does not fit beside what is there: let the real calls size things
		// (exact sizes: a context that is warmed for one graph is usually there for that graph only)
		ctx->graph_arena.reserve(graph_b, false);
		ctx->upload_tmp.reserve(tmp_b, false);
		ctx->ws.reserve(ws_b, false);
		ctx->ws_b.reserve(ws_b2, false);
		ctx->ws2.reserve(ws2_b, false);
		return 0;
	} catch (const std::exception &e) {
		set_err(err, errlen, e.what());
		return 1;
	}
}

extern "C" uint64_t povu_hip_leaf_workspace_estimate(uint32_t n_vtx, uint32_t n_components)
{
	// the PVST of a component has at most one vertex per segment and a root
	return leaf_workspace_bytes(n_vtx, n_components ? n_components : n_vtx, (size_t)n_vtx + (n_components ? n_components : n_vtx));
}

// ---- povu_hip_decompose: the plan of a pass, then its steps
namespace
{

static const char *const SUB_REDO_REFUSAL = "subflubble passes: a component went (or was sent) through the sequential redo of add_flubbles, "
					    "whose PVST layout the inserting passes do not read";

} // namespace

// Every decision a pass takes from its options, in one place.  Refusals that depend on the flags alone are made here;
// those that depend on what the pass finds (a component the laminarity check flags) where it finds it.
PassPlan plan_pass(const povu_hip_opts *opts)
{
	povu_hip_opts o{0, 1, 0};
	if (opts)
		o = *opts;
	if (o.world == 0)
		o.world = 1;
	if (o.rank >= o.world)
		throw HipError("shard rank >= world");
	auto has = [&](uint32_t flag) { return (o.flags & flag) != 0; };
	PassPlan p;
	p.rank = o.rank, p.world = o.world, p.hairpins = has(POVU_HIP_F_HAIRPINS), p.timed = !has(POVU_HIP_F_NO_STAGE_TIMES);
	p.all_seq = has(POVU_HIP_F_SEQUENTIAL), p.seq_tree = has(POVU_HIP_F_SEQ_TREE), p.par_tree = !p.all_seq && !p.seq_tree;
	p.all_sub = has(POVU_HIP_F_SUBFLUBBLES), p.leaf_sub = p.all_sub || has(POVU_HIP_F_LEAF_SUBFLUBBLES);
	p.force_redo = has(POVU_HIP_F_FORCE_REDO), p.redo_odd = has(POVU_HIP_F_REDO_ODD), p.sorted_adj = has(POVU_HIP_F_SORTED_ADJ);
	p.big_class_dfs = has(POVU_HIP_F_BIG_CLASS_DFS), p.sparse_splitters = has(POVU_HIP_F_SPARSE_SPLITTERS);
	p.all_vertex_classes = has(POVU_HIP_F_ALL_VERTEX_CLASSES), p.check_laminar = has(POVU_HIP_F_CHECK_LAMINAR);
	// POVU_HIP_F_ASYNC: the pass may leave its last kernels and the copies of the PVST arrays in flight when it returns
	// (and the next pass may then start under them).  Only the plain all-parallel pass has that form.
	p.overlap_tail = has(POVU_HIP_F_ASYNC) && !p.timed && p.par_tree && !p.hairpins && !p.force_redo && !p.redo_odd && !p.leaf_sub &&
			 !p.check_laminar;
	// heaviest first: the shard assignment and the launch order of the one-lane kernels (the parallel stages do not care,
	// so a single-shard parallel pass skips the sort)
	p.heaviest_first = p.world > 1 || p.all_seq || p.seq_tree || p.force_redo;
	if (p.leaf_sub && (p.all_seq || p.seq_tree))
		throw HipError("the leaf subflubble passes read the state of the parallel stages: not with the sequential tree / all-sequential test modes");
	if (p.all_sub && (p.force_redo || p.redo_odd) && !p.hairpins) // (with --hairpins a flagged component is refused first, leaf_passes)
		throw HipError(SUB_REDO_REFUSAL);
	return p;
}

namespace
{
// The tail of the pass before (POVU_HIP_F_ASYNC) reads the stage workspace (ws2) from the side stream.  A pass that may
// itself overlap waits for it ON THE STREAM, right before its own first write there (carve_stages, component_tables);
// every other pass -- and any pass whose arenas must grow, which frees them -- waits on the host.
static void reserve(povu_hip_ctx *ctx, Arena &ar, size_t bytes)
{
	if (bytes > ar.capacity())
		ctx->wait_tail();
	ar.reserve(bytes);
}

} // namespace

// ---- what a pass sets up ahead of row B: the state of the pass before is forgotten, the pinned scratch rewound, the
// labelling's arrays carved (sized before the component count is known) and the stage timer armed
Sizes rowb_begin(povu_hip_ctx *ctx, const PassPlan &p)
{
	const ResidentGraph &g = ctx->g;
	const Sizes z{g.V, g.E, g.V, 0, 0, 2 * (size_t)g.V, g.n_slots}; // (rows A/B run before the component count is known)
	ctx->last = LastPass{};
	ctx->host.reset();
	ctx->cs.host = ctx->pw.host = ctx->tw.host = &ctx->host;
	reserve(ctx, ctx->ws, rowb_carve_label(nullptr, z, ctx->cs));
	rowb_carve_label(&ctx->ws, z, ctx->cs);
	ctx->timer.reset();
	ctx->timer.enabled = p.timed;
	return z;
}

// ---- row B: labelling, speculative adjacency, re-index
// The host has to know the component count (it sizes the workspaces) and then the components' sizes (the tables of the
// stages): two reads.  Neither is waited for with the stream idle: the words are published by a kernel, an event is
// recorded behind it (HostScratch::mark), and the stream is given its next kernel before the host waits for the event --
//  (1) behind the labelling: the re-index's adjacency kernel, on the assumption that holds for nearly every GFA (vertices
//      grouped by component, no hub, no self loop: it then needs nothing the labels say but the hooks; when the
//      assumption fails its output is simply overwritten by the real re-index);
//  (2) behind the re-index: the tree stage's first kernel (it reads the re-indexed adjacency only; carve_stages).
// Not with stage timers (the kernels would be booked on the wrong stage).
RowB row_b(povu_hip_ctx *ctx, const PassPlan &p, const Sizes &z, StageTimer &tm)
{
	const ResidentGraph &g = ctx->g;
	CompState &cs = ctx->cs;
	hipStream_t s = ctx->stream;
	uint32_t *lab = label_components_enqueue(g, cs, tm, s);
	const HostScratch::Token labelled = ctx->host.mark(s);
	bool spec_adj = false;
	if (!tm.enabled && g.E && sort_free_adjacency(g, p.sorted_adj) && ctx->ws_b.capacity() >= rowb_speculative_adj_bytes(z)) {
		ctx->ws_b.reserve(0); // (rewinds the arena: the two arrays get the places rowb_carve_reindex will give them)
		uint32_t *ladj = ctx->ws_b.take<uint32_t>(2 * z.E + 8), *lle = ctx->ws_b.take<uint32_t>(2 * z.E + 8);
		reindex_speculative_adj(g, cs, ladj, lle, s);
		spec_adj = true;
	}
	ctx->host.wait(labelled);
	const uint32_t C = label_components_finish(cs, lab);
	// what the re-index of THIS graph needs, now that the count, the order and the self loops are known
	const RowBNeeds need{C == 1 || cs.comp_sorted, sort_free_adjacency(g, p.sorted_adj), cs.has_self_loops};
	const size_t need_b = rowb_carve_reindex(nullptr, z, C, need, cs);
	if (spec_adj && need_b > ctx->ws_b.capacity()) { // the arena has to grow under a kernel that writes into it: let it finish, forget it
		HIP_CHECK(hipStreamSynchronize(s));
		spec_adj = false;
	}
	reserve(ctx, ctx->ws_b, need_b);
	rowb_carve_reindex(&ctx->ws_b, z, C, need, cs);
	spec_adj = spec_adj && need.identity && need.sort_free && !need.self_loops; // (else: a kernel that wrote nonsense into arrays about to be rewritten)
	// component sizes on the host (shard assignment, launch order): the last re-index kernel writes them into pinned
	// memory itself
	uint32_t *pub = ctx->host.take<uint32_t>(2 * ((size_t)C + 1) + 4);
	HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void **>(&cs.host_pub), pub, 0));
	count_kernel_d2h((2 * ((size_t)C + 1) + 4) * 4);
	reindex_components(g, cs, C, tm, s, p.sorted_adj, spec_adj);
	return RowB{C, pub, pub + (size_t)C + 1, pub + 2 * ((size_t)C + 1), ctx->host.mark(s)};
}

namespace
{
// ---- stage workspaces, sized with the real component count (z), and the tree stage's first kernel, which goes out
// before the host waits for the component sizes.  Returns whether the stream already waits for the tail of the pass before.
static bool carve_stages(povu_hip_ctx *ctx, const PassPlan &p, const Sizes &z, uint32_t C, const StageTimer &tm)
{
	const StageWsOpts so = stage_opts(z.V, z.E, C, ctx->g.n_empty_sides, p.seq_tree, p.hairpins);
	reserve(ctx, ctx->ws2, carve_workspace(nullptr, 1, z, ctx->cs, ctx->sw, p.hairpins) + (p.all_seq ? 0 : stage_workspace_bytes(z.V, z.E, C, so)));
	carve_workspace(&ctx->ws2, 1, z, ctx->cs, ctx->sw, p.hairpins);
	if (p.all_seq)
		return false;
	TreeWs &tw = ctx->tw;
	stage_workspace_carve(ctx->ws2, ctx->pw, tw, z.V, z.E, C, so);
	tw.walk_arena = &ctx->ws_walk;
	tw.walk_stream = ctx->walk_side.stream;
	tw.walk_fork = ctx->walk_side.fork;
	tw.walk_join = ctx->walk_side.join;
	tw.tour_words_done = false;
	if (!p.par_tree || tm.enabled)
		return false;
	if (ctx->tail_pending) // first write into the stage workspace: behind the tail of the pass before
		HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->tail_done, 0));
	tree_tour_words(ctx->cs, (uint32_t)z.V, (uint32_t)z.E, tw, ctx->stream);
	return ctx->tail_pending;
}

// What the component tables tell the stages.
struct CompTables {
	uint32_t n_stack = 0, n_processed = 0;
};

// ---- component tables: launch order, owner (LPT over vertices + links, the same on every rank), processed components
// (>= 3 vertices, owned by this shard) and their running count `pc` = where a component starts in the dense PVST output,
// and where each component's candidate stack starts.  Host-built in pinned scratch: the upload needs no synchronisation.
static CompTables component_tables(povu_hip_ctx *ctx, const PassPlan &p, uint32_t C, const uint32_t *voff, const uint32_t *eoff,
				   bool tail_waited)
{
	uint32_t *tab_h = ctx->host.take<uint32_t>(5 * ((size_t)C + 1));
	uint32_t *order = tab_h, *owner = tab_h + ((size_t)C + 1), *pc = tab_h + 2 * ((size_t)C + 1), *cproc = tab_h + 3 * ((size_t)C + 1),
		 *stack_off = tab_h + 4 * ((size_t)C + 1);
	if (p.heaviest_first) {
		std::vector<uint64_t> weight(C);
		for (uint32_t c = 0; c < C; c++)
			weight[c] = (uint64_t)(eoff[c + 1] - eoff[c]) + (voff[c + 1] - voff[c]);
		lpt_assign(weight.data(), C, p.world, order, owner);
	} else {
		std::iota(order, order + C, 0u);
		std::fill(owner, owner + C, 0u);
	}
	uint64_t links = 0;
	for (uint32_t c = 0; c < C; c++)
		if (owner[c] == p.rank || p.world == 1)
			links += eoff[c + 1] - eoff[c];
	ctx->last_links = links;
	CompTables t;
	order[C] = owner[C] = cproc[C] = 0;
	pc[0] = 0;
	for (uint32_t c = 0; c < C; c++) {
		const uint32_t nv = voff[c + 1] - voff[c];
		cproc[c] = (nv >= 3 && (p.world == 1 || owner[c] == p.rank)) ? 1u : 0u;
		pc[c + 1] = pc[c] + cproc[c];
		stack_off[c] = t.n_stack;
		t.n_stack += cproc[c] ? nv : 0u; // one candidate-stack entry per segment (its black tree edge)
	}
	stack_off[C] = t.n_stack;
	t.n_processed = pc[C];
	if (ctx->tail_pending && !tail_waited) // first write into the stage workspace: behind the tail of the pass before
		HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->tail_done, 0));
	HIP_CHECK(copy_async(ctx->sw.tables, tab_h, 5 * ((size_t)C + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
	return t;
}

// The one-lane kernels' lists live in their own arena, carved -- and emptied, as the kernels expect them -- only when a
// pass runs those kernels.
struct SeqLanes {
	povu_hip_ctx *ctx;
	const Sizes &z;
	bool hairpins;
	bool carved = false;
	void carve()
	{
		if (carved)
			return;
		ctx->wait_tail();
		ctx->ws_seq.reserve(carve_workspace(nullptr, 2, z, ctx->cs, ctx->sw, hairpins));
		carve_workspace(&ctx->ws_seq, 2, z, ctx->cs, ctx->sw, hairpins);
		carved = true;
	}
	void init(hipStream_t s)
	{
		carve();
		const SeqWs &sw = ctx->sw;
		for (uint32_t *p : {sw.first_child, sw.o_head, sw.i_head, sw.bl, sw.t_hi, sw.t_cls, sw.st_head, sw.st_tail})
			HIP_CHECK(hipMemsetAsync(p, 0xFF, z.T * 4, s));
		HIP_CHECK(hipMemsetAsync(sw.ctr, 0xFF, z.nS * 4, s));
		HIP_CHECK(hipMemsetAsync(sw.cur, 0, z.nS * 4, s));
		HIP_CHECK(hipMemsetAsync(sw.selfloop, 0, z.V, s));
		HIP_CHECK(hipMemsetAsync(sw.last, 0xFF, (z.B + z.T) * 4, s));
		HIP_CHECK(hipMemsetAsync(sw.in_s, 0, z.B + z.T, s));
	}
};

// What rows C-G leave for the result fetch and the record of the pass.
struct RowsOut {
	const uint32_t *sum = nullptr; // outcome of the pass in pinned memory (pass_summary); null: read it when the pass is done
	uint32_t nbad = 0;	       // components through the sequential redo
	bool mixed = false;	       // parallel result for most components, sequential redo for the flagged ones
	bool redo_pvst_only = false, stack_export_pending = false;
	bool fast_tail = false; // the summary came with the PVST count: nothing was synchronised after the tail was enqueued
	PassTail tail;
};

// pass_summary's words, read with the stream drained; f's ev1 goes behind them (recorded again if more work follows)
static const uint32_t *read_summary(povu_hip_ctx *ctx, uint32_t C, bool with_par, const povu_hip_forest &f)
{
	uint32_t *h = ctx->host.take<uint32_t>(PassSummary::words(C));
	count_kernel_d2h(PassSummary::words(C) * 4);
	pass_summary(ctx->sw, with_par ? &ctx->pw : nullptr, C, h, ctx->stream);
	HIP_CHECK(hipEventRecord(f.ev1, ctx->stream));
	HIP_CHECK(hipStreamSynchronize(ctx->stream));
	return h;
}

// ---- rows C-G on the parallel kernels (the tree on the one-lane kernels with POVU_HIP_F_SEQ_TREE), up to the count of
// the components the laminarity check flags; returns the bracket count given to the class stage (< 0: sequential tree)
static int64_t parallel_rows(povu_hip_ctx *ctx, const PassPlan &p, uint32_t C, const uint32_t *gstats, const CompTables &t,
			     povu_hip_forest &f, SeqLanes &lanes, StageTimer &tm, RowsOut &out)
{
	SeqWs &sw = ctx->sw;
	ParWs &pw = ctx->pw;
	hipStream_t s = ctx->stream;
	int64_t dense_nb0 = -1;
	pw.cproc_ps = sw.tables + 2 * ((size_t)C + 1);
	ctx->tw.cproc = sw.tables + 3 * ((size_t)C + 1);
	pw.soff = sw.tables + 4 * ((size_t)C + 1);
	pw.narrow_ordcnt = pw.narrow_srccnt = pw.narrow_incnt = false;
	// Bracket counts per tree vertex as bytes (ParWs::ordcnt8 / srccnt8 / incnt8) when none can reach 256: a vertex sends at most
	// one back edge per link of its side (one, to the root, from a side without links), and a position of the bracket list
	// holds at most a capping and a simplifying bracket more.  Otherwise -- a hub, a fat side of the dense re-index path -- the
	// word kernels run.  The brackets that END at a vertex away from the roots are bounded by the same gate but for the
	// capping brackets that share a target: the class stage says when a byte of incnt8 would have overflowed, and the tree
	// and class stages then run again with all three counts as words (wide_again).
	// POVU_HIP_WIDE_COUNTS (A/B hook, read per pass): 1 = words for all three, 2 = words for srccnt and incnt, 3 = for incnt only.
	auto tree_stage = [&](bool wide_again) {
		const char *ev = getenv("POVU_HIP_WIDE_COUNTS");
		const int wide = wide_again ? 1 : ev ? atoi(ev) : 0;
		const bool fits = std::max<uint32_t>(gstats[0], 1u) + 2u <= 255u;
		pw.narrow_ordcnt = fits && wide != 1;
		pw.narrow_srccnt = pw.narrow_ordcnt && wide != 2;
		pw.narrow_incnt = pw.narrow_srccnt && wide != 3;
		dense_nb0 = run_parallel_tree(ctx->cs, sw, pw, ctx->tw, C, gstats[0], p.big_class_dfs, p.sparse_splitters, tm, s);
	};
	if (p.seq_tree) {
		lanes.init(s);
		tm.begin("tree_seq");
		sw.stages = SEQ_STAGE_TREE;
		launch_seq_components(sw, s);
		tm.end(1);
	} else {
		tree_stage(false);
	}
	pw.all_vertex_classes = p.all_vertex_classes;
	pw.check_laminar = p.check_laminar;
	out.tail.want_overlap = p.overlap_tail;
	out.tail.done = f.ev1;
	out.tail.done2 = ctx->tail_done;
	// the result block is allocated as soon as the number of PVST vertices is known (before the emit kernel): the parallel
	// stages write it straight into pinned host memory, there is no device-to-host copy
	auto alloc_result_block = [&f](size_t total) -> void * {
		f.release_blocks();
		void *dev = nullptr;
		HIP_CHECK(hipHostGetDevicePointer(&dev, f.alloc(total).p, 0));
		return dev;
	};
	if (!run_parallel_dg(ctx->cs, sw, pw, C, t.n_processed, t.n_stack, dense_nb0, alloc_result_block, tm, s, ctx->side, out.tail)) {
		// a byte of incnt8 overflowed (only a pass with narrow_incnt says so): counters cleared, both stages again with words
		ctx->wide_repeats++;
		zero_component_counters(sw, C, pw.comp_bad, pw.err, s);
		tree_stage(true);
		if (!run_parallel_dg(ctx->cs, sw, pw, C, t.n_processed, t.n_stack, dense_nb0, alloc_result_block, tm, s, ctx->side, out.tail))
			throw HipError("class stage: the word form of the bracket counts reported an overflow (internal)");
	}
	out.stack_export_pending = true;
	if (p.redo_odd) // (tests: flag every other component as if its stack were not laminar)
		mark_odd_u32(pw.comp_bad, C, s);
	// Everything the host needs came back with the PVST count, unless something after it can still flag a component (the
	// laminarity check, the test modes) or add to the result (labels, boundaries): then the summary is read again when all
	// of that is done.
	out.fast_tail = out.tail.summary_final && !p.leaf_sub && !p.hairpins && !p.force_redo && !p.redo_odd;
	out.sum = out.fast_tail ? out.tail.early_summary : read_summary(ctx, C, true, f);
	const PassSummary sum(C, out.sum);
	if (sum.err(PassSummary::NO_BRACKET))
		throw HipError("parallel class stage: a tree vertex has no live bracket (internal invariant broken)");
	if (sum.err(PassSummary::WALK_POOL))
		throw HipError("class walk: stack pool exhausted (internal sizing bug)");
	if (sum.err(PassSummary::FOREST_SIZE))
		throw HipError("spanning forest of the links has the wrong size (internal)");
	for (uint32_t c = 0; c < C; c++)
		out.nbad += sum.bad(c) ? 1 : 0;
	return dense_nb0;
}

// ---- the leaf subflubble passes -- find_tiny + find_parallel relabel leaf flubbles (leaf_kernels.hip): the PVSTs the
// parallel stages just emitted here, those of components that go through the redo of add_flubbles after it (redo) --
// and with -s the inserting passes
static void leaf_passes(povu_hip_ctx *ctx, const PassPlan &p, uint32_t C, uint32_t nbad, povu_hip_forest &f, LeafState &leaf_state,
			StageTimer &tm)
{
	hipStream_t s = ctx->stream;
	if (nbad && p.hairpins)
		throw HipError("leaf subflubble passes: with --hairpins a component that needs the sequential redo is rebuilt "
			       "from scratch by the one-lane kernels, whose tree state the passes do not read");
	tm.begin("leaf_subflubbles");
	leaf_prepare(ctx->cs, ctx->sw, ctx->pw, ctx->tw, C, ctx->ws_leaf, leaf_state, s);
	leaf_dense(leaf_state, ctx->sw, ctx->pw, C, s);
	const size_t n = ctx->pw.d_total;
	povu_hip_forest::Block &b = f.blocks.empty() ? f.alloc(n) : f.blocks[0]; // (the parallel stages' own)
	f.labels = n != 0;
	b.sub_ai.resize(n, ctx->pool); // (page-locked, out of the context's pool)
	b.sub_zi.resize(n, ctx->pool);
	b.sub_fam.resize(n, ctx->pool);
	if (n) {
		HIP_CHECK(copy_async(b.sub_ai.data(), leaf_state.dense.ai, n * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(b.sub_zi.data(), leaf_state.dense.zi, n * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(b.sub_fam.data(), leaf_state.dense.fam, n, hipMemcpyDeviceToHost, s));
	}
	tm.end(16);
	HIP_CHECK(hipStreamSynchronize(s));
	if (!p.all_sub)
		return;
	// find_concealed, find_midi, find_smothered insert vertices (sub_kernels.hip); they read the dense PVST the parallel
	// stages wrote, so a component that needs the sequential redo has no place here
	if (nbad || p.force_redo || p.redo_odd)
		throw HipError(SUB_REDO_REFUSAL);
	tm.begin("subflubbles_insert");
	b.subx = std::make_shared<SubForest>();
	run_subflubbles(ctx->cs, ctx->sw, ctx->pw, ctx->tw, leaf_state, C, ctx->host, *b.subx, ctx->pool, s, ctx->ws_sub);
	tm.end(40);
}

// ---- the redo decision: components whose candidate stack is not laminar go through the exact sequential kernels (every
// component with POVU_HIP_F_FORCE_REDO, or for the hairpin report, which the parallel path only has for a whole pass)
static void redo(povu_hip_ctx *ctx, const PassPlan &p, uint32_t C, int64_t dense_nb0, SeqLanes &lanes, const LeafState &leaf_state,
		 StageTimer &tm, RowsOut &out)
{
	SeqWs &sw = ctx->sw;
	hipStream_t s = ctx->stream;
	if (p.force_redo || (out.nbad && p.hairpins)) {
		fill_u32(ctx->pw.comp_bad, C, 1u, s);
		out.nbad = C;
	} else if (out.nbad) {
		out.mixed = true; // (the others keep the dense result the parallel stages wrote)
	}
	if (!out.nbad)
		return;
	tm.begin("redo_seq");
	if (dense_nb0 >= 0 && !p.hairpins) {
		// Only add_flubbles' stack machine (flubbles.cpp:316-365) cannot be evaluated in closed form on such a stack; tree,
		// classes, candidate stack and next_seen of the parallel stages stand.  They are copied into the per-component
		// layout, one lane per flagged component runs the machine.
		lanes.carve();
		export_parallel_stack(ctx->cs, sw, ctx->pw, s);
		out.stack_export_pending = false;
		HIP_CHECK(hipMemsetAsync(sw.in_s, 0, lanes.z.B + lanes.z.T, s));
		sw.stages = SEQ_STAGE_PVST | SEQ_STAGE_GIVEN_STACK;
		out.redo_pvst_only = true;
	} else {
		if (p.leaf_sub)
			throw HipError("leaf subflubble passes: this pass rebuilds the flagged components from scratch with the "
				       "one-lane kernels, whose tree state the passes do not read");
		if (dense_nb0 >= 0) // parallel tree: the one-lane kernels start from scratch
			lanes.init(s);
		sw.stages = dense_nb0 >= 0 ? SEQ_STAGE_ALL : (SEQ_STAGE_CLASSES | SEQ_STAGE_STACK | SEQ_STAGE_PVST);
	}
	sw.comp_sel = ctx->pw.comp_bad;
	if (p.leaf_sub) { // (only reached with the PVST-only redo, see above)
		sw.p_ai = leaf_state.p_ai;
		sw.p_zi = leaf_state.p_zi;
	}
	launch_seq_components(sw, s);
	sw.comp_sel = nullptr;
	if (p.leaf_sub)
		leaf_seq(leaf_state, ctx->cs, sw, ctx->pw.comp_bad, C, s);
	tm.end(1);
	out.sum = nullptr;
}

// ---- rows C-G, on the one-lane kernels (POVU_HIP_F_SEQUENTIAL) or the parallel ones with their leaf passes, hairpin
// report and redo
static RowsOut rows_c_to_g(povu_hip_ctx *ctx, const PassPlan &p, uint32_t C, const uint32_t *gstats, const CompTables &t,
			   povu_hip_forest &f, SeqLanes &lanes, LeafState &leaf_state, StageTimer &tm)
{
	const CompState &cs = ctx->cs;
	SeqWs &sw = ctx->sw;
	hipStream_t s = ctx->stream;
	sw.V = ctx->g.V, sw.E = ctx->g.E, sw.C = C, sw.rank = p.rank, sw.world = p.world, sw.want_depth = p.all_sub;
	sw.voff = cs.voff, sw.eoff = cs.eoff, sw.loff = cs.loff, sw.ladj = cs.ladj, sw.gid_s = cs.gid_s, sw.tip_s = cs.tip_s;
	sw.start_key = cs.start_key, sw.p_ai = sw.p_zi = nullptr;
	tm.begin("traversal_init");
	zero_component_counters(sw, C, p.all_seq ? nullptr : ctx->pw.comp_bad, p.all_seq ? nullptr : ctx->pw.err, s);
	if (p.all_seq)
		lanes.init(s);
	tm.end(p.all_seq ? 14 : 1);
	sw.comp_sel = nullptr;
	RowsOut out;
	if (p.all_seq) {
		tm.begin("traversal_seq");
		sw.stages = SEQ_STAGE_ALL;
		launch_seq_components(sw, s);
		tm.end(1);
		return out;
	}
	const int64_t dense_nb0 = parallel_rows(ctx, p, C, gstats, t, f, lanes, tm, out);
	if (p.leaf_sub) {
		leaf_passes(ctx, p, C, out.nbad, f, leaf_state, tm);
		out.sum = nullptr; // (read again when the pass is done: its total then includes these stages)
	}
	if (p.hairpins && !out.nbad) {
		run_parallel_hairpins(cs, sw, ctx->pw, C, tm, s);
		out.sum = nullptr;
	}
	redo(ctx, p, C, dense_nb0, lanes, leaf_state, tm, out);
	return out;
}

// One array of the one-lane kernels' per-component layout (component c's PVST starts at voff[c] + c) and where it goes:
// `dst` at every tree's `off` -- or, for the hairpin boundaries (`hp`, 16 bytes each), at its `hp_off`.
struct SeqArray {
	const void *src;
	void *dst;
	size_t esz; // bytes per entry
	bool hp = false;
};

// The spans of the trees `ts` in `arrays` to the host: for a few trees (when `spans_if_few`) one copy per span, else one
// bulk copy per array, sliced on the host.  `done`, if given, is recorded behind the copies.
static void fetch_seq(const std::vector<povu_hip_forest::Tree *> &ts, const uint32_t *voff, size_t P, const std::vector<SeqArray> &arrays,
		      bool spans_if_few, hipEvent_t done, hipStream_t s)
{
	struct Span {
		size_t src, dst, bytes;
	};
	auto span = [&](const povu_hip_forest::Tree &t, const SeqArray &x) {
		const size_t pb = (size_t)voff[t.component_id - 1] + (t.component_id - 1);
		return Span{pb * x.esz, (x.hp ? t.hp_off : t.off) * x.esz, (x.hp ? t.n_hairpins : t.n_pvst) * x.esz};
	};
	const bool spans = spans_if_few && ts.size() <= 32;
	std::vector<std::vector<char>> bulk;
	for (const SeqArray &x : arrays)
		if (!spans) {
			bulk.emplace_back(P * x.esz);
			HIP_CHECK(copy_async(bulk.back().data(), x.src, bulk.back().size(), hipMemcpyDeviceToHost, s));
		}
	for (const auto *t : ts)
		for (size_t k = 0; spans && k < arrays.size(); k++) {
			const Span sp = span(*t, arrays[k]);
			if (sp.bytes)
				HIP_CHECK(copy_async((char *)arrays[k].dst + sp.dst, (const char *)arrays[k].src + sp.src, sp.bytes, hipMemcpyDeviceToHost, s));
		}
	if (done)
		HIP_CHECK(hipEventRecord(done, s));
	HIP_CHECK(hipStreamSynchronize(s));
	for (const auto *t : ts)
		for (size_t k = 0; !spans && k < arrays.size(); k++) {
			const Span sp = span(*t, arrays[k]);
			if (sp.bytes)
				memcpy((char *)arrays[k].dst + sp.dst, bulk[k].data() + sp.src, sp.bytes);
		}
}

// the one-lane kernels' PVST arrays (and hairpin boundaries) of the trees `ts` into `dst` ...
static void fetch_seq_pvst(const std::vector<povu_hip_forest::Tree *> &ts, const uint32_t *voff, size_t P, const SeqWs &sw, bool hairpins,
			   const povu_hip_forest::Arrays &dst, size_t n_total, povu_hip_forest &f, hipStream_t s)
{
	std::vector<uint8_t> ors(n_total);
	std::vector<SeqArray> arrays{{sw.p_a, dst.a, 4}, {sw.p_z, dst.z, 4}, {sw.p_parent, dst.parent, 4}, {sw.p_or, ors.data(), 1}};
	if (hairpins)
		arrays.push_back({sw.hairpins, f.hairpins.data(), 16, true});
	fetch_seq(ts, voff, P, arrays, true, f.ev1, s);
	for (size_t i = 0; i < n_total; i++) {
		dst.aor[i] = ors[i] & 1;
		dst.zor[i] = (ors[i] >> 1) & 1;
	}
}

// ... and their subflubble labels (leaf_seq wrote them in the same per-component layout)
static void fetch_seq_labels(const std::vector<povu_hip_forest::Tree *> &ts, const uint32_t *voff, size_t P, const LeafState &ls,
			     povu_hip_forest::Block &b, hipStream_t s)
{
	b.sub_ai.assign(b.total, POVU_NIL);
	b.sub_zi.assign(b.total, POVU_NIL);
	b.sub_fam.assign(b.total, 0);
	fetch_seq(ts, voff, P, {{ls.p_ai, b.sub_ai.data(), 4}, {ls.p_zi, b.sub_zi.data(), 4}, {ls.p_fam, b.sub_fam.data(), 1}}, false, nullptr, s);
}

// ---- the result fetch: the dense layout the parallel stages wrote into f.blocks[0] (a mixed pass: plus blocks[1] for the
// redone components), or the one-lane kernels' per-component layout
static void fetch_result(povu_hip_ctx *ctx, const PassPlan &p, uint32_t C, const uint32_t *voff, const uint32_t *eoff, RowsOut &out,
			 povu_hip_forest &f, const LeafState &leaf_state, StageTimer &tm)
{
	hipStream_t s = ctx->stream;
	const size_t P = (size_t)ctx->g.V + C;
	tm.begin("pvst_d2h");
	const PassSummary sum(C, out.sum ? out.sum : read_summary(ctx, C, !p.all_seq, f));
	for (uint32_t c = 0; c < C; c++)
		if (sum.status(c) == 2)
			throw HipError("internal error: the spanning tree of component " + std::to_string(c + 1) + " did not reach every side");
	f.total_components = C;
	size_t total = 0, total_hp = 0;
	for (uint32_t c = 0; c < C; c++) {
		if (sum.npvst(c) == 0)
			continue;
		povu_hip_forest::Tree t;
		t.component_id = c + 1; // decompose.cpp:129
		t.n_vtx = voff[c + 1] - voff[c];
		t.n_links = eoff[c + 1] - eoff[c];
		t.n_pvst = sum.npvst(c);
		t.off = total;
		t.hp_off = total_hp;
		t.n_hairpins = p.hairpins ? sum.nbry(c) : 0;
		t.sub_c = c;
		total += sum.npvst(c);
		total_hp += t.n_hairpins;
		f.trees.push_back(t);
	}
	f.hairpins.resize(2 * total_hp);
	std::vector<povu_hip_forest::Tree *> redone;
	if (p.all_seq || (out.nbad && !out.mixed)) { // the one-lane kernels' layout for every tree
		if (!f.blocks.empty() && f.blocks[0].total != total)
			f.release_blocks();
		if (f.blocks.empty())
			f.alloc(total);
		for (auto &t : f.trees)
			redone.push_back(&t);
		tm.end(0);
		fetch_seq_pvst(redone, voff, P, ctx->sw, p.hairpins, f.blocks[0], total, f, s);
		f.labels = p.leaf_sub && total;
		if (p.leaf_sub)
			fetch_seq_labels(redone, voff, P, leaf_state, f.blocks[0], s);
		return;
	}
	// the parallel stages wrote every PVST back to back into f.blocks[0]
	if (!out.mixed && (sum.total() != total || total != ctx->pw.d_total))
		throw HipError("internal error: dense PVST size mismatch");
	if (f.blocks.empty())
		f.alloc(ctx->pw.d_total);
	size_t redo_total = 0;
	for (auto &t : f.trees) {
		if (out.mixed && sum.bad(t.component_id - 1)) {
			t.off = redo_total;
			redo_total += t.n_pvst;
			redone.push_back(&t);
		} else {
			t.off = sum.doff(t.component_id - 1);
		}
	}
	bool more = false;
	for (const auto &t : f.trees)
		if (t.n_hairpins) {
			const size_t pb = (size_t)voff[t.component_id - 1] + (t.component_id - 1);
			HIP_CHECK(copy_async(f.hairpins.data() + 2 * t.hp_off, ctx->sw.hairpins + 2 * pb, (size_t)t.n_hairpins * 16,
					     hipMemcpyDeviceToHost, s));
			more = true;
		}
	tm.end(0);
	if (!redone.empty()) { // the redone components get a block of their own
		const int bi = (int)f.blocks.size();
		povu_hip_forest::Block &x = f.alloc(redo_total);
		for (auto *t : redone)
			t->blk = bi;
		fetch_seq_pvst(redone, voff, P, ctx->sw, p.hairpins, x, redo_total, f, s);
		if (p.leaf_sub)
			fetch_seq_labels(redone, voff, P, leaf_state, x, s);
	} else if (out.fast_tail && out.tail.overlapped && !more) {
		// the arrays are still on their way: the caller (or the next accessor of the forest) waits for ev1
		f.pending = true;
		ctx->tail_pending = true;
	} else if (out.fast_tail && !more) {
		HIP_CHECK(hipEventSynchronize(f.ev1)); // (recorded behind the last copy by run_parallel_dg)
		if (tm.enabled)
			HIP_CHECK(hipStreamSynchronize(s)); // (the stage events themselves have to complete before they are read)
	} else if (more || tm.enabled || out.fast_tail) {
		HIP_CHECK(hipEventRecord(f.ev1, s));
		HIP_CHECK(hipStreamSynchronize(s));
	}
}

// ---- stage times, and the pass total unless its arrays are still on their way
static void stage_times(povu_hip_ctx *ctx, const StageTimer &tm, povu_hip_forest &f)
{
	ctx->last_times.clear();
	for (auto &r : tm.recs) {
		povu_hip_stage_time st{};
		snprintf(st.name, sizeof st.name, "%s", r.name.c_str());
		float ms = 0;
		HIP_CHECK(hipEventElapsedTime(&ms, r.a, r.b));
		st.ms = ms;
		st.launches = r.launches;
		ctx->last_times.push_back(st);
	}
	if (!f.pending) {
		povu_hip_stage_time st{};
		snprintf(st.name, sizeof st.name, "total");
		f.ready();
		st.ms = f.pass_ms;
		ctx->last_times.push_back(st);
	}
}

} // namespace

extern "C" povu_hip_forest *povu_hip_decompose(povu_hip_ctx *ctx, const povu_hip_opts *opts, char *err, size_t errlen)
{
	// declared outside the try block: on a failure the stream is drained BEFORE the forest returns its pinned
	// result block to the pool (kernels that write into it may still be queued)
	std::unique_ptr<povu_hip_forest> f;
	XferScope xfer(ctx);
	try {
		if (ctx && !ctx->g.block && ctx->shard_total_components) { // a shard without components: nothing to do
			f = std::make_unique<povu_hip_forest>();
			f->pool = ctx->pool;
			f->total_components = ctx->shard_total_components;
			ctx->last_times.clear();
			ctx->last_links = 0;
			return f.release();
		}
		if (!ctx || !ctx->g.block)
			throw HipError("no graph resident: call povu_hip_graph_upload first");
		HIP_CHECK(hipSetDevice(ctx->device));
		const PassPlan p = plan_pass(opts);
		if (!p.overlap_tail)
			ctx->wait_tail();
		const ResidentGraph &g = ctx->g;
		Sizes z = rowb_begin(ctx, p);
		StageTimer &tm = ctx->timer;
		// the forest owns the two events that time its pass: ev0 at the first kernel, ev1 behind the last byte that reaches the host
		f = std::make_unique<povu_hip_forest>();
		f->pool = ctx->pool;
		HIP_CHECK(hipEventCreate(&f->ev0));
		HIP_CHECK(hipEventCreate(&f->ev1));
		HIP_CHECK(hipEventRecord(f->ev0, ctx->stream));

		const RowB rb = row_b(ctx, p, z, tm);
		const uint32_t C = rb.C;
		z.set_components(C);
		const bool tail_waited = carve_stages(ctx, p, z, C, tm);
		ctx->host.wait(rb.sizes);
		const CompTables tables = component_tables(ctx, p, C, rb.voff, rb.eoff, tail_waited);
		f->meta_reserve = (size_t)C + 1; // room behind the arrays for the tree table of povu_hip_forest_share
		SeqLanes lanes{ctx, z, p.hairpins};
		LeafState leaf_state;
		RowsOut out = rows_c_to_g(ctx, p, C, rb.gstats, tables, *f, lanes, leaf_state, tm);
		fetch_result(ctx, p, C, rb.voff, rb.eoff, out, *f, leaf_state, tm);
		if (!p.leaf_sub)
			ctx->ws_leaf.release(); // (kept from one -s pass to the next, like the inserting passes' arena below: a hipMalloc of
						// several GB right after the hipFree of the pass before stalled for over a second once; a
						// pass without the leaf passes gives it back)
		if (!p.all_sub)
			ctx->ws_sub.release(); // (the inserting passes keep their phase arenas from one -s pass to the next, no longer)
		stage_times(ctx, tm, *f);
		ctx->last = LastPass{true, p, C, out.nbad, out.mixed, out.redo_pvst_only, out.stack_export_pending};
		ctx->last.narrow_counts = !p.all_seq && !p.seq_tree && ctx->pw.narrow_ordcnt;
		ctx->last.narrow_forms = !ctx->last.narrow_counts ? 0 : 1 | (ctx->pw.narrow_srccnt ? 2 : 0) | (ctx->pw.narrow_incnt ? 4 : 0);
		ctx->last.prefix_records = ctx->last.narrow_counts ? ctx->pw.prefix_records : 0;
		if (p.world == 1 && ctx->shard_comp_ids.empty()) { // (povu_hip_forest_walks: a forest of the whole resident graph)
			f->walk_ctx = ctx;
			f->walk_gen = g.gen;
		}
		return f.release();
	} catch (const std::exception &e) {
		if (ctx && ctx->stream)
			(void)hipStreamSynchronize(ctx->stream);
		if (ctx && ctx->side.stream)
			(void)hipStreamSynchronize(ctx->side.stream);
		f.reset();
		set_err(err, errlen, e.what());
		return nullptr;
	}
}

extern "C" uint32_t povu_hip_forest_total_components(const povu_hip_forest *f) { return f ? f->total_components : 0; }
extern "C" uint32_t povu_hip_forest_tree_count(const povu_hip_forest *f) { return f ? (uint32_t)f->trees.size() : 0; }

extern "C" int povu_hip_forest_wait(povu_hip_forest *f)
{
	if (!f)
		return 1;
	f->ready();
	return 0;
}
extern "C" double povu_hip_forest_pass_ms(povu_hip_forest *f)
{
	if (!f)
		return -1.0;
	f->ready();
	return f->pass_ms;
}

extern "C" double povu_hip_forest_span_ms(povu_hip_forest *first, povu_hip_forest *last)
{
	if (!first || !last || !first->ev0 || !last->ev1)
		return -1.0;
	first->ready();
	last->ready();
	float ms = 0;
	return hipEventElapsedTime(&ms, first->ev0, last->ev1) == hipSuccess ? (double)ms : -1.0;
}

extern "C" int povu_hip_forest_get(const povu_hip_forest *f, uint32_t i, povu_hip_tree *out)
{
	if (!f || !out || i >= f->trees.size())
		return 1;
	const_cast<povu_hip_forest *>(f)->ready(); // (the arrays of a POVU_HIP_F_ASYNC forest may still be on their way)
	const auto &t = f->trees[i];
	out->component_id = t.component_id;
	out->n_vtx = t.n_vtx;
	out->n_links = t.n_links;
	out->n_pvst = t.n_pvst;
	const auto &b = f->blocks[(size_t)t.blk];
	out->a_id = b.a + t.off;
	out->z_id = b.z + t.off;
	out->a_or = b.aor + t.off;
	out->z_or = b.zor + t.off;
	out->parent = b.parent + t.off;
	out->n_hairpins = t.n_hairpins;
	out->hairpins = t.n_hairpins ? f->hairpins.data() + 2 * t.hp_off : nullptr;
	return 0;
}

extern "C" int povu_hip_forest_raw(const povu_hip_forest *f, const void **block, size_t *bytes, uint64_t *total,
				   uint64_t offsets[5])
{
	if (!f || !block || !bytes || !total || !offsets || f->blocks.size() > 1)
		return 1; // (several blocks -- a merged forest, a mixed pass: no single raw view)
	const_cast<povu_hip_forest *>(f)->ready();
	if (f->blocks.empty()) { // (a forest without trees, of a shard without components)
		*block = nullptr, *bytes = 0, *total = 0;
		std::fill(offsets, offsets + 5, 0ull);
		return 0;
	}
	const auto &b = f->blocks[0];
	*block = b.p;
	*bytes = b.bytes;
	*total = b.total;
	const char *p = static_cast<const char *>(b.p);
	offsets[0] = (uint64_t)((const char *)b.a - p);
	offsets[1] = (uint64_t)((const char *)b.z - p);
	offsets[2] = (uint64_t)((const char *)b.parent - p);
	offsets[3] = (uint64_t)((const char *)b.aor - p);
	offsets[4] = (uint64_t)((const char *)b.zor - p);
	return 0;
}

extern "C" uint64_t povu_hip_forest_first(const povu_hip_forest *f, uint32_t i)
{
	return (f && i < f->trees.size()) ? (uint64_t)f->trees[i].off : 0;
}

extern "C" void povu_hip_forest_free(povu_hip_forest *f) { delete f; }

// mto::to_pvst::write_pvst, src/mto/to_pvst.cpp:23-109
extern "C" int povu_hip_forest_get_sub(const povu_hip_forest *f, uint32_t i, const uint32_t **ai, const uint32_t **zi,
				       const uint8_t **fam)
{
	if (!f || i >= f->trees.size())
		return 1;
	const auto &t = f->trees[i];
	const auto &b = f->blocks[(size_t)t.blk];
	if (!f->labels || t.off + t.n_pvst > b.sub_fam.size())
		return 3; // the forest was not decomposed with POVU_HIP_F_LEAF_SUBFLUBBLES
	if (ai)
		*ai = b.sub_ai.data() + t.off;
	if (zi)
		*zi = b.sub_zi.data() + t.off;
	if (fam)
		*fam = b.sub_fam.data() + t.off;
	return 0;
}

extern "C" int povu_hip_forest_get_subtree(const povu_hip_forest *f, uint32_t i, povu_hip_subtree *out)
{
	if (!f || !out || i >= f->trees.size())
		return 1;
	const_cast<povu_hip_forest *>(f)->ready();
	const auto &t = f->trees[i];
	const SubForest *x = f->blocks[(size_t)t.blk].subx.get();
	if (!x || t.sub_c + 1 >= x->voff.size())
		return 3; // the forest was not decomposed with POVU_HIP_F_SUBFLUBBLES
	const uint64_t b = x->voff[t.sub_c], e = x->voff[t.sub_c + 1];
	out->n_total = (uint32_t)(e - b);
	out->n_flubble_like = t.n_pvst;
	out->n_concealed = x->counts[3 * (size_t)t.sub_c];
	out->n_midi = x->counts[3 * (size_t)t.sub_c + 1];
	out->n_smothered = x->counts[3 * (size_t)t.sub_c + 2];
	out->fam = x->fam + b;
	out->or1 = x->or1 + b;
	out->or2 = x->or2 + b;
	out->route = x->route + b;
	out->id1 = x->id1 + b;
	out->id2 = x->id2 + b;
	out->child_off = x->coff + b;
	out->child = x->child;
	return 0;
}

// the sites of every tree through povu_hip_sites_add_tree (host/vcf.cpp): the extended tree of -s, else the PVST with the T / O
// letters of --leaf-subflubbles, else the PVST as it is
extern "C" povu_hip_sites *povu_hip_forest_sites(const povu_hip_forest *f)
{
	auto *s = f ? static_cast<povu_hip_sites *>(calloc(1, sizeof(povu_hip_sites))) : nullptr;
	std::vector<uint32_t> par;
	for (uint32_t i = 0; s && i < f->trees.size(); i++) {
		povu_hip_subtree x;
		povu_hip_tree t;
		const uint8_t *fam = nullptr;
		int rc;
		if (povu_hip_forest_get_subtree(f, i, &x) == 0) {
			par.assign(x.n_total, POVU_HIP_NIL);
			for (uint32_t v = 0; v < x.n_total; v++)
				for (uint32_t k = x.child_off[v]; k < x.child_off[v + 1]; k++)
					if (x.child[k] < x.n_total)
						par[x.child[k]] = v;
			rc = povu_hip_sites_add_tree(s, i, x.n_total, x.id1, x.id2, x.or1, x.or2, par.data(), x.fam);
		} else {
			rc = povu_hip_forest_get(f, i, &t);
			povu_hip_forest_get_sub(f, i, nullptr, nullptr, &fam); // (leaves fam null when the forest carries no letters)
			rc = rc ? rc : povu_hip_sites_add_tree(s, i, t.n_pvst, t.a_id, t.z_id, t.a_or, t.z_or, t.parent, fam);
		}
		if (rc) {
			povu_hip_sites_free(s);
			s = nullptr;
		}
	}
	return s;
}

// write_pvst, src/mto/to_pvst.cpp:31-109, of a tree with its -s vertices
extern "C" char *povu_hip_pvst_format_subtree(const povu_hip_subtree *t, size_t *len)
{
	if (!t)
		return nullptr;
	std::string o;
	o.reserve(32 * (size_t)t->n_total + 64);
	o += "H\t0.0.3\t.\t.\t.\n";
	for (uint32_t v = 0; v < t->n_total; v++) {
		o += (char)t->fam[v];
		o += '\t';
		o += std::to_string(v);
		o += '\t';
		if (t->fam[v] == 'D') {
			o += '.';
		} else { // id_or_t::as_str, include/povu/graph/types.hpp:85-95
			o += t->or1[v] ? '<' : '>';
			o += std::to_string(t->id1[v]);
			o += t->or2[v] ? '<' : '>';
			o += std::to_string(t->id2[v]);
		}
		o += '\t';
		const uint32_t c0 = t->child_off[v], c1 = t->child_off[v + 1];
		if (c0 == c1) {
			o += '.';
		} else { // print_with_comma, include/povu/common/utils.hpp:44-55
			for (uint32_t k = c0; k < c1; k++) {
				o += std::to_string(t->child[k]);
				if (k + 1 < c1)
					o += ", ";
			}
		}
		o += '\t';
		if (t->route[v])
			o += (char)t->route[v];
		else
			o += '.';
		o += '\n';
	}
	char *buf = static_cast<char *>(malloc(o.size() + 1));
	if (!buf)
		return nullptr;
	memcpy(buf, o.data(), o.size() + 1);
	if (len)
		*len = o.size();
	return buf;
}

extern "C" char *povu_hip_forest_pvst_text(const povu_hip_forest *f, uint32_t i, size_t *len)
{
	povu_hip_subtree st;
	if (povu_hip_forest_get_subtree(f, i, &st) == 0)
		return povu_hip_pvst_format_subtree(&st, len);
	povu_hip_tree t;
	if (povu_hip_forest_get(f, i, &t) != 0)
		return nullptr;
	const uint8_t *fam = nullptr;
	if (povu_hip_forest_get_sub(f, i, nullptr, nullptr, &fam) != 0)
		fam = nullptr;
	return povu_hip_pvst_format_fam(t.n_pvst, t.a_id, t.z_id, t.a_or, t.z_or, t.parent, fam, len);
}

extern "C" char *povu_hip_pvst_format(uint32_t n_pvst, const uint32_t *a_id, const uint32_t *z_id, const uint8_t *a_or,
				      const uint8_t *z_or, const uint32_t *parent, size_t *len)
{
	return povu_hip_pvst_format_fam(n_pvst, a_id, z_id, a_or, z_or, parent, nullptr, len);
}

extern "C" char *povu_hip_pvst_format_fam(uint32_t n_pvst, const uint32_t *a_id, const uint32_t *z_id, const uint8_t *a_or,
					  const uint8_t *z_or, const uint32_t *parent, const uint8_t *fam, size_t *len)
{
	if (n_pvst == 0 || !a_id || !z_id || !a_or || !z_or || !parent)
		return nullptr;
	if (fam)
		for (uint32_t v = 0; v < n_pvst; v++)
			if (fam[v] != (v == 0 ? 'D' : 'F') && (v == 0 || (fam[v] != 'T' && fam[v] != 'O')))
				return nullptr; // line letters this writer knows: D for the root, F / T / O below it
	struct {
		uint32_t n_pvst;
		const uint32_t *a_id, *z_id, *parent;
		const uint8_t *a_or, *z_or;
	} t{n_pvst, a_id, z_id, parent, a_or, z_or};
	for (uint32_t v = 1; v < n_pvst; v++)
		if (parent[v] >= v)
			return nullptr; // a PVST parent always precedes its children (emission order)
	const uint32_t n = t.n_pvst;
	// children of every PVST vertex in emission order (children_v push_back, pvst.hpp:882-892)
	std::unique_ptr<uint32_t[]> coff(new uint32_t[(size_t)n + 2]), cadj(new uint32_t[n]); // (uninitialised)
	std::fill(coff.get(), coff.get() + n + 2, 0u);
	for (uint32_t v = 1; v < n; v++)
		coff[t.parent[v] + 2]++; // (shifted by one: after the sums coff[p + 1] is where p's children start, and the fill
	for (uint32_t v = 0; v < n; v++) //  below advances it to where they end = where those of p + 1 start)
		coff[v + 2] += coff[v + 1];
	for (uint32_t v = 1; v < n; v++)
		cadj[coff[t.parent[v] + 1]++] = v;
	// One buffer of the largest size the text can have, written front to back (a 10^6-vertex PVST is 5 * 10^6 numbers: a
	// library call per number and a growing string were most of the CLI's write time).  Per line at most: letter + tab 2,
	// vertex 10, tab 1, the two oriented endpoints 22, tab 1, '.' 1, closing field 3; per child entry 10 + ", ".
	const size_t cap = 16 + (size_t)n * 40 + (size_t)n * 12 + 1;
	char *buf = (char *)malloc(cap);
	if (!buf)
		return nullptr;
	static const char D2[] = "0001020304050607080910111213141516171819202122232425262728293031323334353637383940414243444546474849"
				 "5051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";
	char *o = buf;
	auto put = [&](uint32_t v) {
		const int len = v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 :
				v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
		char *e = o + len;
		o = e;
		while (v >= 100u) {
			const uint32_t r = v % 100u;
			v /= 100u;
			e -= 2;
			e[0] = D2[2 * r], e[1] = D2[2 * r + 1];
		}
		if (v >= 10u)
			e[-2] = D2[2 * v], e[-1] = D2[2 * v + 1];
		else
			e[-1] = (char)('0' + v);
	};
	memcpy(o, "H\t0.0.3\t.\t.\t.\n", 14); // to_pvst.cpp:23-28
	o += 14;
	for (uint32_t v = 0; v < n; v++) {
		*o++ = fam ? (char)fam[v] : (v == 0 ? 'D' : 'F'); // to_pvst.cpp:52-79: the line identifier follows the vertex family
		*o++ = '\t';
		put(v);
		*o++ = '\t';
		if (v == 0) {
			*o++ = '.';
		} else { // id_or_t::as_str, include/povu/graph/types.hpp:85-95
			*o++ = t.a_or[v] ? '<' : '>';
			put(t.a_id[v]);
			*o++ = t.z_or[v] ? '<' : '>';
			put(t.z_id[v]);
		}
		*o++ = '\t';
		const uint32_t c0 = coff[v], c1 = coff[v + 1];
		if (c0 == c1) {
			*o++ = '.';
		} else { // print_with_comma, include/povu/common/utils.hpp:44-55
			for (uint32_t k = c0; k < c1; k++) {
				put(cadj[k]);
				if (k + 1 < c1)
					*o++ = ',', *o++ = ' ';
			}
		}
		*o++ = '\t';
		*o++ = v == 0 ? '.' : 'L';
		*o++ = '\n';
	}
	*o = 0;
	if (len)
		*len = (size_t)(o - buf);
	return buf;
}

extern "C" int povu_hip_last_stage_times(const povu_hip_ctx *ctx, povu_hip_stage_time *out, int max)
{
	if (!ctx)
		return 0;
	int n = (int)ctx->last_times.size();
	if (out)
		for (int i = 0; i < n && i < max; i++)
			out[i] = ctx->last_times[i];
	return n;
}

extern "C" uint32_t povu_hip_last_seq_redo(const povu_hip_ctx *ctx) { return ctx ? ctx->last.seq_redo : 0; }

extern "C" uint64_t povu_hip_last_links_processed(const povu_hip_ctx *ctx) { return ctx ? ctx->last_links : 0; }

extern "C" int povu_hip_last_narrow_counts(const povu_hip_ctx *ctx)
{
	return ctx && ctx->last.valid && ctx->last.narrow_counts ? ctx->last.narrow_forms : 0;
}
extern "C" int povu_hip_last_prefix_records(const povu_hip_ctx *ctx) { return ctx && ctx->last.valid ? ctx->last.prefix_records : 0; }
extern "C" uint64_t povu_hip_wide_repeats(const povu_hip_ctx *ctx) { return ctx ? ctx->wide_repeats : 0; }

extern "C" int povu_hip_last_black_only_classes(const povu_hip_ctx *ctx)
{
	return ctx && ctx->last.valid && !ctx->last.plan.all_seq && ctx->pw.black_only_used ? 1 : 0;
}

extern "C" int povu_hip_last_crossings(povu_hip_ctx *ctx, uint32_t out[2])
{
	if (!ctx || !out)
		return 1;
	out[0] = out[1] = 0;
	if (!ctx->last.valid || ctx->last.plan.all_seq || !ctx->pw.laminar_checked)
		return 0;
	ctx->quiesce();
	if (hipSetDevice(ctx->device) != hipSuccess)
		return 2;
	static_assert(PW_N_CROSSED == PW_N_X + 1, "the two crossing words are copied as a pair");
	return hipMemcpy(out, ctx->pw.err + PW_N_X, 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
}

extern "C" int povu_hip_last_lsz_field(povu_hip_ctx *ctx, uint32_t out[2])
{
	if (!ctx || !out)
		return 1;
	out[0] = out[1] = 0;
	if (!ctx->last.valid || ctx->last.plan.all_seq || !ctx->pw.black_only_used)
		return 0;
	ctx->quiesce();
	if (hipSetDevice(ctx->device) != hipSuccess)
		return 2;
	try {
		out[0] = ctx->pw.lsz_field.w;
		out[1] = count_saturated(ctx->pw, ctx->stream);
	} catch (const std::exception &) {
		return 2;
	}
	return 0;
}

extern "C" int povu_hip_last_laminar_check_ran(const povu_hip_ctx *ctx)
{
	return ctx && ctx->last.valid && !ctx->last.plan.all_seq && ctx->pw.laminar_checked ? 1 : 0;
}
