// context.hip -- the context behind the C ABI (include/povu_hip.h) and its memory: the pool of page-locked result blocks, context
// create / destroy and the arenas, the resident graph and its upload, the carving of the decompose workspaces (declared to
// the pass in context.hpp) and the workspace estimates and prewarm built on it.
#include "context.hpp"

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>

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

// What the stage workspace of a pass has to hold (par_kernels.hpp: StageWsOpts).  The plain all-parallel pass needs neither
// the per-vertex tables of a sequential tree stage, nor the keys of its bracket sort, nor the hairpin report's arrays, and
// takes the wave walk's arrays only when it meets large classes.  Brackets: every link outside the spanning forest of
// the segments starts at most one back edge (E - (V - C) of them), every side without links at most one to the root
// (spanning_tree.cpp:433-438), and the class stage adds at most one capping or simplifying edge per tree vertex.
StageWsOpts stage_opts(size_t V, size_t E, size_t C, size_t empty_sides, bool seq_tree, bool hairpins)
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
