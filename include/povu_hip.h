/*
 * povu_hip.h -- C ABI of the MI355X (gfx950) `decompose` hot path.
 *
 * This is the boundary a povu maintainer binds instead of the CPU calls that
 * sit between "GFA parsed" and "PVST ready to write" in
 *   povu::subcommands::decompose::do_decompose   app/subcommand/decompose.cpp:94-160
 * i.e. it replaces, for that path and nothing else:
 *   bd::VG (adjacency built by mto::from_gfa::to_bd)    src/mto/from_gfa.cpp:191-277
 *   bd::VG::componetize                                  src/povu/graph/bidirected.cpp:477-602
 *   pst::Tree::from_bd                                   src/povu/graph/spanning_tree.cpp:262-463
 *   povu::flubbles::find_flubbles                        src/povu/algorithms/flubbles.cpp:721-745
 * (INTEGRATION.md shows the reference-side stub.)
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 * All functions return 0 / non-NULL on success; on failure they return
 * non-zero / NULL and write a message to `err` (when given).  There is no CPU
 * fallback: without a usable HIP device every compute entry point fails.
 *
 * Threading: a context owns one HIP stream and one workspace arena and must be
 * used by one thread at a time; independent contexts may be used concurrently
 * (the reference's FFI makes the same promise, povu-rs/src/graph.rs:425).
 */
#ifndef POVU_HIP_H
#define POVU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POVU_HIP_NIL 0xFFFFFFFFu
/* vertex sides, reference pgt::v_end_e (include/povu/graph/types.hpp:39-42) */
#define POVU_SIDE_L 0
#define POVU_SIDE_R 1
/* tip marks per vertex (reference bd::VG::tips_, src/mto/from_gfa.cpp:262-277) */
#define POVU_TIP_NONE 0
#define POVU_TIP_L 1
#define POVU_TIP_R 2

typedef struct povu_hip_ctx povu_hip_ctx;
typedef struct povu_hip_forest povu_hip_forest;

/* number of visible HIP devices (0 when none; never touches a device) */
int povu_hip_device_count(void);

/* create / destroy a context on `device` */
povu_hip_ctx *povu_hip_create(int device, char *err, size_t errlen);
void povu_hip_destroy(povu_hip_ctx *ctx);
/* gives every workspace arena of `ctx` back to the device; the resident graph, paths, sequences, a received shard and the
 * packed shards stay (povu_hip_arena_report says which is which).  The next call reserves what it needs again.  Ends the debug
 * exports of the last pass.  0 on success */
int povu_hip_release_workspace(povu_hip_ctx *ctx);

/*
 * Row A (device part).  Copies the link arrays to HBM and builds the per-side
 * CSR of the bidirected graph there (what bd::VG::add_vertex/add_edge/add_tip
 * build on the CPU, bidirected.cpp:309-340).
 *   vid[n_vtx]   segment id of vertex idx (the loader adds vertices ascending by id)
 *   v1,v2[n_links] endpoint vertex idx, s1,s2[n_links] endpoint side (POVU_SIDE_*)
 *   tips[n_vtx]  POVU_TIP_* per vertex, or NULL to infer them as to_bd does
 * The graph stays resident until the next upload or povu_hip_destroy.
 */
int povu_hip_graph_upload(povu_hip_ctx *ctx, uint32_t n_vtx, const uint32_t *vid, uint32_t n_links,
			  const uint32_t *v1, const uint8_t *s1, const uint32_t *v2, const uint8_t *s2,
			  const uint8_t *tips, char *err, size_t errlen);

/* device time of the last upload by HIP events, milliseconds: [0] host-to-device copies, [1] CSR build (side
 * degrees, offsets, per-side sorted adjacency, other-end table, tips), [2] reverse-slot table */
int povu_hip_last_upload_times(const povu_hip_ctx *ctx, double out_ms[3]);

typedef struct {
	uint32_t rank;	/* this process' shard (component sharding, 0-based) */
	uint32_t world; /* number of shards; 0 or 1 = everything */
	uint32_t flags; /* POVU_HIP_F_* */
} povu_hip_opts;
#define POVU_HIP_F_HAIRPINS 1u /* also report hairpin boundaries (--hairpins, flubbles.cpp:712-717) */
#define POVU_HIP_F_SEQUENTIAL 2u /* force the one-lane-per-component kernels for every stage */
#define POVU_HIP_F_SEQ_TREE 4u /* sequential spanning tree, parallel classes/stack/PVST (A/B testing) */
#define POVU_HIP_F_FORCE_REDO 8u /* treat every component as flagged for the sequential redo (tests) */
#define POVU_HIP_F_REDO_ODD 256u /* treat every second component as flagged for the sequential redo (tests of the mixed result) */
#define POVU_HIP_F_NO_STAGE_TIMES 32u /* record only the pass total, not the per-stage HIP events */
#define POVU_HIP_F_BIG_CLASS_DFS 64u /* always walk the classes with the filtered-scan-list DFS large classes get (A/B testing) */
#define POVU_HIP_F_SPARSE_SPLITTERS 128u /* list ranking with 1-in-16 splitters instead of 1-in-8 (A/B testing) */
#define POVU_HIP_F_ALL_VERTEX_CLASSES 512u /* number the cycle classes of all tree edges, not just the black ones the candidate stack holds (A/B testing) */
#define POVU_HIP_F_CHECK_LAMINAR 1024u /* always run the laminarity check of the candidate stack's (prev, i) intervals; by default it only runs when the literal hi_2 rule capped differently from the second-highest reach, DESIGN.md section 4 has the proof for the other case (A/B testing, fuzzing) */
#define POVU_HIP_F_LEAF_SUBFLUBBLES 2048u /* the two relabelling passes of `-s`: find_tiny (tiny.cpp:100-129) and find_parallel (parallel.cpp:263-287) on every PVST; the forest then also carries ai / zi and the line letter of every vertex (povu_hip_forest_get_sub).  Not the reference's whole `-s`: that is POVU_HIP_F_SUBFLUBBLES */
#define POVU_HIP_F_SUBFLUBBLES 8192u /* all five passes of `-s` (app/subcommand/decompose.cpp:63-70): implies POVU_HIP_F_LEAF_SUBFLUBBLES, then find_concealed (concealed.cpp:1198-1243), find_midi (midi.cpp:225-268) and find_smothered (smothered.cpp:385-432) INSERT vertices into every PVST; the forest carries the extended trees (povu_hip_forest_get_subtree) and povu_hip_forest_pvst_text prints them.  Parity unpinned: the reference holds no T / O / C / M / S line; undefined behaviour of the reference is decided as oracle/povu_oracle_sub.inc lists */
#define POVU_HIP_F_ASYNC 4096u /* povu_hip_decompose returns as soon as the forest is laid out -- tree table, sizes, the page-locked result block -- while the last kernels and the copy of the PVST arrays to the host are still in flight; povu_hip_forest_wait (or any accessor of the forest: they wait by themselves) completes it.  A second povu_hip_decompose on the same context may start at once: its kernels run while the copy engine still moves the first result over PCIe.  Ignored (the call completes before it returns) without POVU_HIP_F_NO_STAGE_TIMES, with hairpins, subflubble labels, the test modes, and when the pass needs the laminarity check */
#define POVU_HIP_F_SORTED_ADJ 16u /* build the local adjacency with the radix sort hub graphs use (A/B testing) */

/*
 * Rows B-G.  Decomposes the resident graph: weakly connected components
 * (numbered 1.. by minimum vertex idx, decompose.cpp:129), component
 * re-indexing, biedged spanning tree, cycle-equivalence classes, candidate
 * stack, next_seen and the PVST of every component with >= 3 vertices
 * (decompose.cpp:135-142) that belongs to this shard.  The result lives in
 * host memory.
 */
povu_hip_forest *povu_hip_decompose(povu_hip_ctx *ctx, const povu_hip_opts *opts, char *err, size_t errlen);

/*
 * Row B on its own (what `povu info` and `povu prune` need, app/subcommand/info.cpp:19-45,
 * prune.cpp:17-41): the components exactly as bd::VG::componetize builds them -- ordered by minimum
 * vertex idx, vertices ascending, links in first-encounter order stored from the encountering side,
 * self loops as (ve, complement(ve)) (bidirected.cpp:552-569, :66-77).
 */
typedef struct {
	uint32_t n_components;
	uint32_t n_vtx, n_links;
	const uint32_t *vtx_off;  /* [n_components + 1] component c owns vertices [vtx_off[c], vtx_off[c+1]) */
	const uint32_t *link_off; /* [n_components + 1] */
	const uint32_t *vtx_id;	  /* [n_vtx] segment id, local vertex order, component-major */
	const uint8_t *vtx_tip;	  /* [n_vtx] POVU_TIP_* */
	const uint32_t *l_v1, *l_v2; /* [n_links] LOCAL vertex idx of the two ends, local link order */
	const uint8_t *l_s1, *l_s2;  /* [n_links] sides */
} povu_hip_components;
povu_hip_components *povu_hip_componetize(povu_hip_ctx *ctx, char *err, size_t errlen);
void povu_hip_components_free(povu_hip_components *c);

/* ---- multi-GPU: component sharding, one process per GPU ----
 * Replaces the static per-thread chunks of do_decompose (app/subcommand/decompose.cpp:78-92,116-157): the
 * components of the graph resident on the ROOT rank are labelled there (row B's union-find kernels), bin-packed
 * over the ranks (greedy longest-processing-time on links + segments), the links are partitioned on the device and
 * every rank receives the sub-graph of its components; ranks decompose independently; the PVST arrays are gathered
 * on the root.  No collective touches the traversal itself. */
typedef struct povu_hip_shards povu_hip_shards;
typedef struct {
	uint32_t n_vtx, n_links, n_components; /* of this shard */
	uint64_t weight;		       /* LPT load: links + segments (+1 per component) */
	size_t bytes;			       /* size of the packed shard */
	const void *device_ptr;		       /* packed shard in the root's HBM */
} povu_hip_shard_info;
/* LPT assignment of `n` weights to `world` ranks: heaviest first (stable), each to the least loaded rank (lowest
 * rank on ties), every placed item also costs 1.  Host only -- no GPU needed. */
int povu_hip_lpt_assign(const uint64_t *weights, uint32_t n, uint32_t world, uint32_t *owner_out);
/* Partitions the graph resident in `ctx` into `world` packed shards in device memory.  Vertices keep their
 * ascending global order inside a shard and links their L-line order, so a shard's own component numbering
 * preserves the global order. */
povu_hip_shards *povu_hip_shard_partition(povu_hip_ctx *ctx, uint32_t world, char *err, size_t errlen);
uint32_t povu_hip_shards_world(const povu_hip_shards *s);
uint32_t povu_hip_shards_total_components(const povu_hip_shards *s);
int povu_hip_shards_get(const povu_hip_shards *s, uint32_t rank, povu_hip_shard_info *out);
/* device time of the partition (HIP events, ms): [0] labelling, [1] weights + LPT, [2] partition kernels */
int povu_hip_shards_times(const povu_hip_shards *s, double out_ms[3]);
/* (the packed shards live in an arena of `ctx`: they stay valid until the next partition on that context or its destruction)
 * copies packed shard `rank` to host memory (`dst` holds info.bytes) -- for transports other than RCCL */
int povu_hip_shards_export(const povu_hip_shards *s, povu_hip_ctx *ctx, uint32_t rank, void *dst);
void povu_hip_shards_free(povu_hip_shards *s);
/* Makes a packed shard the resident graph of `ctx` (CSR built on the device).  `packed` is host memory
 * (on_device = 0) or memory of ctx's device (on_device = 1).  The shard's component ids (1-based ids in the whole
 * graph, ascending) are kept in the context for povu_hip_forest_globalize / the gather. */
int povu_hip_graph_upload_shard(povu_hip_ctx *ctx, const void *packed, size_t bytes, int on_device, char *err, size_t errlen);
/* number of components of the WHOLE graph the resident shard was cut from (0: the resident graph is no shard) */
uint32_t povu_hip_shard_total_components(const povu_hip_ctx *ctx);
/* rewrites the component ids of a forest computed on a shard to the ids of the whole graph */
int povu_hip_forest_globalize(povu_hip_forest *f, const povu_hip_ctx *ctx);
/* Wire format of a forest: [u64 n_trees, u64 total_entries, u64 total_components | per tree u32 component id, n_vtx,
 * n_links, n_pvst | a_id | z_id | parent (u32 x total) | a_or | z_or (u8 x total)], every section padded to 64 B. */
size_t povu_hip_forest_pack_size(const povu_hip_forest *f);
int povu_hip_forest_pack(const povu_hip_forest *f, void *dst, size_t cap);
/* merges packed forests (host memory) into one forest, trees ordered by component id */
povu_hip_forest *povu_hip_forest_merge(povu_hip_ctx *ctx, const void *const *packed, const size_t *bytes, uint32_t n,
				       char *err, size_t errlen);

/* RCCL communicator owned by the library (ncclSend / ncclRecv over xGMI on the context's stream).  The unique id
 * is created on one rank (povu_hip_comm_unique_id) and handed to the others by the launcher. */
typedef struct povu_hip_comm povu_hip_comm;
#define POVU_HIP_COMM_ID_BYTES 128
int povu_hip_comm_unique_id(char id[POVU_HIP_COMM_ID_BYTES], char *err, size_t errlen);
povu_hip_comm *povu_hip_comm_create(povu_hip_ctx *ctx, const char id[POVU_HIP_COMM_ID_BYTES], uint32_t rank, uint32_t world,
				    char *err, size_t errlen);
void povu_hip_comm_destroy(povu_hip_comm *c);
/* Scatter: on the root (rank 0) `shards` is the partition of its resident graph, elsewhere NULL.  On return every
 * rank's context holds its shard as resident graph (on the root it replaces the whole graph; a root that wants to
 * keep the whole graph resident scatters from a second context).  Collective: every rank of the communicator must
 * call it.  Two failures travel in the handshake and make the call fail on ALL ranks before any shard moves: the root has
 * no partition for exactly `world` ranks, a receiver has no room for its shard.  Bad ARGUMENTS (a null handle, a
 * destination context that is not the communicator's) fail on the calling rank alone, before its first collective: the
 * other ranks then wait -- a caller's bug, not a run-time condition.  EXPERIMENTAL: the library's own RCCL transfers have
 * never run on more than one GPU (the one-process engine below and the torch.distributed path of bench.py are what is
 * rehearsed).  Every RCCL call of a communicator runs on the communicator's own stream. */
int povu_hip_comm_scatter(povu_hip_comm *c, const povu_hip_shards *shards, povu_hip_ctx *dst_ctx, char *err, size_t errlen);
/* Gather: every rank passes the (globalized) forest of its shard; the root gets the merged forest, the others an
 * empty one.  Collective like the scatter: a forest that cannot travel (hairpin boundaries, a merged forest) or a root
 * without room fails the call on all ranks before any block moves. */
povu_hip_forest *povu_hip_comm_gather(povu_hip_comm *c, const povu_hip_forest *mine, char *err, size_t errlen);
/* wall time of the last scatter / gather on this rank, milliseconds */
int povu_hip_comm_times(const povu_hip_comm *c, double out_ms[2]);

/* ---- gather without a second PCIe crossing (several processes on one node) ----
 * A rank's decompose already lands its PVST block in page-locked HOST memory over its own GPU's PCIe link.  After
 * povu_hip_share_results the blocks of a context's forests are POSIX shared-memory segments ("/povu.<tag>.<k>",
 * page-locked and mapped for the device): the root maps a rank's segment by name and reads the arrays where they are.
 * What the ranks exchange is one 64-byte descriptor each (RCCL all-gather, torch.distributed, a pipe ...).
 * Replaces the per-thread ownership of do_decompose's workers (app/subcommand/decompose.cpp:116-157), which write from
 * their own memory. */
/* from now on this context's result blocks are shared segments named after `tag` (at most 96 characters, no '/');
 * the multi-process convention is tag = "<job>.<rank>" */
int povu_hip_share_results(povu_hip_ctx *ctx, const char *tag, char *err, size_t errlen);
/* describes the block of `f` for another process: desc = [magic, segment k, segment bytes, trees, entries, components of the
 * whole graph, offset of the tree table, 0 (the caller stores the sender's rank here)]; the tree table is written into
 * the segment behind the arrays.  A forest whose trees sit in several blocks is first brought into one.  Returns 2 when the
 * forest's block is no shared segment, 4 for hairpin boundaries / subflubble labels (they do not travel). */
int povu_hip_forest_share(povu_hip_forest *f, uint64_t desc[8]);
/* Root: the merged forest of `n` descriptors (8 words each, word 7 = sender rank; segments "/povu.<job_tag>.<rank>.<k>"
 * are mapped read-only and stay mapped in `ctx`) and of its own forest `own` (taken over, may be NULL; the descriptor
 * with rank `own_rank` is skipped).  The other ranks' arrays stay THEIR memory: the merged forest is valid until the
 * sender frees the forest it described -- in a collective loop, until the sender's next gather. */
povu_hip_forest *povu_hip_forest_attach(povu_hip_ctx *ctx, povu_hip_forest *own, uint32_t own_rank, const char *job_tag,
					const uint64_t *descs, uint32_t n, char *err, size_t errlen);
/* bytes this context has moved since it was created: [0] host to device, [1] device to host (copies and results kernels
 * write straight into page-locked memory), [2] sent to / [3] received from other GPUs (xGMI) */
int povu_hip_transfer_bytes(const povu_hip_ctx *ctx, uint64_t out[4]);

/* ---- one process, N GPUs (`povu decompose --gpus N`) ----
 * The multi-threaded form of do_decompose (app/subcommand/decompose.cpp:116-157: every worker owns its components from
 * graph to file) with GPUs for workers: one context and one host thread per device.  The root device labels the
 * components, bin-packs them (LPT) and partitions the links; the shards travel over xGMI (RCCL ncclSend / ncclRecv, one
 * communicator per device); every GPU decomposes its shard and copies its PVST block into page-locked host memory over
 * ITS OWN PCIe link -- the one address space makes that the gather; nothing returns through the root's link. */
typedef struct povu_hip_multi povu_hip_multi;
/* devices[n]: HIP device of every rank (rank 0 = root).  The same device may be named more than once (rehearsal on a
 * one-GPU box: shards are then loaded straight from the partition, no RCCL). */
povu_hip_multi *povu_hip_multi_create(const int *devices, uint32_t n, char *err, size_t errlen);
void povu_hip_multi_destroy(povu_hip_multi *m);
uint32_t povu_hip_multi_world(const povu_hip_multi *m);
/* the whole graph to the root device (povu_hip_graph_upload on the root's graph context) */
int povu_hip_multi_upload(povu_hip_multi *m, uint32_t n_vtx, const uint32_t *vid, uint32_t n_links, const uint32_t *v1,
			  const uint8_t *s1, const uint32_t *v2, const uint8_t *s2, const uint8_t *tips, char *err, size_t errlen);
/* label + LPT + partition on the root, shards to their devices, every rank builds its CSR.  With keep_graph = 0 the
 * root gives the whole graph's memory back first-thing after the partition (a CLI run never needs it again). */
int povu_hip_multi_scatter(povu_hip_multi *m, int keep_graph, char *err, size_t errlen);
/* Every rank decomposes its resident shard on its own thread (flags: POVU_HIP_F_*).  `sink`, when given, runs ON THE
 * WORKER'S THREAD with that rank's forest (global component ids) as soon as it is done -- a CLI formats and writes its
 * files there, like the reference's workers; a non-zero return fails the call.  Returns the merged forest (no array is
 * copied: it takes over every rank's blocks).  With POVU_HIP_F_ASYNC | POVU_HIP_F_NO_STAGE_TIMES in `flags` (and no sink) the
 * call returns while the ranks' PVST arrays are still on their way to the host -- the merged forest waits for them like any
 * POVU_HIP_F_ASYNC forest -- and the next call's kernels run under those copies. */
typedef int (*povu_hip_multi_sink)(uint32_t rank, const povu_hip_forest *f, void *user);
povu_hip_forest *povu_hip_multi_decompose(povu_hip_multi *m, uint32_t flags, povu_hip_multi_sink sink, void *user, char *err,
					  size_t errlen);
typedef struct {
	int device;
	uint32_t n_vtx, n_links, n_components; /* of the rank's shard */
	uint64_t shard_bytes;
	double recv_ms, csr_ms;		 /* last scatter: until the shard was there; CSR build */
	double decompose_ms, sink_ms;	 /* last decompose */
	uint64_t h2d, d2h, peer_out, peer_in; /* povu_hip_transfer_bytes of the rank's context */
} povu_hip_multi_rank_info;
int povu_hip_multi_rank(const povu_hip_multi *m, uint32_t rank, povu_hip_multi_rank_info *out);
/* [0] label, [1] weights + LPT, [2] partition kernels (device time on the root), [3] wall of the last scatter, [4] wall of
 * the last decompose (slowest rank + merge), [5] merge alone */
int povu_hip_multi_times(const povu_hip_multi *m, double out_ms[6]);
/* "none" (one rank), "rccl", "peer-copy" (hipMemcpyPeerAsync; also the fallback when RCCL cannot be initialised: the
 * reason is appended) or "same-device" */
const char *povu_hip_multi_transport(const povu_hip_multi *m);
/* the context of worker `rank` (NULL when out of range): for the debug exports of the pass povu_hip_multi_decompose just ran --
 * call them from the sink callback (it runs on the worker's own thread, the only one that may use the context then) */
povu_hip_ctx *povu_hip_multi_context(povu_hip_multi *m, uint32_t rank);
/* a context that holds a shard: ids[k] = id (1-based, of the whole graph) of the shard's k-th component, the rank the debug
 * exports and the sidecar of --structure-export address a component by.  0 on success, 1 when the resident graph is no shard. */
int povu_hip_shard_component_ids(const povu_hip_ctx *ctx, const uint32_t **ids, uint32_t *n);

/* Completes a forest of a POVU_HIP_F_ASYNC decompose (no-op otherwise): returns when its arrays are in host memory. */
int povu_hip_forest_wait(povu_hip_forest *f);
/* HIP-event time of the pass that produced `f`, from its first kernel to the last byte in host memory, milliseconds
 * (waits for the forest first; < 0 when the forest carries none: merged forests, empty shards) */
double povu_hip_forest_pass_ms(povu_hip_forest *f);
/* HIP-event time from the first kernel of the pass behind `first` to the last byte of the pass behind `last` (both of one
 * context): what a run of overlapped passes took on the device */
double povu_hip_forest_span_ms(povu_hip_forest *first, povu_hip_forest *last);

/* components of the WHOLE graph (all shards), including skipped ones */
uint32_t povu_hip_forest_total_components(const povu_hip_forest *f);
/* PVSTs held by this forest (this shard's components with >= 3 vertices) */
uint32_t povu_hip_forest_tree_count(const povu_hip_forest *f);

typedef struct {
	uint32_t component_id; /* 1-based, file name <id>.pvst */
	uint32_t n_vtx, n_links;
	uint32_t n_pvst; /* PVST vertices incl. the dummy root 0 */
	/* arrays of n_pvst entries, PVST vertex idx = emission order; entry 0 = dummy root */
	const uint32_t *a_id, *z_id;   /* flubble endpoints (segment ids) */
	const uint8_t *a_or, *z_or;    /* 0 forward '>', 1 reverse '<' */
	const uint32_t *parent;	       /* PVST parent idx, POVU_HIP_NIL for the root */
	uint32_t n_hairpins;	       /* with POVU_HIP_F_HAIRPINS */
	const uint64_t *hairpins;      /* pairs (b1,b2) */
} povu_hip_tree;

int povu_hip_forest_get(const povu_hip_forest *f, uint32_t i, povu_hip_tree *out);
/* With POVU_HIP_F_LEAF_SUBFLUBBLES: per PVST vertex of tree i (n_pvst entries, entry 0 = dummy root) the spanning-tree
 * vertices ai / zi that pvst::Flubble::create takes (compute_ai_zi, flubbles.cpp:264-290; POVU_HIP_NIL for the root) and
 * the line letter 'D' 'F' 'T' (tiny) 'O' (parallel).  Any of the three pointers may be NULL.  Returns 3 when the
 * forest carries none. */
int povu_hip_forest_get_sub(const povu_hip_forest *f, uint32_t i, const uint32_t **ai, const uint32_t **zi, const uint8_t **fam);
/* With POVU_HIP_F_SUBFLUBBLES: tree i after all five passes of -s (pvst::Tree of include/povu/graph/pvst.hpp:719-900 as
 * write_pvst sees it).  Vertices [0, n_flubble_like) are those of povu_hip_forest_get, relabelled; the inserted ones follow
 * in the order the reference adds them (concealed, midi, smothered).  Per vertex: the line letter ('D' 'F' 'T' 'O' 'C' 'M'
 * 'S'), the two boundaries in the order as_str() prints them (orientation 0 = '>'), the route letter ('L' 'R', 0 = none) and
 * its children, in the reference's order: child[child_off[v] .. child_off[v + 1]).  Returns 3 when the forest carries none. */
typedef struct {
	uint32_t n_total, n_flubble_like, n_concealed, n_midi, n_smothered;
	const uint8_t *fam, *or1, *or2, *route;
	const uint32_t *id1, *id2;
	const uint32_t *child_off; /* [n_total + 1], offsets into `child` */
	const uint32_t *child;
} povu_hip_subtree;
int povu_hip_forest_get_subtree(const povu_hip_forest *f, uint32_t i, povu_hip_subtree *out);
/* write_pvst (src/mto/to_pvst.cpp:31-109) of such a tree; malloc'd, free with povu_hip_buffer_free */
char *povu_hip_pvst_format_subtree(const povu_hip_subtree *t, size_t *len);
/*
 * The forest's arrays as ONE page-locked host block (what a multi-GPU gather ships):
 * offsets[0..4] = byte offsets of a_id, z_id, parent (u32 x total) and a_or, z_or (u8 x total);
 * tree i occupies entries [first[i], first[i] + n_pvst) of every array (first = povu_hip_forest_first).
 */
int povu_hip_forest_raw(const povu_hip_forest *f, const void **block, size_t *bytes, uint64_t *total, uint64_t offsets[5]);
uint64_t povu_hip_forest_first(const povu_hip_forest *f, uint32_t i);
void povu_hip_forest_free(povu_hip_forest *f);

/* ---- walks of every flubble ("Flubble walks": decided here, not reference behaviour) ----
 * A step is (segment, orientation); (v, '>') leaves v through its r side, (v, '<') through its l side, and a link from that
 * side to side y of u gives the next step (u, '>') when y is l, (u, '<') when y is r (parallel links count once).  Every PVST
 * vertex but the root of its tree is one query: from its first boundary step S to its second boundary step Z (for a forest
 * of POVU_HIP_F_SUBFLUBBLES the vertices of the extended trees, povu_hip_forest_get_subtree).  A walk starts with S, ends
 * with Z and holds no segment twice; walks come in lexicographic order of their (segment id, '>' before '<') keys -- the
 * order of a DFS that tries successors by ascending id, '>' first.  That DFS counts one expansion per step it appends to a
 * prefix (Z included, S not); a prefix of max_steps steps that does not end at Z is not extended (status LONG); it stops
 * at the (max_walks + 1)-th walk (MORE: the first max_walks are reported) or when an expansion beyond max_expansions would
 * be needed (BUDGET: the walks found so far are reported).  Queries are numbered in tree order, then PVST vertex order
 * within the tree, each root skipped. */
typedef struct {
	uint32_t max_walks;	 /* K, 0 = 64 */
	uint32_t max_steps;	 /* L, 0 = 1000 (the reference's MAX_FLUBBLE_STEPS) */
	uint32_t max_expansions; /* E, 0 = 65536 */
	uint32_t flags;		 /* POVU_HIP_W_* */
} povu_hip_walk_opts;
#define POVU_HIP_W_FORCE_TIER2 1u /* run every query with the second-tier kernel (tests) */
#define POVU_HIP_WALK_MORE 1u	  /* status bits per query */
#define POVU_HIP_WALK_LONG 2u
#define POVU_HIP_WALK_BUDGET 4u
typedef struct {
	uint64_t n_queries, n_walks, n_steps;
	const uint32_t *walk_off; /* [n_queries + 1] walks of query q: [walk_off[q], walk_off[q + 1]) */
	const uint32_t *step_off; /* [n_walks + 1] steps of walk w: [step_off[w], step_off[w + 1]) */
	const uint32_t *step_id;  /* [n_steps] segment id */
	const uint8_t *step_or;	  /* [n_steps] 0 '>', 1 '<' */
	const uint8_t *status;	  /* [n_queries] POVU_HIP_WALK_* bits */
	uint64_t n_tier2;	  /* queries the second-tier kernel ran (the first tier hands over what outgrows its limits) */
	double device_ms;	  /* HIP-event time of the call, first upload to last byte on the host */
} povu_hip_walks;
/* Enumerates the walks of every query of `f` on the graph resident in `ctx` (opts NULL = defaults).  Refused with a
 * message when `f` was not made by povu_hip_decompose on this context from its current upload, when it is sharded, merged
 * or attached, when the segment ids of the resident graph do not ascend with the vertex index, or when the output does
 * not fit (32-bit offsets, device memory).  Free with povu_hip_walks_free. */
povu_hip_walks *povu_hip_forest_walks(povu_hip_ctx *ctx, povu_hip_forest *f, const povu_hip_walk_opts *opts, char *err,
				      size_t errlen);
void povu_hip_walks_free(povu_hip_walks *w);

/* ---- traversals of every flubble by the paths of the graph ("Flubble traversals": decided here, not
 * reference behaviour) ----
 * Makes `n_paths` paths resident beside the graph now uploaded: the steps of path k are [step_off[k], step_off[k + 1]),
 * step_id the segment id, step_rev 0 for '>' (GFA '+'), 1 for '<'.  The paths belong to this upload: the next
 * povu_hip_graph_upload drops them.  Refused when no graph is resident, when its segment ids do not ascend with the vertex
 * index, when a step names an id the graph does not have (the message names the path and the step), when a path has 2^32
 * steps or more, or when device memory runs out.  0 on success */
int povu_hip_paths_upload(povu_hip_ctx *ctx, uint32_t n_paths, const uint64_t *step_off, const uint32_t *step_id,
			  const uint8_t *step_rev, char *err, size_t errlen);
/* The queries are those of povu_hip_forest_walks.  Every occurrence of S in a path starts a forward scan and every occurrence
 * of flip(Z) a reverse scan; a scan ends at the next step on either boundary segment and is a traversal when that step is Z
 * (flip(S)) within max_steps steps.  The alleles of a query are the distinct S -> Z step sequences of its traversals,
 * numbered in the order of their first traversal; traversals come in (path, first step) order. */
typedef struct {
	uint32_t max_steps; /* 0 = 65 536; else at least 2 */
	uint32_t flags;	    /* POVU_HIP_T_* */
} povu_hip_trav_opts;
#define POVU_HIP_T_FORCE_TIER2 1u /* run every scan with the wave-per-scan kernel (tests) */
#define POVU_HIP_T_INVERSIONS 2u  /* povu_hip_call only: SUBR records too ("Inversion calls"); ignored elsewhere */
#define POVU_HIP_T_NESTED 4u	  /* povu_hip_call only: alleles modulo enclosed sites, levels and parents by geometry ("Nested calls") */
#define POVU_HIP_T_MERGE 8u	  /* povu_hip_call_profile under POVU_HIP_PROFILE_DECOMPOSED only: equal primitives merged ("Merged primitives") */
#define POVU_HIP_T_OFFREF 16u	  /* povu_hip_call / _call_profile only: sites no reference path crosses, on a surrogate path ("Off-reference calls") */
#define POVU_HIP_T_UNTANGLE 32u	  /* povu_hip_call / _call_profile only: per-copy genotypes where a path laps a site, by lap alignment ("Untangled calls") */
/* povu_hip_call and its kin, with POVU_HIP_T_NESTED or a profile that implies it only: a `*` ALT where an enclosing allele deletes
 * the site ("Spanning alleles").  Refused without a nested call and under the left-normalized and decomposed profiles */
#define POVU_HIP_T_SPANNING 64u
#define POVU_HIP_TRAV_LONG 1u	  /* status bits per query: a scan would need more than max_steps steps */
#define POVU_HIP_TRAV_STRAY 2u	  /* a scan met a boundary step that does not close it */
#define POVU_HIP_TRAV_OPEN 4u	  /* a scan reached the end of its path */
typedef struct {
	uint64_t n_queries, n_traversals, n_alleles, n_steps;
	const uint64_t *trav_off;   /* [n_queries + 1] traversals of query q: [trav_off[q], trav_off[q + 1]) */
	const uint64_t *allele_off; /* [n_queries + 1] alleles of query q: [allele_off[q], allele_off[q + 1]) */
	const uint8_t *status;	    /* [n_queries] POVU_HIP_TRAV_* bits */
	const uint32_t *path;	    /* [n_traversals] path index (upload order) */
	const uint32_t *first;	    /* [n_traversals] step of the path where the traversal begins (S, or flip(Z) when reverse) */
	const uint32_t *last;	    /* [n_traversals] step of the path where it ends */
	const uint32_t *allele;	    /* [n_traversals] allele number within its query */
	const uint8_t *reverse;	    /* [n_traversals] 1: the path reads the flubble from Z to S */
	const uint64_t *step_off;   /* [n_alleles + 1] steps of allele a: [step_off[a], step_off[a + 1]) */
	const uint32_t *step_id;    /* [n_steps] segment id, S -> Z */
	const uint8_t *step_or;	    /* [n_steps] 0 '>', 1 '<' */
	uint64_t n_tier2;	    /* scans the wave-per-scan kernel ran */
	uint64_t n_hash_splits;	    /* alleles split off a group of equal (length, hash) by the exact comparison */
	double device_ms;	    /* HIP-event time of the call, first upload to last byte on the host */
} povu_hip_traversals;
/* Traversals of every query of `f` by the paths resident in `ctx` (opts NULL = defaults).  Refused like
 * povu_hip_forest_walks (forest not made from this context's current upload; sharded, merged or attached forest; ids not
 * ascending), when no paths are resident, and when the scan tasks, traversals or allele steps reach 2^32 (the scans are
 * 32-bit) or do not fit device memory.  Free with povu_hip_traversals_free. */
povu_hip_traversals *povu_hip_forest_traversals(povu_hip_ctx *ctx, povu_hip_forest *f, const povu_hip_trav_opts *opts, char *err,
						size_t errlen);
void povu_hip_traversals_free(povu_hip_traversals *t);

/* ---- variant calls ("Variant calls": decided here, not reference behaviour) ----
 * Makes the sequences of the graph now uploaded resident beside it: segment of vertex index v (ascending segment id) has
 * the bytes seq[seq_off[v] .. seq_off[v + 1]).  The next povu_hip_graph_upload drops them.  Refused when `n_vtx` is not the
 * resident graph's vertex count or the offsets decrease.  0 on success */
int povu_hip_segments_upload(povu_hip_ctx *ctx, uint32_t n_vtx, const uint64_t *seq_off, const char *seq, char *err, size_t errlen);
/* the PVST vertices to call, one query each, in tree order then vertex order (the queries of povu_hip_forest_walks) */
typedef struct {
	uint32_t n;
	const uint32_t *id1, *id2; /* boundary segment ids */
	const uint8_t *or1, *or2;  /* 0 '>', 1 '<' */
	const uint32_t *parent;	   /* query of the parent vertex, POVU_HIP_NIL for a child of the root */
	const uint32_t *height;	   /* PVST height, the root's children 1 (LV = height - 1) */
	const uint8_t *family;	   /* line letter: 'F', or 'T' 'O' 'C' 'M' 'S' (a subflubble: skipped with its subtree) */
	const uint32_t *tree;	   /* tree of the vertex (presence of the reference paths is per tree) */
} povu_hip_sites;
/* the reference paths (ascending path indices) and the genotype slots: slot of every resident path, sample of every slot
 * (slots of a sample are consecutive) */
typedef struct {
	uint32_t n_refs;
	const uint32_t *ref_path;
	uint32_t n_slots, n_samples;
	const uint32_t *sample_of_slot;
} povu_hip_call_refs;
#define POVU_HIP_CALL_ANCHORED 1u /* record flags */
#define POVU_HIP_CALL_TANGLED 2u
#define POVU_HIP_CALL_INS 4u
#define POVU_HIP_CALL_DEL 8u /* neither INS nor DEL: SUB */
/* an inversion record (POVU_HIP_T_INVERSIONS): query = POVU_HIP_NIL, first = the step of `path` where the inverted run
 * begins, n_steps its steps, ref_allele 0, n_alleles 2, one AC; its block holds REF (the run's bases) and then ALT (their
 * reverse complement), the AT strings every step of the run and the flipped steps backwards */
#define POVU_HIP_CALL_SUBR 16u
/* with POVU_HIP_T_NESTED: the site has fewer classes than exact alleles (the record hides enclosed variation; TANGLED too) /
 * the `popped` profile kept the record although its level is above max_level, because its ancestors were popped */
#define POVU_HIP_CALL_COLLAPSED 32u
#define POVU_HIP_CALL_RESCUED 64u
/* under POVU_HIP_PROFILE_LEFT_NORMALIZED: the record was changed by the left-normalisation (pos is the normalised POS, its
 * normalised alleles are those of block norm_block) */
#define POVU_HIP_CALL_NORMALIZED 128u
#define POVU_HIP_GT_MISSING 0xFFFFu
typedef struct {
	uint64_t n_records, n_slots, n_blocks, n_spelled, n_seq_bytes, n_at_bytes, n_refs;
	/* per record, in (reference path, POS, query) order */
	const uint32_t *query, *path, *first, *ref_allele, *n_alleles, *an, *ns, *block;
	const uint64_t *pos;
	const uint8_t *flags;	 /* POVU_HIP_CALL_* */
	const uint64_t *ac_off;	 /* [n_records + 1] AC of ALT i (1-based) of record r: ac[ac_off[r] + i - 1] */
	const uint32_t *ac;
	const uint16_t *gt;	 /* [n_records * n_slots] allele in record numbering (REF 0), POVU_HIP_GT_MISSING for '.' */
	/* the alleles of a query spelled in one orientation ("block", the query and the orientation its records need): allele
	 * a of the block's query is spelled allele block_off[b] + a */
	const uint64_t *block_off; /* [n_blocks + 1] */
	const uint64_t *seq_off, *at_off; /* [n_spelled + 1] byte offsets into seq / at */
	const char *seq, *at;	   /* the bases (anchor base first when anchored) and the AT step strings ('>id<id...') */
	const uint64_t *contig_len; /* [n_refs] bases of every reference path */
	double device_ms;
	/* with POVU_HIP_T_INVERSIONS (else n_steps all 0 and the counters 0) */
	const uint32_t *n_steps; /* [n_records] steps of an inversion record's run, 0 for a flubble record */
	uint64_t n_inv_records;	 /* records with POVU_HIP_CALL_SUBR */
	uint64_t n_inv_heads;	 /* run heads found */
	uint64_t n_inv_long;	 /* runs of more than max_steps steps (dropped) */
	uint64_t n_inv_tier2;	 /* runs the wave-per-run kernel extended (longer than 64 steps, or all with _T_FORCE_TIER2) */
	/* per record.  Without POVU_HIP_T_NESTED: level = the site's height - 1, parent_query = POVU_HIP_NIL, ref_spelled =
	 * block_off[block] + ref_allele and the counters 0.  With it ("Nested calls") ref_allele, n_alleles, gt and ac count
	 * classes, a block holds one spelled allele per class (its representative) and REF is spelled allele ref_spelled: the
	 * block's, or one of its own behind the flubble blocks when the reference's exact allele is not the representative */
	const uint32_t *level;	      /* [n_records] LV; 0 for an inversion record */
	const uint32_t *parent_query; /* [n_records] site of the enclosing record (PS), POVU_HIP_NIL: none */
	const uint64_t *ref_spelled;  /* [n_records] */
	uint64_t n_enclosed;	      /* records with a parent (before the profile drops any) */
	uint64_t n_collapsed_sites;   /* called sites of two classes or more that have fewer classes than exact alleles */
	uint64_t n_popped;	      /* `popped` profile: records reached and dropped as big */
	uint64_t n_rescued;	      /* `popped` profile: records kept above max_level (POVU_HIP_CALL_RESCUED) */
	uint64_t nested;	      /* 1: made with POVU_HIP_T_NESTED (the VCF carries PS) */
	/* per record ("Left-normalised calls").  Outside POVU_HIP_PROFILE_LEFT_NORMALIZED, and for a record it left unchanged:
	 * raw_pos = pos, norm_block = POVU_HIP_NIL, the others 0.  A changed record (POVU_HIP_CALL_NORMALIZED) keeps block and
	 * ref_spelled (its raw alleles and every AT string) and has a block norm_block of n_alleles spelled alleles of its own,
	 * REF first and the ALTs in the order they are written, that hold the normalised texts (their AT strings are empty) */
	const uint64_t *raw_pos;	     /* [n_records] POS before the normalisation */
	const uint32_t *norm_block;	     /* [n_records] */
	const uint32_t *norm_shift, *norm_chop, *norm_trim; /* [n_records] s, r and u of the closed form */
	uint64_t n_normalized;		     /* records with POVU_HIP_CALL_NORMALIZED */
	uint64_t max_shift;		     /* the largest norm_shift */
	uint64_t n_norm_compared;	     /* bases the backward walks compared, over every (record, ALT) */
	/* per row ("Decomposed calls"), in (reference path, row POS, record, ALT, alignment order).  Outside
	 * POVU_HIP_PROFILE_DECOMPOSED: n_rows 0, the arrays NULL, the counters 0.  A row is one primitive of the alignment of
	 * its record's REF and ALT row_alt, or that ALT kept whole; the record arrays above stay the raw call's.  The row's REF
	 * is row_lead (when not 0) and then bytes [row_ref_start, row_ref_start + row_ref_len) of the record's REF text, its
	 * ALT row_lead and then bytes [row_alt_start, row_alt_start + row_alt_len) of that ALT's text */
	uint64_t n_rows;
	const uint32_t *row_record; /* [n_rows] record of the row */
	const uint32_t *row_alt;    /* [n_rows] its ALT, 1-based */
	const uint8_t *row_kind;    /* [n_rows] POVU_HIP_ROW_* */
	const uint8_t *row_reason;  /* [n_rows] POVU_HIP_REASON_* of a _ROW_PASS row, else 0 */
	const uint32_t *row_index;  /* [n_rows] k of snp<k>, ins<k>, del<k>: counts within the kind and the ALT from 1; else 0 */
	const uint64_t *row_pos;    /* [n_rows] POS */
	const uint32_t *row_ref_start, *row_ref_len, *row_alt_start, *row_alt_len;
	const uint8_t *row_lead;    /* [n_rows] 0, or the anchor base of an indel written in front of both: the REF base in
				     * front of it, the reference path's base in front of POS for an indel at offset 0 */
	const uint32_t *row_ac, *row_an, *row_ns; /* [n_rows] counted on the projected genotypes (0 stays, row_alt is 1, else missing) */
	uint64_t n_decomposed_alts;  /* (record, ALT) written as primitives */
	uint64_t n_passthrough_alts; /* (record, ALT) kept whole (_ROW_PASS); a _ROW_RAW row counts as neither */
	uint64_t n_prim_tier2;	     /* pairs the striped kernel aligned (a text longer than 64 bytes, or all with _T_FORCE_TIER2) */
	uint64_t n_prim_cells;	     /* sum of (len REF + 1) * (len ALT + 1) over the aligned pairs */
	/* per merged row ("Merged primitives"), in the order of their first members among the rows.  Without POVU_HIP_T_MERGE:
	 * merged 0, n_mrows 0, the arrays NULL, the counters 0.  A merged row is a group of rows that are the same primitive
	 * (reference path, POS and both written texts after upper-casing; a _ROW_PASS row is a group of its own); its first
	 * member is its representative.  The row arrays above are those of the call without the flag */
	uint64_t merged;	     /* 1: made with POVU_HIP_T_MERGE (the VCF is written from the merged rows) */
	uint64_t n_mrows;
	const uint64_t *mrow_off;    /* [n_mrows + 1] members of merged row g: mrow_member[mrow_off[g] .. mrow_off[g + 1]) */
	const uint32_t *mrow_member; /* [n_rows] row indices, the members of a group in row order */
	const uint8_t *mrow_gt;	     /* [n_mrows * n_slots] the joint genotype of every slot: 0, 1, or 0xFF for '.' */
	const uint32_t *mrow_ac, *mrow_an, *mrow_ns; /* [n_mrows] counted on mrow_gt */
	uint64_t n_merged_groups;    /* groups of two members or more */
	uint64_t n_merged_members;   /* rows in those groups */
	uint64_t n_merge_splits;     /* groups split off a run of equal (POS, lengths, hash) by the exact comparison */
	uint64_t n_ref_consistent;   /* (group, slot) entries that are 0 only because the slot's own ALT lies outside the group's span */
	uint64_t n_gt_conflicts;     /* (group, slot) entries with a vote for 1 and a vote for 0 (written 1) */
	/* with POVU_HIP_T_OFFREF ("Off-reference calls").  Without the flag: offref 0, the counts 0, the arrays NULL.  A site that
	 * is not callable, lies under no subflubble and has a traversal is a candidate; one with no callable or candidate child is
	 * called off-reference on its surrogate, the path of its first traversal, whose traversals give its records: `path` is
	 * then the surrogate, `pos` counts along it.  The host of such a record is the tightest traversal by the same path of a
	 * site the reference paths call (two alleles or more) that strictly encloses it */
	uint64_t offref;	      /* 1: made with POVU_HIP_T_OFFREF */
	const uint8_t *rec_offref;    /* [n_records] 1: an off-reference record */
	const uint32_t *host_query;   /* [n_records] site of the host, POVU_HIP_NIL: none */
	const uint32_t *host_allele;  /* [n_records] exact allele of the host traversal within its site, POVU_HIP_NIL: none */
	uint64_t n_off_contigs;	      /* surrogate paths that are no reference path and carry a record */
	const uint32_t *off_contig_path; /* [n_off_contigs] ascending */
	const uint64_t *off_contig_len;	 /* [n_off_contigs] bases of the path */
	uint64_t n_offref_sites;      /* sites called off-reference with two alleles or more */
	uint64_t n_offref_records;
	uint64_t n_offref_hosted;     /* off-reference records with a host */
	/* with POVU_HIP_T_UNTANGLE ("Untangled calls").  Without the flag: untangled 0, the counts 0, the arrays NULL.  The laps of
	 * a path through a site are its traversals of it in path order.  Where the reference path and the one path of a slot both
	 * lap a site in one direction each, at most 64 times, the slot's laps are aligned with the reference's (unit cost, the tie
	 * rule of "Decomposed calls") and the record of reference lap j takes the slot's allele from the lap aligned with j ('.'
	 * when none is); every other entry keeps the rule of "Variant calls".  Inversion records: 0 everywhere */
	uint64_t untangled;	      /* 1: made with POVU_HIP_T_UNTANGLE */
	const uint8_t *rec_unt;	      /* [n_records] 1: some entry of the record was aligned in a table of two laps or more (written with LN, LC, GT:CN) */
	const uint32_t *lap;	      /* [n_records] lap of the reference path the record is, from 1 */
	const uint32_t *n_laps;	      /* [n_records] laps of the reference path through the site */
	const uint16_t *lap_count;    /* [n_records * n_slots] traversals of the site by the slot's paths, saturating at 65 535 */
	uint64_t n_unt_tasks;	      /* alignments run: distinct (site, reference path, path) with two laps or more on a side */
	uint64_t n_unt_records;	      /* records with rec_unt */
	uint64_t n_unt_missing;	      /* reference laps without a partner, over the alignments */
	uint64_t n_unt_extra;	      /* laps of the other path without a partner, over the alignments */
	uint64_t n_unt_fallback;      /* (record, slot) entries of two traversals or more that were left to the rule of "Variant calls" */
	/* of povu_hip_call_restricted with regions ("Region calls").  Without regions: 0 */
	uint64_t n_regions;	      /* intervals after normalisation (per path sorted, overlapping and touching ones merged) */
	uint64_t n_region_sites;      /* sites that pass: their S or Z segment is marked */
	uint64_t n_region_masked;     /* sites whose scans were masked: n_sites - n_region_sites, 0 where masking is not allowed */
	uint64_t n_region_dropped;    /* flubble records the late filter dropped (0 under masking) */
	/* of povu_hip_call_clustered with a threshold ("Clustered calls").  Without one: cluster_ppm 0, the arrays NULL, the counts
	 * 0.  With one ref_allele, n_alleles, gt and ac count clusters of exact alleles, a block holds one spelled allele per cluster
	 * (its representative) and REF is spelled allele ref_spelled, as in a nested call */
	uint64_t cluster_ppm;	      /* the threshold T = F * 10^6 the call was made with */
	const uint8_t *rec_clustered; /* [n_records] 1: the record's site has fewer clusters than exact alleles (written with NX, MINSIM) */
	const uint32_t *cl_minsim;    /* [n_records] the lowest sim_ppm of any member of any of the site's clusters to its representative */
	const uint32_t *cl_nx;	      /* [ac_off[n_records] + n_records] exact alleles behind written allele i (0: REF) of record r: cl_nx[ac_off[r] + r + i] */
	uint64_t n_cluster_sites;     /* called sites of two exact alleles or more: the sites that were clustered */
	uint64_t n_clustered_sites;   /* ... left with two clusters or more and fewer clusters than exact alleles */
	uint64_t n_cluster_vanished;  /* ... left with one cluster: they give no record */
	uint64_t n_cluster_keys;      /* inner steps of the exact alleles of those sites: the keys of the bags */
	uint64_t n_cluster_pairs;     /* (exact allele, representative) pairs the leader loops met */
	uint64_t n_cluster_pruned;    /* ... of which the weight bound skipped (0 with POVU_HIP_CLUSTER_NO_BOUND) */
	uint64_t n_cluster_tier2;     /* bags the device-wide sort sorted (more than 64 keys, or all with _T_FORCE_TIER2) */
	/* with POVU_HIP_T_SPANNING ("Spanning alleles").  Without the flag: spanning 0, rec_star NULL, the counts 0.  An entry
	 * (record, slot) is spanned when no path of the slot traverses the record's site, the site's search was not cut short and a
	 * path of the slot traverses the site of some enclosing record (the chain of parent_query, taken before the profile drops
	 * any).  A record with a spanned entry has one more ALT, its last, written `*`: n_alleles counts it, ac has an entry for it,
	 * the spanned entries of gt carry its number n_alleles - 1, an and ns count them.  It has no spelled allele: the block of the
	 * record holds n_alleles - 1 alleles */
	uint64_t spanning;	      /* 1: made with POVU_HIP_T_SPANNING */
	const uint8_t *rec_star;      /* [n_records] 1: the record's last ALT is `*` */
	uint64_t n_star_records;      /* records with rec_star */
	uint64_t n_star_entries;      /* spanned (record, slot) entries of those records */
} povu_hip_calls;
/* The calls of `sites` by the reference paths `refs` among the paths resident in `ctx` (sequences resident too).  opts as
 * for povu_hip_forest_traversals (NULL = defaults).  Refused like the traversals, when no sequences are resident, when a
 * site's boundary is no segment of the graph, for a query of more than 65 534 alleles in a called site, 2^32 records or
 * more, a spelled byte that is no nucleotide code (the message names the segment), and output beyond device memory.  With
 * POVU_HIP_T_INVERSIONS in opts->flags the inversion records of the reference paths against every other resident path are
 * merged in ((reference path, POS, query, first, n_steps) order; `sites` may be empty); refused then too for 2^32 path
 * steps or run heads or more.  With POVU_HIP_T_OFFREF the off-reference records are added (the record order becomes (path,
 * POS, query, first); inversion records stay those of the reference paths); the flag is refused together with
 * POVU_HIP_T_NESTED, POVU_HIP_T_MERGE or any profile other than _RAW_GRAPH.  With POVU_HIP_T_UNTANGLE the rows of the sites
 * a path laps are rewritten from lap alignments (the records and their order stay); refused together with POVU_HIP_T_NESTED,
 * POVU_HIP_T_MERGE, POVU_HIP_T_OFFREF or any profile other than _RAW_GRAPH, for 2^32 (reference run, slot) entries or more and
 * for a partner table beyond device memory.  Free with povu_hip_calls_free. */
povu_hip_calls *povu_hip_call(povu_hip_ctx *ctx, const povu_hip_sites *sites, const povu_hip_call_refs *refs,
			      const uint32_t *slot_of_path, const povu_hip_trav_opts *opts, char *err, size_t errlen);
/* The profiles of a nested call ("Nested calls"): what is kept of the flubble records, decided on the device before any
 * allele is spelled (inversion records are always kept).  A length of 0 is no limit.  A record is big when its REF is
 * longer than max_ref_length or any allele it writes is longer than max_allele_length.  _TOP_LEVEL_ONLY keeps level 0;
 * _POPPED keeps the records that are reached (level <= max_level, or the parent is big and reached) and not big. */
#define POVU_HIP_PROFILE_RAW_GRAPH 0u
#define POVU_HIP_PROFILE_TOP_LEVEL_ONLY 1u
#define POVU_HIP_PROFILE_POPPED 2u
/* "Left-normalised calls": every record is kept, an indel is moved to the left end of its repeat and common bases are
 * chopped and trimmed.  Does not imply POVU_HIP_T_NESTED (may be combined with it and with _T_INVERSIONS); max_level and the
 * lengths are ignored */
#define POVU_HIP_PROFILE_LEFT_NORMALIZED 3u
/* "Decomposed calls": every record is kept and every (REF, ALT) of a flubble record is aligned (unit-cost edit distance, gaps
 * as far left as the optimum allows) and written as its primitives, one row each (povu_hip_calls.n_rows, row_*).  Does not
 * imply POVU_HIP_T_NESTED (may be combined with it and with _T_INVERSIONS); max_level and max_ref_length are ignored,
 * max_allele_length is the longest text that is aligned: 0 means POVU_HIP_PRIM_MAX_LENGTH, more than that is refused.  With
 * POVU_HIP_T_MERGE in opts->flags equal primitives of different ALTs and records are merged into one row with joint genotypes
 * (povu_hip_calls.n_mrows, mrow_*; refused for 2^32 (group, slot) entries or more); the flag with any other profile is refused */
#define POVU_HIP_PROFILE_DECOMPOSED 4u
#define POVU_HIP_PRIM_MAX_LENGTH 512u
#define POVU_HIP_ROW_RAW 0u /* the record as the raw call writes it: its one ALT is one primitive that spells POS, REF and ALT */
#define POVU_HIP_ROW_SNP 1u
#define POVU_HIP_ROW_INS 2u
#define POVU_HIP_ROW_DEL 3u
#define POVU_HIP_ROW_PASS 4u /* the ALT kept whole */
#define POVU_HIP_REASON_NONE 0u
#define POVU_HIP_REASON_MAX_ALLELE_LENGTH 1u /* a text is longer than the cap */
#define POVU_HIP_REASON_CONTIG_START 2u	     /* an indel at offset 0 of a record at POS 1: no base to anchor it on */
#define POVU_HIP_REASON_EMPTY_ALLELE 3u
#define POVU_HIP_REASON_EQUALS_REF 4u /* the texts are equal after upper-casing */
#define POVU_HIP_REASON_SUBR 5u	      /* an inversion record: passes through whole */
typedef struct {
	uint32_t profile; /* POVU_HIP_PROFILE_* */
	uint32_t max_level;
	uint64_t max_ref_length, max_allele_length;
} povu_hip_call_profile_opts;
/* povu_hip_call under a profile (NULL: povu_hip_call itself).  _TOP_LEVEL_ONLY and _POPPED imply POVU_HIP_T_NESTED; an unknown
 * profile is refused */
povu_hip_calls *povu_hip_call_profile(povu_hip_ctx *ctx, const povu_hip_sites *sites, const povu_hip_call_refs *refs,
				      const uint32_t *slot_of_path, const povu_hip_trav_opts *opts, const povu_hip_call_profile_opts *profile,
				      char *err, size_t errlen);
/* "Region calls": the call restricted to intervals of resident paths.  A region holds the 1-based positions [start, end) of
 * path `path` (any resident path, reference or not); a step of that path is in it when its bases meet the interval (a segment
 * without bases counts as one position); a segment is marked when a step on it is in a region; a site passes when its S or Z
 * segment is marked, an inversion record when the segment of its first or last step is.  The records are exactly those the
 * same call without regions writes for the sites and inversion records that pass, every field the same, in the same order.
 * Where the call is not nested (no POVU_HIP_T_NESTED, no profile that implies it) the sites that do not pass are masked in
 * front of the traversal pipeline and cost no scan; a nested call computes over every site and selects its records at the
 * end.  POVU_HIP_REGION_NO_MASK selects at the end in every call (tests).  Refused: a path index that is no resident path,
 * start >= end, end >= 2^63, more than 65 536 regions, and regions together with POVU_HIP_T_OFFREF. */
typedef struct {
	uint32_t path, reserved;
	uint64_t start, end; /* [start, end), 1-based */
} povu_hip_region;
#define POVU_HIP_REGION_NO_MASK 1u /* tests: scan every site, select records at the end only */
typedef struct {
	uint32_t n, flags;
	const povu_hip_region *region;
} povu_hip_call_regions;
/* povu_hip_call_profile restricted to `regions` (NULL or n == 0: povu_hip_call_profile itself, byte for byte) */
povu_hip_calls *povu_hip_call_restricted(povu_hip_ctx *ctx, const povu_hip_sites *sites, const povu_hip_call_refs *refs,
					 const uint32_t *slot_of_path, const povu_hip_trav_opts *opts, const povu_hip_call_profile_opts *profile,
					 const povu_hip_call_regions *regions, char *err, size_t errlen);
/* `name:start-end` (split at the last ':' and the first '-' behind it, both numbers of digits alone, at most 18; start < end) to
 * a region of the path named exactly `name` among names[0 .. n_paths).  Host only.  0, or 1 and the refusal in err */
int povu_hip_region_parse(const char *text, uint32_t n_paths, const char *const *names, povu_hip_region *out, char *err, size_t errlen);
/* "Clustered calls" (modelled on `vg deconstruct -L`): the exact alleles of a called site whose bags of inner segments are
 * similar (weighted multiset Jaccard I / U >= min_similarity_ppm / 10^6, compared exactly in integers) are one cluster, found by
 * leader clustering in allele order (best fit among the representatives, ties to the lowest cluster), and the records count
 * clusters: ALT i is the representative of cluster i, REF the reference's own exact allele.  Refused together with
 * POVU_HIP_T_NESTED and the profiles that imply it, the left-normalized and decomposed profiles, POVU_HIP_T_MERGE, _T_OFFREF and
 * _T_UNTANGLE, for a threshold above 10^6, and for an allele that walks one segment more than 65 536 times.  Composes with
 * POVU_HIP_T_INVERSIONS and with regions */
typedef struct {
	uint32_t min_similarity_ppm; /* T in 1 .. 10^6; 0: not clustered */
	uint32_t flags;		     /* POVU_HIP_CLUSTER_* */
} povu_hip_call_cluster_opts;
#define POVU_HIP_CLUSTER_NO_BOUND 1u /* tests: no pair of bags is skipped by the weight bound */
/* povu_hip_call_restricted with clusters (cluster NULL or min_similarity_ppm == 0: povu_hip_call_restricted itself, byte for byte) */
povu_hip_calls *povu_hip_call_clustered(povu_hip_ctx *ctx, const povu_hip_sites *sites, const povu_hip_call_refs *refs,
					const uint32_t *slot_of_path, const povu_hip_trav_opts *opts, const povu_hip_call_profile_opts *profile,
					const povu_hip_call_regions *regions, const povu_hip_call_cluster_opts *cluster, char *err, size_t errlen);
/* F as decimal text with at most six decimals, 0 < F <= 1, to *ppm = F * 10^6 exactly.  Host only.  0, or 1 and the refusal in err */
int povu_hip_cluster_parse(const char *text, uint32_t *ppm, char *err, size_t errlen);
void povu_hip_calls_free(povu_hip_calls *c);

/*
 * Serialises tree `i` exactly as mto::to_pvst::write_pvst does
 * (src/mto/to_pvst.cpp:23-109).  Returns a malloc'd buffer (free with
 * povu_hip_buffer_free) and its length.
 */
char *povu_hip_forest_pvst_text(const povu_hip_forest *f, uint32_t i, size_t *len);
/* the same serialiser on caller-provided PVST arrays (host only, no GPU needed); NULL on bad input */
char *povu_hip_pvst_format(uint32_t n_pvst, const uint32_t *a_id, const uint32_t *z_id, const uint8_t *a_or,
			   const uint8_t *z_or, const uint32_t *parent, size_t *len);
/* ... with the line letter of every vertex given ('D' for entry 0, then 'F' / 'T' / 'O'); fam == NULL = all flubbles */
char *povu_hip_pvst_format_fam(uint32_t n_pvst, const uint32_t *a_id, const uint32_t *z_id, const uint8_t *a_or,
			       const uint8_t *z_or, const uint32_t *parent, const uint8_t *fam, size_t *len);
void povu_hip_buffer_free(void *p);

/* ---- PVST reader (host only): mto::from_pvst::read_pvst + pvst::Tree::comp_heights,
 * src/mto/from_pvst.cpp:162-302, include/povu/graph/pvst.hpp:807-836 ---- */
typedef struct {
	uint32_t n;	    /* vertices in file order */
	char *type;	    /* D F T O M C S */
	uint32_t *file_id;  /* second column */
	uint32_t *a_id, *z_id;
	uint8_t *a_or, *z_or;
	uint8_t *route;	    /* 0 = L (start to end), 1 = R */
	uint32_t *parent;   /* idx of the parent vertex, POVU_HIP_NIL for the root */
	uint32_t *height;   /* distance from the root */
} povu_pvst_doc;
povu_pvst_doc *povu_pvst_parse(const char *text, size_t len, char *err, size_t errlen);

/* GFA v1 text of a whole graph in the arrays povu_hip_graph_upload takes (mto::to_gfa::write_gfa's record shapes,
 * src/mto/to_gfa.cpp:13-56): `S <id> A` per segment, `L <a> <+|-> <b> <+|-> 0M` per link, `+` = out of a's r side / into
 * b's l side -- the inverse of the loader contract, so that writing and loading a graph is the identity.  Host only. */
int povu_hip_gfa_write(const char *path, uint32_t n_vtx, const uint32_t *vid, uint32_t n_links, const uint32_t *v1,
		       const uint8_t *s1, const uint32_t *v2, const uint8_t *s2, char *err, size_t errlen);
void povu_pvst_doc_free(povu_pvst_doc *doc);

/* ---- the host half of a call (host only, no GPU needed): what povu_hip_call takes, from names and trees, and what it gives,
 * as VCF text (INTEGRATION.md "Variant calls": reference paths, samples and slots, the VCF) ---- */
/* The reference paths and the PanSN samples and slots of the paths named `path_name`: refs.ref_path the paths whose name
 * starts with one of the prefixes (ascending), a name `sample#hap#rest` with an all-digit hap that sample's slot `hap` (a
 * sample's slots consecutive, ascending by hap), any other name a sample of its own; samples in order of their first path. */
typedef struct {
	povu_hip_call_refs refs;	/* for povu_hip_call */
	uint32_t n_paths;
	const uint32_t *slot_of_path; /* [n_paths] for povu_hip_call */
	const char *const *sample;	/* [refs.n_samples] names, in column order */
	const int64_t *slot_hap;	/* [refs.n_slots] PanSN hap number of the slot, -1 for a name that has none */
} povu_hip_call_names;
/* NULL and a message that lists the prefixes when no name starts with one of them.  Free with _free. */
povu_hip_call_names *povu_hip_call_names_make(uint32_t n_paths, const char *const *path_name, uint32_t n_prefixes,
					      const char *const *prefix, char *err, size_t errlen);
void povu_hip_call_names_free(povu_hip_call_names *n);
/* Appends the sites of tree number `tree` to the owned `s` (of _sites_of_docs / _forest_sites, or zeroed by the caller and freed
 * with _sites_free): n vertices in PVST vertex order, a root (family 'D'; family NULL: entry 0, every other vertex 'F') is
 * skipped and the others numbered on; parent the vertex index (POVU_HIP_NIL or a root: none), height 1 under a root and one
 * more than the parent's elsewhere (0 for a vertex without parent).  0 on success */
int povu_hip_sites_add_tree(povu_hip_sites *s, uint32_t tree, uint32_t n, const uint32_t *id1, const uint32_t *id2,
			    const uint8_t *or1, const uint8_t *or2, const uint32_t *parent, const uint8_t *family);
/* the sites of parsed PVST files in component order (tree k = docs[k]) */
povu_hip_sites *povu_hip_sites_of_docs(const povu_pvst_doc *const *docs, uint32_t n);
/* the sites of a forest: the extended trees of POVU_HIP_F_SUBFLUBBLES when it carries them (parent = the last vertex that
 * lists it as child), else its PVSTs with the line letters of POVU_HIP_F_LEAF_SUBFLUBBLES when it carries those */
povu_hip_sites *povu_hip_forest_sites(const povu_hip_forest *f);
void povu_hip_sites_free(povu_hip_sites *s);
/* The VCF of `c` (made by povu_hip_call from `sites` and `names`; path_name as given to _names_make): header, a contig line
 * per reference path, the column line, the records (a POVU_HIP_CALL_SUBR record: ID from the first and last step of its
 * REF AT string, both written '>' when both are '<'; VARTYPE=SUBR, no ES, no LV).  date NULL = today (%Y%m%d); only_prefix
 * NULL = every reference, else the contig lines and records of the reference paths whose name starts with it; the records
 * are formatted in chunks on up to `threads` threads (at least 1024 records each).  malloc'd, free with
 * povu_hip_buffer_free; NULL on arguments that do not belong together. */
char *povu_hip_calls_vcf(const povu_hip_calls *c, const povu_hip_sites *sites, const povu_hip_call_names *names,
			 const char *const *path_name, const char *date, const char *only_prefix, uint32_t threads, size_t *len);
/* ... of a call made under `profile` (POVU_HIP_PROFILE_*).  povu_hip_calls_vcf reads nothing behind n_inv_tier2 of `c` (a
 * caller built against the struct of before stays valid) and writes the plain call's text; this entry reads the fields behind it.  A nested call's text
 * carries one ##INFO line for PS behind the header and PS=<the parent's ID> behind LV of a record with a parent; under
 * _TOP_LEVEL_ONLY every flubble record's ID gets `:top` and its INFO ORIGIN, PROFILE and PASSTHROUGH, under _POPPED a rescued
 * record's ID gets `:rescued` and its INFO ORIGIN, PARENT, PROFILE, RESCUED_CHILD and POPPED_PARENT, any other ORIGIN,
 * PROFILE and PASSTHROUGH; the ##INFO lines of those keys stand before the contig lines.  level, parent_query and
 * ref_spelled may be NULL (a hand-made povu_hip_calls): then the plain call's values hold.  Under _LEFT_NORMALIZED a record
 * with POVU_HIP_CALL_NORMALIZED is written with POS, REF and ALT normalised, `:norm` behind its ID and ORIGIN, RAW_ALT_INDEX,
 * PROFILE, LEFT_NORMALIZED, RAW_POS, RAW_REF and RAW_ALT behind LV (or PS), any other record as the raw call writes it; raw_pos
 * or norm_block NULL: no record was changed.  Under _DECOMPOSED the rows are written instead of the records (INTEGRATION.md
 * "Decomposed calls": IDs `<label>:<alt>:snp<k>` / `ins<k>` / `del<k>` / `passthrough`, `<label>:subr-passthrough`; a _ROW_RAW row is
 * its record's raw line); NULL row arrays: the raw records; with mrow_off not NULL the merged rows are written instead of the rows
 * ("Merged primitives": a group of two or more as its representative with `MERGED=<members>;MERGED_FROM=<ids>` behind
 * `DECOMPOSED=T`, GT and the counts from mrow_*; NULL when a member index or an offset points outside the rows).  Under the other profiles the fields behind `nested` are not
 * read.  NULL for an unknown profile */
char *povu_hip_calls_vcf_profile(const povu_hip_calls *c, const povu_hip_sites *sites, const povu_hip_call_names *names,
				 const char *const *path_name, const char *date, const char *only_prefix, uint32_t threads, uint32_t profile,
				 size_t *len);
/* With rec_unt not NULL or untangled set (POVU_HIP_T_UNTANGLE) _vcf_profile writes the header lines of LN, LC and CN behind those
 * above and an untangled record with `;LN=<lap>;LC=<n_laps>` behind LV, FORMAT GT:CN and every sample column <GT>:<CN>; NULL when
 * only some of rec_unt, lap, n_laps and lap_count are given.
 * With rec_offref not NULL or offref set (POVU_HIP_T_OFFREF; a call without records has no arrays) _vcf_profile writes the off-reference records too: `;OFFREF=T` and, with a host,
 * `;HOST=<its label>;HA=<its allele>` behind LV, the ##INFO lines of the three keys in front of the contig lines, and behind
 * the reference paths' contig lines one for every surrogate of off_contig_path (of those the prefix selects); NULL when a
 * host_query or an off_contig_path points outside its range.  _vcf_rest is the same text for the records whose CHROM starts
 * with none of the n_prefixes prefixes: no contig line of a reference path, those of the surrogates that start with none */
char *povu_hip_calls_vcf_rest(const povu_hip_calls *c, const povu_hip_sites *sites, const povu_hip_call_names *names,
			      const char *const *path_name, const char *date, const char *const *prefix, uint32_t n_prefixes, uint32_t threads,
			      uint32_t profile, size_t *len);

/* ---- VCF checks ("VCF checks": decided here, pinned where the reference states it): does a VCF still
 * describe the graph?  For every record and every haplotype that carries an allele, the allele's AT walk must occur in a path
 * of that haplotype (zien::validate::validate_vcf_records, src/zien/validate/validate.cpp, bounded by the path and with the
 * reverse reading accepted) ---- */
/* the status of a task: a (record, sample column, phase) with a called allele */
#define POVU_HIP_V_FOUND_FWD 0u /* the walk occurs contiguously in a path of the task's slot, entirely inside that path */
#define POVU_HIP_V_FOUND_REV 1u /* not forward, but flip(w[m - 1]) .. flip(w[0]) does (ABSENT under POVU_HIP_V_FORWARD_ONLY) */
#define POVU_HIP_V_ABSENT 2u
#define POVU_HIP_V_NO_AT 3u    /* no AT, fewer walks than the allele's number + 1, or an empty walk */
#define POVU_HIP_V_BAD_STEP 4u /* a step names a segment the graph does not have */
#define POVU_HIP_V_NO_SLOT 5u  /* no sample has the column's name, or the phase is beyond its slots */
/* (checked in this order: NO_AT, BAD_STEP, NO_SLOT, FOUND_FWD, FOUND_REV, ABSENT).  In front of them all: a task that names an
 * allele spelled `*` (the spanning allele of VCF 4.2, "Spanning alleles") is not searched and is FOUND_FWD -- the allele is
 * absent by an overlapping event and there is nothing to find; its AT entry `*` is read as a walk without steps.  As a
 * record's reason also: */
#define POVU_HIP_V_MISSPELLED 6u
#define POVU_HIP_V_N_STATUS 6u /* task statuses */
/* the spelling of an allele (POVU_HIP_V_SPELLING): not checked (the flag is off, no walk, a walk with a bad step or no text for
 * it), the text is the concatenation of all steps, of the first step's last base and the other steps, or neither */
#define POVU_HIP_V_SPELL_NONE 0u
#define POVU_HIP_V_SPELL_WHOLE 1u
#define POVU_HIP_V_SPELL_ANCHORED 2u
#define POVU_HIP_V_SPELL_MISSPELLED 3u
/* povu_hip_vcf_opts.flags */
#define POVU_HIP_V_FORWARD_ONLY 1u /* the reference's literal rule: a walk found only reversed is ABSENT */
#define POVU_HIP_V_SPELLING 2u	   /* also compare REF / ALT with the sequences of the walks (needs povu_hip_segments_upload) */
#define POVU_HIP_V_FORCE_TIER2 4u  /* every search through the wave-per-unit kernel (tests) */
/* A parsed VCF (host only).  Alleles of a record: REF, then the ALTs (`.`: none), then one without text for every AT walk beyond
 * them.  An allele's steps are its AT walk ([step_off[a], step_off[a + 1]); allele_walk 0: the record's AT has no such walk, which
 * differs from an empty one only in the text), its text REF or the ALT as written.  Tasks: per record in (allele, column, phase)
 * order, the allele numbered within the record (it may lie beyond the record's alleles: NO_AT). */
typedef struct {
	uint64_t n_samples, n_records, n_alleles, n_steps, n_text_bytes, n_tasks, n_id_bytes;
	const char *const *sample;  /* [n_samples] the names of the sample columns */
	const uint64_t *rec_line;   /* [n_records] line of the text, from 1 */
	const uint64_t *rec_pos;    /* [n_records] POS */
	const uint64_t *rec_id_off; /* [n_records + 1] ID of record r: ids[rec_id_off[r] .. rec_id_off[r + 1]) */
	const char *ids;
	const uint64_t *allele_off; /* [n_records + 1] alleles of record r */
	const uint64_t *task_off;   /* [n_records + 1] tasks of record r */
	const uint64_t *step_off;   /* [n_alleles + 1] */
	const uint64_t *text_off;   /* [n_alleles + 1] */
	const uint8_t *allele_walk; /* [n_alleles] 1: AT holds a walk for the allele; bit 1 (2): the allele has a text */
	const uint32_t *step_id;    /* [n_steps] segment id */
	const uint8_t *step_or;	    /* [n_steps] 0 '>', 1 '<' */
	const char *text;	    /* [n_text_bytes] */
	const uint32_t *task_record, *task_allele, *task_col, *task_phase; /* [n_tasks] */
	/* (behind everything the VCF checks read: what povu_hip_vcf_compare reads beside it) */
	uint64_t n_chroms;
	const char *const *chrom;   /* [n_chroms] the distinct CHROM strings, in order of first appearance */
	const uint32_t *rec_chrom;  /* [n_records] */
} povu_hip_vcf_doc;
/* Reads VCF text: the #CHROM line names the sample columns; per record ID, POS, REF, ALT, the AT key of INFO (comma-separated,
 * one walk per allele, REF first; a walk is `[<>]id` repeated) and the GT subfield, whose position is found in FORMAT (a record
 * without GT has no tasks).  A GT is split at `|` and `/`, entry j is phase j, `.` entries are skipped.  The records are parsed in
 * chunks on up to `threads` threads.  A malformed line (fewer than 8 columns, a column count that differs from the #CHROM
 * line's, a POS or a GT entry that is no number, a walk that is no walk, a record in front of the #CHROM line) is refused: NULL and
 * a message that begins `line <n>: `; of several the first.  Free with povu_hip_vcf_doc_free. */
povu_hip_vcf_doc *povu_hip_vcf_parse(const char *text, size_t len, uint32_t threads, char *err, size_t errlen);
void povu_hip_vcf_doc_free(povu_hip_vcf_doc *d);
/* The samples and slots of the paths named `path_name` by the rule of povu_hip_call_names_make, without reference prefixes
 * (refs.n_refs is 0).  Free with povu_hip_call_names_free. */
povu_hip_call_names *povu_hip_vcf_names_make(uint32_t n_paths, const char *const *path_name, char *err, size_t errlen);
/* Column c, phase j of `doc` is the j-th slot of the sample named like the column: col_first[c] that sample's first slot and
 * col_slots[c] the number of its slots (0: no sample has the name).  [doc->n_samples] each.  0 on success */
int povu_hip_vcf_columns(const povu_hip_vcf_doc *doc, const povu_hip_call_names *names, uint32_t *col_first, uint32_t *col_slots);
typedef struct {
	uint32_t flags; /* POVU_HIP_V_* */
} povu_hip_vcf_opts;
typedef struct {
	uint64_t n_records, n_tasks, n_alleles;
	const uint8_t *task_status;  /* [n_tasks] POVU_HIP_V_FOUND_FWD .. _NO_SLOT */
	const uint8_t *allele_spell; /* [n_alleles] POVU_HIP_V_SPELL_* */
	const uint8_t *rec_invalid;  /* [n_records] 1: a task is not FOUND_*, or an allele is misspelled */
	/* the first failure of an invalid record in (allele, column, phase) order, a misspelled allele in front of the tasks of that
	 * allele: its reason (a status, or POVU_HIP_V_MISSPELLED), its allele within the record and its task (POVU_HIP_NIL for a
	 * misspelled allele; all three POVU_HIP_NIL / 0xFF for a valid record) */
	const uint8_t *rec_reason;
	const uint32_t *rec_allele, *rec_task;
	uint64_t n_status[POVU_HIP_V_N_STATUS]; /* tasks of every status */
	uint64_t n_invalid, n_misspelled;
	uint64_t n_tier2; /* (allele, direction) searches the wave-per-unit kernel ran */
	double device_ms; /* HIP-event time of the call, first upload to last byte on the host */
} povu_hip_vcf_report;
/* Checks `doc` against the graph and the paths resident in `ctx`; names: of the resident paths' names (povu_hip_vcf_names_make or
 * povu_hip_call_names_make).  One search per (allele, direction) over the index of the occurrences of every path word, whatever
 * the number of slots that carry the allele.  opts NULL = no flag.  Refused when no graph or no paths are resident, when `names`
 * is of another number of paths, with POVU_HIP_V_SPELLING when no sequences are resident, when the segment ids do not ascend
 * with the vertex index, on 2^32 path steps, alleles, steps, tasks or (allele, slot) pairs or more, and when device memory runs
 * out.  Free with povu_hip_vcf_report_free. */
povu_hip_vcf_report *povu_hip_vcf_check(povu_hip_ctx *ctx, const povu_hip_vcf_doc *doc, const povu_hip_call_names *names,
					const povu_hip_vcf_opts *opts, char *err, size_t errlen);
void povu_hip_vcf_report_free(povu_hip_vcf_report *r);
/* Both files of `povu vcf --report` (host only; the report may be hand-made).  report.tsv: the reference's header
 * `rec_idx ID POS AT Hap ID sample` (tabs) and a seventh column `reason`, then one line per invalid record for its first failure:
 * the record's index, ID and POS, the failing allele's walk written `[<>]id` (empty without one), the PanSN hap number of the
 * task's slot (1 when the name has none or there is no slot; `.` for a misspelled allele), the column's name (`.` likewise) and
 * the lower-case status name.  summary.txt: `No errors\n`, or `Error rate: %.2f%%\n` of invalid records over all records.  Both
 * malloc'd (povu_hip_buffer_free); NULL when the three do not belong together. */
char *povu_hip_vcf_report_text(const povu_hip_vcf_report *r, const povu_hip_vcf_doc *doc, const povu_hip_call_names *names,
			       size_t *report_len, char **summary, size_t *summary_len);

/* ---- VCF comparison ("VCF comparison": this project's own definition; the flag names of `povu vcf --compare`
 * are those of the reference's unfinished option): how do the calls of document A differ from those of document B?  One item per
 * (record, ALT) of either document, keyed by (CHROM, POS', REF', ALT') after the case fold and the suffix-then-prefix trim; items
 * of equal keys form a group; per group and sample column common to both documents the doses of both sides are compared ---- */
#define POVU_HIP_M_KEYED 0u   /* state of an item */
#define POVU_HIP_M_SKIPPED 1u /* ALT `*`, symbolic or a breakend, REF empty or `.`: counted, keyed nowhere, group POVU_HIP_NIL */
#define POVU_HIP_M_SHARED 0u  /* class of a group: members of both sides */
#define POVU_HIP_M_ONLY_A 1u
#define POVU_HIP_M_ONLY_B 2u
typedef struct {
	uint64_t n_items_a, n_items_b, n_groups, n_common_samples;
	/* per side and item (document order: record, then ALT): the record, the ALT's number (from 1), the state, POS' and the bytes
	 * the trims took at the end (first) and at the front of both texts, the group (POVU_HIP_NIL for a skipped item; POS' and
	 * the trims are 0 then) */
	const uint32_t *item_record_a, *item_record_b, *item_alt_a, *item_alt_b;
	const uint8_t *item_state_a, *item_state_b;
	const uint64_t *item_pos_a, *item_pos_b;
	const uint32_t *item_suffix_a, *item_suffix_b, *item_prefix_a, *item_prefix_b, *item_group_a, *item_group_b;
	/* per group, numbered in the order of their first items (A's items, then B's): class, members of either side, the first item
	 * (an item of A, or n_items_a + an item of B) */
	const uint8_t *group_class;
	const uint32_t *group_n_a, *group_n_b, *group_first;
	/* per common sample, in the order of A's columns: its column in A and in B, the cells of every class */
	const uint32_t *sample_col_a, *sample_col_b;
	const uint64_t *sample_tp, *sample_fp, *sample_fn, *sample_gteq;
	uint64_t n_shared, n_only_a, n_only_b; /* groups */
	uint64_t n_skipped_a, n_skipped_b;     /* items */
	uint64_t n_samples_only_a, n_samples_only_b;
	uint64_t n_tier2;  /* items the wave-per-item kernel trimmed and hashed */
	uint64_t n_splits; /* groups the exact comparison split off a run of equal hashes */
	double device_ms;  /* HIP-event time of the call, first upload to last byte on the host */
} povu_hip_vcf_cmp;
/* Compares `doc_a` (the calls) with `doc_b` (the other side), both of povu_hip_vcf_parse.  Needs no graph, paths or sequences:
 * a fresh context will do.  Of opts->flags only POVU_HIP_V_FORCE_TIER2 is read (every item through the wave kernel; tests).
 * Two documents without a common sample are compared: the per-sample tables are empty then.  Refused: a null context or
 * document, a document whose arrays do not belong together, 2^32 - 64 or more records, alleles, items, tasks or text bytes in
 * the two documents together, and when device memory runs out.  Free with povu_hip_vcf_cmp_free. */
povu_hip_vcf_cmp *povu_hip_vcf_compare(povu_hip_ctx *ctx, const povu_hip_vcf_doc *doc_a, const povu_hip_vcf_doc *doc_b,
				       const povu_hip_vcf_opts *opts, char *err, size_t errlen);
void povu_hip_vcf_cmp_free(povu_hip_vcf_cmp *c);
/* Both files of `povu vcf --compare` (host only; the comparison may be hand-made).  compare.tsv: the header
 * `side CHROM POS REF ALT rec_idx ID n` (tabs), then one line per ONLY_A / ONLY_B group in group order: `A` or `B`, the trimmed
 * key (letters in upper case), the first member's record index and ID, the number of members.  summary.txt: the groups of
 * every class with precision S / (S + X), recall S / (S + Y) and F1 2S / (2S + X + Y) to four decimals (`nan` where the
 * denominator is 0), the same from the summed tp / fp / fn, one line per common sample, and the skipped items and the
 * unmatched sample columns when there are any.  Both malloc'd (povu_hip_buffer_free); NULL when the three do not belong
 * together. */
char *povu_hip_vcf_cmp_text(const povu_hip_vcf_cmp *c, const povu_hip_vcf_doc *doc_a, const povu_hip_vcf_doc *doc_b, size_t *compare_len,
			    char **summary, size_t *summary_len);

/* ---- Haplotype comparison ("Haplotype comparison": this project's own definition): per region, sample and
 * phase, do documents A and B spell the same bases?  Every (record, ALT) of a placed record becomes an edit (s, e, T) -- the
 * reference bases [s, e), 0-based and half-open, replaced by T -- by the full suffix-then-prefix trim; the spans of the records
 * of both documents (widened, with a reference, by the reach of every indel through its repeat) fall into windows; per (window,
 * common sample, phase) cell the edits either side's GT entries name are applied to the window's text and the two haplotypes
 * compared byte by byte ---- */
#define POVU_HIP_H_EDIT 0u	/* state of an item: it has an edit */
#define POVU_HIP_H_UNSPELLED 1u /* ALT `*`, symbolic or a breakend (the skip rule of the VCF comparison) */
#define POVU_HIP_H_UNPLACED 2u	/* its record is unplaced */
/* the status of a cell, the first that applies */
#define POVU_HIP_H_INCONSISTENT 0u /* a REF field of the window differs from the window's text */
#define POVU_HIP_H_NOCALL_A 1u	   /* no record of the window on side A has a GT entry for (sample, phase) */
#define POVU_HIP_H_NOCALL_B 2u
#define POVU_HIP_H_UNSPELLED_A 3u /* an entry names an unspelled ALT, or one beyond the record's ALTs */
#define POVU_HIP_H_UNSPELLED_B 4u
#define POVU_HIP_H_CONFLICT_A 5u /* two applied edits overlap, or two insertions stand at one point */
#define POVU_HIP_H_CONFLICT_B 6u
#define POVU_HIP_H_EQUAL_REF 7u /* both haplotypes are the window's text: no edit on either side */
#define POVU_HIP_H_EQUAL 8u	/* the same bytes */
#define POVU_HIP_H_DIFFER 9u
#define POVU_HIP_H_N_STATUS 10u
#define POVU_HIP_H_MAX_REACH_DEFAULT 256u
#define POVU_HIP_H_MAX_REACH_MOST 65536u
typedef struct {
	uint32_t flags;	    /* POVU_HIP_V_FORCE_TIER2 alone is read */
	uint32_t max_reach; /* bases an indel's reach may run in either direction, 0 .. POVU_HIP_H_MAX_REACH_MOST */
} povu_hip_vcf_hap_opts;
typedef struct {
	uint64_t n_records_a, n_records_b, n_items_a, n_items_b, n_groups, n_windows, n_cells, n_common_samples;
	/* per side and record: 1 when placed, its window (POVU_HIP_NIL when unplaced) */
	const uint8_t *rec_placed_a, *rec_placed_b;
	const uint32_t *rec_window_a, *rec_window_b;
	/* per side and item (document order: record, then ALT): the record, the ALT's number (from 1), the state, the edit's s and
	 * e, the bytes the trims took at the end and at the front, the reach to the left and to the right, the edit group (equal
	 * edits of either side share one; numbered in the order of their first items, A's first).  An item that is no _H_EDIT has
	 * 0 everywhere and group POVU_HIP_NIL */
	const uint32_t *item_record_a, *item_record_b, *item_alt_a, *item_alt_b;
	const uint8_t *item_state_a, *item_state_b;
	const int64_t *item_s_a, *item_s_b, *item_e_a, *item_e_b;
	const uint32_t *item_suffix_a, *item_suffix_b, *item_prefix_a, *item_prefix_b, *item_left_a, *item_left_b, *item_right_a, *item_right_b;
	const uint32_t *item_group_a, *item_group_b;
	/* per window, in (CHROM, lo) order: the CHROM (numbered by first appearance in A, then B's new ones), [lo, hi), the records
	 * of either side, 1 when inconsistent and then the lowest offending record (a record of A, or n_records_a + a record of B;
	 * else POVU_HIP_NIL) */
	const uint32_t *win_chrom;
	const int64_t *win_lo, *win_hi;
	const uint32_t *win_n_a, *win_n_b;
	const uint8_t *win_inconsistent;
	const uint32_t *win_offender;
	/* per cell, in (window, common sample, phase) order: the status, the distinct edits applied on either side, and for a cell
	 * that was compared (_EQUAL_REF, _EQUAL, _DIFFER) both haplotype lengths (else 0); for a _DIFFER cell the first differing
	 * index, the shorter length when one haplotype is a prefix of the other (else all ones) */
	const uint32_t *cell_window, *cell_sample, *cell_phase;
	const uint8_t *cell_status;
	const uint32_t *cell_edits_a, *cell_edits_b;
	const uint64_t *cell_len_a, *cell_len_b, *cell_first_diff;
	/* per common sample, in the order of A's columns: its column in A and in B, its cells of every status
	 * (sample_status[x * POVU_HIP_H_N_STATUS + status]) */
	const uint32_t *sample_col_a, *sample_col_b;
	const uint64_t *sample_status;
	uint64_t n_status[POVU_HIP_H_N_STATUS]; /* cells of every status */
	uint64_t n_inconsistent;		   /* windows */
	uint64_t n_unplaced_a, n_unplaced_b;	   /* records */
	uint64_t n_reach_capped;		   /* edits whose reach the cap stopped */
	uint64_t n_tier2;			   /* items the wave-per-item kernel trimmed and hashed */
	uint64_t n_splits;			   /* edit groups the exact comparison split off a run of equal hashes */
	uint32_t reference;			   /* 1: reference mode */
	double device_ms;			   /* HIP-event time of the call, first upload to last byte on the host */
} povu_hip_vcf_hap;
/* Compares the haplotypes `doc_a` and `doc_b` (both of povu_hip_vcf_parse) spell.  path_name NULL: no reference -- a record is
 * placed when its REF is neither empty nor `.`, a window's text is taken from the REF fields over it (where several cover a
 * base, the greatest folded byte; any disagreement makes the window inconsistent) and no graph need be resident.  Else
 * reference mode: path_name[n_paths] names the resident paths (povu_hip_paths_upload, povu_hip_segments_upload), CHROM names a
 * path exactly, a record must lie within its path, and every indel reaches through its repeat.  opts NULL: no flag, max_reach
 * POVU_HIP_H_MAX_REACH_DEFAULT.  Refused: null context or documents, documents whose arrays do not belong together, a POS of
 * 2^40 or more, 2^32 - 64 or more records, alleles, items, tasks, text bytes or window-text bytes in the two documents together,
 * reference mode without resident paths and sequences or with another number of path names, max_reach above
 * POVU_HIP_H_MAX_REACH_MOST, and when device memory runs out.  Free with povu_hip_vcf_hap_free. */
povu_hip_vcf_hap *povu_hip_vcf_haplotypes(povu_hip_ctx *ctx, const povu_hip_vcf_doc *doc_a, const povu_hip_vcf_doc *doc_b,
					  const char *const *path_name, uint32_t n_paths, const povu_hip_vcf_hap_opts *opts, char *err,
					  size_t errlen);
void povu_hip_vcf_hap_free(povu_hip_vcf_hap *h);
/* Both files of `povu vcf --compare --haplotypes` (host only; the result may be hand-made).  haplotypes.tsv: the header
 * `CHROM START END sample phase status len_a len_b first_diff edits_a edits_b` (tabs; START 1-based, END inclusive), then one
 * line per cell that is neither _EQUAL_REF nor _EQUAL, in cell order; the lengths and the first difference are `.` but for a
 * _DIFFER cell.  hap_summary.txt: the windows and the inconsistent ones, the cells of every status, `Concordance`
 * (EQUAL_REF + EQUAL) / (those + DIFFER) and `Non-reference concordance` EQUAL / (EQUAL + DIFFER) to four decimals (`nan` at a
 * zero denominator), one line per common sample in A's column order, the unplaced records and the capped reaches when there
 * are any.  Both malloc'd (povu_hip_buffer_free); NULL when the three do not belong together. */
char *povu_hip_vcf_hap_text(const povu_hip_vcf_hap *h, const povu_hip_vcf_doc *doc_a, const povu_hip_vcf_doc *doc_b, size_t *haplotypes_len,
			    char **summary, size_t *summary_len);

/* ---- consensus haplotypes: a document's calls applied to the paths its CHROMs name (INTEGRATION.md "Consensus haplotypes") ---- */
#define POVU_HIP_C_ROUNDTRIP 1u /* povu_hip_vcf_cons_opts.flags: compare every haplotype with the one path of its slot */
#define POVU_HIP_C_NO_TEXT 2u	/* lengths, counts and the round trip only: the text stays on the device */
#define POVU_HIP_C_TIME_WRITE 8u /* write_ms is measured: an event pair around the materialiser, and the call waits for it there */
/* (POVU_HIP_V_FORCE_TIER2, 4, is read beside them: every item through the wave-per-item kernel; tests) */
/* bytes of the output a workgroup of the materialiser writes: 256 lanes, one 16-byte store each (DESIGN.md "Consensus
 * haplotypes") */
#define POVU_HIP_C_TILE_BYTES 4096u
/* the round trip of a haplotype */
#define POVU_HIP_C_RT_NONE 0u	   /* not asked for */
#define POVU_HIP_C_RT_EQUAL 1u	   /* the consensus spells the path, letters folded */
#define POVU_HIP_C_RT_DIFFER 2u	   /* rt_first_diff: the first differing offset, the shorter length when one is a prefix */
#define POVU_HIP_C_RT_NO_PATH 3u   /* no path in the slot (and the contig); the column names no sample; a phase beyond its slots */
#define POVU_HIP_C_RT_AMBIGUOUS 4u /* more than one */
#define POVU_HIP_C_N_RT 5u
typedef struct {
	uint32_t flags;		      /* POVU_HIP_C_*, POVU_HIP_V_FORCE_TIER2 */
	uint32_t n_select;	      /* entries of both lists below */
	const uint32_t *select_col;   /* [n_select] sample columns, or NULL: every column */
	const uint32_t *select_chrom; /* [n_select] CHROM ids of the document, or NULL: every CHROM.  Both lists are read as sets
				       * (an entry may repeat): the haplotypes are those of a selected column on a selected CHROM */
} povu_hip_vcf_cons_opts;
typedef struct {
	uint64_t n_haps; /* haplotypes, in (CHROM id, column, phase) order: one per (CHROM, column, phase) with a task on a placed
			  * record of the CHROM */
	const uint32_t *hap_chrom, *hap_col, *hap_phase; /* [n_haps] */
	const uint64_t *hap_len, *hap_off;		 /* [n_haps] bytes, and where they begin in `text` */
	/* [n_haps] kept edits; edits dropped as duplicates, as enclosed, as overlapping; tasks that name an unspelled ALT or one
	 * beyond the record's; placed records of the CHROM without a task */
	const uint32_t *n_applied, *n_duplicate, *n_enclosed, *n_overlap, *n_unspelled, *n_nocall;
	const uint8_t *rt_status;  /* [n_haps] POVU_HIP_C_RT_* */
	const uint32_t *rt_path;   /* [n_haps] the path compared with (POVU_HIP_NIL: none) */
	const uint64_t *rt_path_len, *rt_first_diff; /* [n_haps] its bases (0: none); ~0 unless _RT_DIFFER */
	const char *text;	   /* [n_text_bytes] the haplotypes one after another; NULL under POVU_HIP_C_NO_TEXT */
	uint64_t n_text_bytes;	   /* the sum of hap_len */
	uint64_t n_unplaced;	   /* records */
	uint64_t n_tier2;	   /* items the wave-per-item kernel trimmed */
	uint32_t roundtrip;	   /* 1: POVU_HIP_C_ROUNDTRIP was set */
	double device_ms;	   /* HIP-event time of the call, first upload to last byte on the host */
	double write_ms;	   /* ... of the materialiser alone under POVU_HIP_C_TIME_WRITE, else 0 */
} povu_hip_vcf_cons;
/* Applies the calls of `doc` (of povu_hip_vcf_parse) to the resident paths its CHROMs name (path_name[n_paths]: the resident
 * paths' names; of several paths of one name the first counts) and gives every haplotype's text.  opts NULL: no flag, no
 * selection.  Refused: null context or document, a document whose arrays do not belong together, no resident paths or
 * sequences, another number of path names, a selected column or CHROM the document does not have, a POS of 2^40 or more,
 * 2^32 - 64 or more records, alleles, items, tasks or text bytes, an output of 2^32 - 64 bytes or more (the message gives the
 * byte count: select fewer columns or CHROMs per call), and when device memory runs out.  A document without a haplotype is
 * not refused: n_haps is 0.  Free with povu_hip_vcf_cons_free. */
povu_hip_vcf_cons *povu_hip_vcf_consensus(povu_hip_ctx *ctx, const povu_hip_vcf_doc *doc, const char *const *path_name, uint32_t n_paths,
					  const povu_hip_vcf_cons_opts *opts, char *err, size_t errlen);
void povu_hip_vcf_cons_free(povu_hip_vcf_cons *c);
/* The three files of `povu vcf --consensus` (host only; the result may be hand-made).  consensus.fa: per haplotype a record
 * `>{sample}#{hap}#{CHROM}` -- hap the PanSN hap number of the slot (names: povu_hip_vcf_names_make of path_name) where the
 * sample has one for the phase, else the phase -- and its text in lines of `width` bytes (0: one line; an empty haplotype has
 * no line); empty when c->text is NULL.  roundtrip.tsv: the header `CHROM sample phase status len path path_len first_diff
 * applied duplicate enclosed overlap unspelled nocall` (tabs), then one line per haplotype that is not _RT_EQUAL; path and
 * path_len are `.` without a path, first_diff is `.` unless _RT_DIFFER.  cons_summary.txt: the haplotypes and their bases, the
 * haplotypes of every round-trip status, the edits of every kind, the unplaced records when there are any.  All malloc'd
 * (povu_hip_buffer_free); NULL when the arguments do not belong together. */
char *povu_hip_vcf_cons_text(const povu_hip_vcf_cons *c, const povu_hip_vcf_doc *doc, const povu_hip_call_names *names,
			     const char *const *path_name, uint32_t width, size_t *fasta_len, char **roundtrip, size_t *roundtrip_len, char **summary,
			     size_t *summary_len);

/* ---- measurement (bench.py, povu-stage-cost lines) ---- */
typedef struct {
	char name[48];	  /* kernel group */
	double ms;	  /* HIP-event time on the context's stream, last decompose */
	uint32_t launches;
} povu_hip_stage_time;
/* stage timings of the last povu_hip_decompose on this context */
int povu_hip_last_stage_times(const povu_hip_ctx *ctx, povu_hip_stage_time *out, int max);
typedef struct { char name[24]; int resident; uint64_t bytes; } povu_hip_arena_info;
/* every device arena of the context, in declaration order: its name, whether povu_hip_release_workspace keeps it,
 * and the bytes it holds now.  Returns the count (fills at most `max`). */
int povu_hip_arena_report(const povu_hip_ctx *ctx, povu_hip_arena_info *out, int max);
/* components redone by the one-lane kernels in the last decompose (only the test modes POVU_HIP_F_FORCE_REDO / _REDO_ODD
 * send any: crossing candidate-stack intervals, the one case that used to, are resolved by the parallel stage itself) */
uint32_t povu_hip_last_seq_redo(const povu_hip_ctx *ctx);
/* 1 when the last decompose numbered the cycle classes of the black tree edges only (the default whenever the
 * literal hi_2 rule of flubbles.cpp:566-574 picked the second-highest reach everywhere and no hairpins were asked
 * for), 0 when it went over all tree edges */
int povu_hip_last_black_only_classes(const povu_hip_ctx *ctx);
/* non-zero when the last decompose kept the bracket counts per tree vertex as bytes between the tree stage and the placing of
 * the brackets (no side of the graph has more than 253 links, and POVU_HIP_WIDE_COUNTS=1 is not set in the environment), 0
 * when the word kernels ran.  The bits say which counts were bytes: 1 ordcnt (always set then), 2 srccnt, 4 incnt */
int povu_hip_last_narrow_counts(const povu_hip_ctx *ctx);
/* Which prefix sums the class stage of the last pass read as packed count records (one 16-byte record per twelve byte
 * counts) instead of words: bit 0 = the sums of the in-counts (psin), bit 1 = the range starts of the
 * bracket lists.  Records are taken exactly where the matching count is a byte (povu_hip_last_narrow_counts bits 2 / 1),
 * unless POVU_HIP_WORD_PREFIX in the environment (read per pass) says words: 1 = both, 2 = psin, 3 = the range starts. */
int povu_hip_last_prefix_records(const povu_hip_ctx *ctx);
/* passes of this context, since it was created, that ran their tree and class stages a second time with word counts
 * because a byte of incnt would have passed 255 (capping brackets that share one target); such a pass reports 0 above */
uint64_t povu_hip_wide_repeats(const povu_hip_ctx *ctx);
/* 1 when the last decompose ran the laminarity check of the candidate stack's (prev, i) intervals (only when the literal
 * hi_2 rule capped differently from the second-highest reach somewhere, or with POVU_HIP_F_CHECK_LAMINAR) */
int povu_hip_last_laminar_check_ran(const povu_hip_ctx *ctx);
/* after a pass that ran the laminarity check: out[0] = candidate-stack entries whose (previous occurrence, this occurrence)
 * interval holds an entry that reaches back beyond it, out[1] = those whose class had really been popped off
 * add_flubbles' stack by then (flubbles.cpp:326-343) -- decided in place by the parallel stage, no sequential redo */
int povu_hip_last_crossings(povu_hip_ctx *ctx, uint32_t out[2]);
/* after a pass that numbered the classes of the black tree edges only: out[0] = the bits of the class sort's payload that
 * carried the size of an entry's bracket list above its stack index (32 - the bits of the number of stack entries, at most 8;
 * POVU_HIP_LSZ_FIELD in the environment, read per pass, lowers that cap, 0 = no field), out[1] = the candidate-stack
 * entries whose size did not fit (>= 2^out[0] - 1) and was looked up in the per-entry array instead -- all of them when
 * out[0] is 0; they are counted by this call, from the sorted order the pass left on the device (tests and profiles
 * only: one more kernel).  (0, 0) behind any other pass. */
int povu_hip_last_lsz_field(povu_hip_ctx *ctx, uint32_t out[2]);
/* number of links in the components this shard processed in the last decompose */
uint64_t povu_hip_last_links_processed(const povu_hip_ctx *ctx);

/* ---- stage-level parity hooks (tests only; device state of the last decompose) ----
 * After a pass that redid SOME components with the one-lane kernels (povu_hip_last_seq_redo() between 1 and the
 * component count - 1) the classes and candidate stacks sit in two layouts: povu_hip_debug_tree (when `cls` is asked
 * for), povu_hip_debug_edge_ids and povu_hip_debug_stack then return 4 instead of exporting half-valid state. */
/* copies comp_of[v] (0-based component rank) and local vertex idx for every GLOBAL vertex idx */
int povu_hip_debug_components(povu_hip_ctx *ctx, uint32_t *comp_of, uint32_t *local_idx);
/* tree arrays of component `comp` (0-based rank): sizes via n_tree first call with NULLs; `cls` is defined for the
 * child ends of black tree edges, and for the others too only when povu_hip_last_black_only_classes() == 0.
 * typ: bits 0-1 the vertex type (0 l, 1 r, 2 dummy), bit 2 the parent tree edge is black, bit 3 the vertex has no parent
 * (set by the parallel stages only: a pass with POVU_HIP_F_SEQUENTIAL leaves it clear) */
int povu_hip_debug_tree(povu_hip_ctx *ctx, uint32_t comp, uint32_t *n_tree, uint32_t *gid, uint8_t *typ,
			uint32_t *par, uint32_t *cls);
/* id of the tree edge into each tree vertex (tree_edge_id[0] = 0xFFFFFFFF): tree and back edges share one counter in
 * creation order (Tree::add_tree_edge / add_be, spanning_tree.cpp:784-805).  Conformance export only; returns 3 after a
 * pass that built the tree with the one-lane kernels (POVU_HIP_F_SEQUENTIAL / POVU_HIP_F_SEQ_TREE). */
int povu_hip_debug_edge_ids(povu_hip_ctx *ctx, uint32_t comp, uint32_t *n_tree, uint32_t *tree_edge_id);
/* three counter words of the last pass's class walks (tree stage, parallel form): out[0] = 2-edge-connected classes of
 * more than one side, out[1] = classes the one-lane walk handed to the wave walk (0 with POVU_HIP_F_BIG_CLASS_DFS: it
 * did not run), out[2] = entries the wave walks' stacks took from their pool (the sum of their chunk sizes).  Read-only:
 * adds nothing to a pass.  Returns 3 / 4 like povu_hip_debug_edge_ids. */
int povu_hip_debug_walk_words(povu_hip_ctx *ctx, uint32_t out[3]);
/* the children-vector pool of the last pass's splice (POVU_HIP_F_SUBFLUBBLES), component `comp`: out[0] = slots the vectors
 * took, out[1] = slots the layout gave the component.  Read-only: adds no launch, copy or synchronisation to a pass.
 * Returns 3 when the last pass ran without the inserting passes, 5 when it had no component `comp`. */
int povu_hip_debug_splice_pool(povu_hip_ctx *ctx, uint32_t comp, uint32_t out[2]);
/* candidate stack of component `comp`: tree vertex of each entry, class, next_seen */
int povu_hip_debug_stack(povu_hip_ctx *ctx, uint32_t comp, uint32_t *n, uint32_t *tree_vtx, uint32_t *cls,
			 uint32_t *next_seen);

/* ---- rows A and B alone (graph_kernels.hip; tests/test_gpu_rowb.py) ----
 * Both read arrays the context owns (the resident graph, the row-B workspace), so no guard bands lie around them.
 * 0 = ok, 1 = bad arguments or no graph resident, 2 = device error. */
/* What the last upload left: off [2 * n_vtx + 1]; adj / aoth / atwin [off[2 * n_vtx]] (room for 2 * n_links words each);
 * tip [n_vtx]; words = { adjacency slots, most links on one segment, sides without links, 1 when the slot fill built the
 * adjacency lists / 0 when the radix sort did }.  Read-only: no kernel is launched. */
int povu_hip_debug_csr(povu_hip_ctx *ctx, uint32_t *off, uint32_t *adj, uint32_t *aoth, uint32_t *atwin, uint8_t *tip,
		       uint32_t words[4]);
/* Runs the row-B step of a pass (labelling, speculative adjacency, re-index: the pass's own function, behind the pass's
 * own workspace set-up) on the resident graph under the pass flags `flags`, and exports what it left.  The caller gives
 * room for the largest case: voff / eoff / start_key n_vtx + 1 entries (n_components + 1, n_components + 1 and
 * n_components are written; a start key of ~0 = the component has no tip), comp / pos n_vtx (0-based component and sorted
 * position of every segment), loff 2 * n_vtx + 1 (offsets of the local side lists, by sorted side), ladj / lle 2 * n_links
 * (n_local_slots are written: other sorted side and link word of every local slot).  stats0 = stats[0] as the stages read
 * it, n_cross = the length of the union-find's cross list.  Invalidates the state of the last pass. */
#define POVU_HIP_ROWB_IDENTITY 1u      /* one component, or the segments already in (component, idx) order */
#define POVU_HIP_ROWB_SORT_FREE 2u     /* the sort-free adjacency builder (k_local_adj) */
#define POVU_HIP_ROWB_LEAN_IDENTITY 4u /* both: sorted space is the global vertex space, nothing is renumbered */
#define POVU_HIP_ROWB_SELF_LOOPS 8u    /* the labelling saw a self loop */
#define POVU_HIP_ROWB_DENSE_EDGES 16u  /* the builder that numbers the local links densely ran */
#define POVU_HIP_ROWB_SPEC_KEPT 32u    /* the adjacency written ahead of the component count was kept */
typedef struct {
	uint32_t n_components, n_local_slots, stats0, path_bits, n_cross;
	uint32_t *voff, *eoff, *comp, *pos, *loff, *ladj, *lle;
	uint64_t *start_key;
} povu_hip_rowb;
int povu_hip_debug_row_b(povu_hip_ctx *ctx, uint32_t flags, povu_hip_rowb *out);

/* ---- unit-test hooks for the device-wide primitives (primitives.hip; tests/test_gpu_primitives.py) ----
 * Each call works in device memory of its own and uses nothing of the context but its stream.  The primitive's scratch
 * has exactly the size the primitive asks for and is filled with a non-zero byte before the call; every device output
 * lies between two guard bands (at least 64 words of a fixed pattern each) that are read back after the call.
 * 0 = ok, 1 = bad arguments, 2 = device error, 5 = the primitive changed a guard byte. */
/* exclusive scan of in[0..n) (op 0 = sum mod 2^32, 1 = running maximum) and, when in2 is given, an independent sum scan
 * of in2[0..n2) in the same launch; op 2 = sum mod 2^64 of n 64-bit values, in and out holding each as a pair of
 * words, low word first (in2 unused).
 * op 3: in / in2 hold n / n2 BYTES, one element each (scan_exclusive_u8; in2 optional, either length may be 0);
 * op 4: sums of in[i] - in2[i], both of n words (scan_exclusive_diff_u32; out2 unused);
 * op 5: running xor of in and of in2, both of n words (scan_exclusive_xor_u32_pair);
 * op 6: running xor of n 16-byte words (scan_exclusive_xor_u128; in2 unused).  With POVU_HIP_SCAN_N_DEV or-ed on, n2 is
 *       placed in a device word and passed as n_dev: only the first min(n2 + 1, n) words exist and are written, and the
 *       rest of the output counts as a guard band.
 * POVU_HIP_SCAN_IN_PLACE, or-ed onto op 0, 1 or 2 (without in2): the output IS the input on the device. */
#define POVU_HIP_SCAN_SUM 0
#define POVU_HIP_SCAN_MAX 1
#define POVU_HIP_SCAN_U64 2
#define POVU_HIP_SCAN_U8 3
#define POVU_HIP_SCAN_DIFF 4
#define POVU_HIP_SCAN_XOR_PAIR 5
#define POVU_HIP_SCAN_XOR_U128 6
/* op 7: sums of in[i] - in2[i] with `in` n BYTES and in2 n words (scan_exclusive_diff_u8_u32; out2 unused);
 * op 8: sums of the n words of `in` and of the n2 BYTES of in2 in one launch (scan_exclusive_u32_u8_pair) */
#define POVU_HIP_SCAN_DIFF_U8 7
#define POVU_HIP_SCAN_MIXED_PAIR 8
/* op 9: sums of in[i] - in2[i] with `in` and in2 both n BYTES (scan_exclusive_diff_u8_u8; out2 unused) */
#define POVU_HIP_SCAN_DIFF_U8_U8 9
/* op 10: INCLUSIVE sums of the n words of `in` (scan_inclusive_u32; in2 unused) */
#define POVU_HIP_SCAN_INCLUSIVE 10
#define POVU_HIP_SCAN_IN_PLACE 0x100
#define POVU_HIP_SCAN_N_DEV 0x200
int povu_hip_debug_scan(povu_hip_ctx *ctx, int op, const uint32_t *in, uint32_t *out, size_t n, const uint32_t *in2,
			uint32_t *out2, size_t n2);
/* sort_pairs_u32: the n pairs (keys[i], vals[i]) in the stable order of the low `bits` bits of the keys (0 counts as 1);
 * inputs and outputs are distinct device buffers */
int povu_hip_debug_sort(povu_hip_ctx *ctx, const uint32_t *keys, const uint32_t *vals, size_t n, unsigned bits,
			uint32_t *keys_out, uint32_t *vals_out);
/* compact_flagged_u8: the indices of the non-zero bytes of flags[0..n), ascending, into out (room for n), their number
 * into *count; the device output behind the first *count indices counts as a guard band */
int povu_hip_debug_compact(povu_hip_ctx *ctx, const uint8_t *flags, size_t n, uint32_t *out, uint32_t *count);
/* totals_u32: tot[0] = the 64-bit sum of a[0..n), tot[1] = that of b[0..n) (0 when b is NULL) */
int povu_hip_debug_totals(povu_hip_ctx *ctx, const uint32_t *a, const uint32_t *b, size_t n, uint64_t tot[2]);
/* ---- unit-test hooks for the look-up structures above the primitives (segtree.hpp, common.hpp; tests/test_gpu_lookups.py) ----
 * Same conventions: device memory of the call's own, nothing of the context but its stream, scratch and unwritten outputs
 * filled with a non-zero byte, every device output between guard bands.  0 = ok, 1 = bad arguments, 2 = device error,
 * 5 = a guard byte changed.  The hooks call the real functions; their own kernels only shape the inputs. */
/* Coarse min segment tree: seg_build over val[0..n) (n = 0 allowed), then one lane per query.  The device copy of the
 * values is 16-byte aligned and padded to the next multiple of 16 with ZEROS; the tree buffer has exactly
 * SegTree::tree_words(n) words.  queries: nq x (kind, l, r, x), kind one of the three below (x unused by MIN); out[i] =
 * seg_min(l, r) / seg_first_less(l, r, x) / seg_last_less(l, r, x), 0xFFFFFFFF for an empty range or no such index.
 * r > n is refused (1); l > r is an empty range.  tree (optional): the nodes [0, 2 P), node 1 the root, node 0
 * undefined, P = the number of blocks of 16 values rounded up to a power of two (at least 1); P (optional): that number. */
#define POVU_HIP_SEG_MIN 0
#define POVU_HIP_SEG_FIRST_LESS 1
#define POVU_HIP_SEG_LAST_LESS 2
int povu_hip_debug_segtree(povu_hip_ctx *ctx, const uint32_t *val, size_t n, const uint32_t *queries, size_t nq, uint32_t *out,
			   uint32_t *tree, uint32_t *P);
/* Bit-rank directory over flags[0..n) (a non-zero byte = set): a producer of the shape of the bridge-flag kernel (256
 * lanes, four flags a lane, bitrank_store_wave), then bitrank_build over n / 64 + 1 records.  rank[i] = bitrank(pos[i])
 * = set flags in front of pos[i] (pos[i] <= n, else 1); test[i] = bitrank_test(pos[i]) as 0 / 1 where pos[i] < n, left
 * unwritten (0xC5C5C5C5) where pos[i] == n.  records (optional): the n / 64 + 2 records of four words (bits 0..31, bits
 * 32..63, set flags in front, 0), the last one the closing record. */
int povu_hip_debug_bitrank(povu_hip_ctx *ctx, const uint8_t *flags, size_t n, const uint32_t *pos, size_t nq, uint32_t *rank,
			   uint32_t *test, uint32_t *records);
/* Count records (common.hpp): scan_count_records_u8 over the n0 BYTES of in0 and, in the same launch, the n1 bytes of in1
 * (in1 may be NULL, either length may be 0), then one lane per query.  A record is four words: the counts of twelve
 * consecutive elements as bytes (words 0..2; zero behind the end of the array) and the sum of every count in front of
 * them (word 3).  rec0 / rec1 (optional): the (n + 11) / 12 records that hold an element; the slack record behind them
 * must come back unwritten (else 5).  prefix[i] = cntrec_prefix(pos[i]) = the sum in front of element pos[i], count[i] =
 * cntrec_count(pos[i]) = that element; pos[i] >= n is refused (1).  tile (optional, filled whatever else happens):
 * elements a tile of the scan's two-launch form / of its one-launch form covers. */
int povu_hip_debug_count_records(povu_hip_ctx *ctx, const uint8_t *in0, size_t n0, const uint32_t *pos0, size_t nq0, uint32_t *rec0,
				 uint32_t *prefix0, uint32_t *count0, const uint8_t *in1, size_t n1, const uint32_t *pos1, size_t nq1,
				 uint32_t *rec1, uint32_t *prefix1, uint32_t *count1, uint64_t tile[2]);
/* append_in_order: workgroups of 256 lanes, each over 16 384 positions of flags[0..n), append their set positions to
 * list (room for n); *count = the length.  A workgroup's positions form one ascending stretch; the order of the
 * stretches is up to the atomics.  The device list behind the first *count entries counts as a guard band. */
int povu_hip_debug_append(povu_hip_ctx *ctx, const uint8_t *flags, size_t n, uint32_t *list, uint32_t *count);
/* unit-test hook for the list ranking of the tree stage: suffix sums (inclusive, mod 2^32) along the lists next[0..n)
 * (NIL = end of a list; heads[0..nh) = their first elements, NIL entries allowed) -- mode 0: ra of the 0/1 weights w;
 * mode 1: the pre-order events' two sums (element x enters when x % 3 == 0, see list_rank.hip), ra and rb.  bits =
 * splitter bucket bits, 2..6 (0: the default).  Elements in no list get no defined value.  0 = ok, 1 = bad arguments,
 * 2 = device error. */
int povu_hip_debug_list_rank(povu_hip_ctx *ctx, uint32_t n, const uint32_t *next, const uint8_t *w, const uint32_t *heads,
			     uint32_t nh, int mode, uint32_t bits, uint32_t *ra, uint32_t *rb);
/* What the level-0 walk of a list ranking left in its records (list_rank.hpp: a record is one narrow word -- the owner as
 * a signed delta to its bucket, the partial sums in small fields -- or, where a field does not fit, an escaped pair of words).
 * Counted by a kernel of its own that walks the lists again behind the ranking.  hist[33 * d + p] = live elements whose
 * owner delta needs d bits (zigzag: 2|v| or 2|v| - 1) and whose partial sums need p bits (the events: the wider of the two),
 * whatever the fields in use are. */
typedef struct povu_hip_rank_records {
	uint64_t live;		  /* elements a walk reaches */
	uint64_t escaped;	  /* ... whose record is escaped (all of them when final_ranks) */
	uint32_t final_ranks;	  /* the events' 16-bit partials overflowed: the records hold final ranks */
	uint32_t bucket_bits;	  /* splitter bucket bits of the ranking */
	uint32_t delta_bits;	  /* field of the signed owner delta: [-2^(delta_bits-1), 2^(delta_bits-1)) */
	uint32_t partial_bits[2]; /* fields of the partial sums: the tour's one (second: 0); the events' partial(a) and partial(a) - partial(b) */
	uint64_t hist[33 * 33];
} povu_hip_rank_records;
/* which: 0 = the tour's records of the last pass, 1 = its pre-order events' (both collected only when the environment
 * variable POVU_HIP_RANK_STATS was set while the pass ran), 2 = those of the last povu_hip_debug_list_rank call.  esc
 * (optional, which == 2 only, n_esc = that call's n): 1 where the element's record carries the escape bit (elements in no
 * list: undefined).  Read-only.  0 = ok, 1 = bad arguments or no pass, 3 = nothing was collected. */
int povu_hip_debug_rank_escapes(povu_hip_ctx *ctx, int which, povu_hip_rank_records *out, uint8_t *esc, size_t n_esc);
/* timing hook (tools/scan_time.py): `reps` exclusive scans (op as above) of n device-resident words, ms per scan by HIP
 * events; < 0 on error */
double povu_hip_debug_scan_time(povu_hip_ctx *ctx, size_t n, int reps, int op);

/* device workspace (bytes) one plain povu_hip_decompose call reserves for a graph of this size whose vertices come grouped
 * by component and that has no hub vertex (> 48 links) and no self loop -- a pangenome GFA --, excluding the resident graph
 * itself (~42 B/link + 13 B/segment), the one-lane kernels' lists and the wave walk's arrays (44 B per side, taken by the
 * first pass that meets a 2-edge-connected class of more than 256 sides); sides without links are assumed to number two per
 * component and one segment in 64.  The general case: povu_hip_workspace_breakdown.  n_components = 0 assumes the worst
 * case (every segment its own component); 0 when it cannot be computed */
uint64_t povu_hip_workspace_estimate(uint32_t n_vtx, uint32_t n_links, uint32_t n_components);
/* the parts of that estimate: [0] rows A/B state of a graph whose vertices come grouped by component, without hub vertices
 * or self loops ([6]: the general case), [1] tree / result arrays all execution modes share, [2] / [3] class stage: arrays
 * the tree stage already writes / arrays first written by the class stage, [4] / [5] tree stage: arrays that outlive it / its
 * own.  [3] and [5] share one stretch (the larger of the two counts) */
int povu_hip_workspace_breakdown(uint32_t n_vtx, uint32_t n_links, uint32_t n_components, uint64_t out[7]);
/* Reserves the device memory a graph of this size will need (resident graph, CSR build scratch, decompose workspace for
 * the worst case of components) on a context that holds nothing yet, so that the first upload + decompose do not pay for
 * the allocation: meant to run on another thread while the caller still parses its input, when that takes longer than
 * bringing the runtime up (the CLI does so with POVU_CLI_PREWARM=1; exact sizes, no head room).  Best effort:
 * returns 0 and reserves nothing when the worst case does not fit; 1 + message only for bad arguments / HIP errors.  Must
 * not run concurrently with another call on the same context. */
int povu_hip_prewarm(povu_hip_ctx *ctx, uint32_t n_vtx, uint32_t n_links, char *err, size_t errlen);
/* upper bound of the EXTRA device memory POVU_HIP_F_LEAF_SUBFLUBBLES takes while its stage runs (allocated and released
 * inside the call; n_components = 0: not known) */
uint64_t povu_hip_leaf_workspace_estimate(uint32_t n_vtx, uint32_t n_components);

const char *povu_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif
