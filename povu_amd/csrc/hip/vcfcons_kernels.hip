// vcfcons_kernels.hip -- povu_hip_vcf_consensus (include/povu_hip.h): the calls of one parsed VCF applied to the resident paths
// its CHROMs name, one text per (CHROM, sample column, phase), and each text compared with the path of its slot.
//
// The definition is INTEGRATION.md "Consensus haplotypes" (restated in tests/vcfcons_ref.py; the rules that are plain
// arithmetic are vcfcons_rules.hpp).  The document goes through the front end of the comparisons as a pair whose second
// document is empty (vcf_pair.hpp); placement, the edits and the edit groups are the haplotype comparison's (vcfhap_edits.hpp,
// exact_groups.hpp).  Coordinates on the device carry one more than the 0-based value.
//   place     a lane per record; the placed records of every CHROM counted;
//   edits     the two tiers over EditPolicy; groups numbered in first-item order; the items sorted by (s, insertion first,
//             e descending, group): an item's place in that order is what its tasks sort by;
//   tasks     a lane per task: it takes part when its record is placed and its column and CHROM are selected; the tasks
//             sorted by (CHROM, column, phase, kind, place); heads give the haplotypes, the tasks with an edit are a
//             haplotype's tail, in the order of the definition;
//   lists     a wave per haplotype, 64 edits a chunk with carries: the exclusive running maximum of the ends (the wave
//             max-scan of the haplotype comparison's conflicts) decides the drops, a ballot ranks the kept edits, the wave
//             sum-scan of their length changes places each in its haplotype; the lengths, then one device-wide scan for
//             the haplotypes' offsets in the output;
//   spell     a lane per base: every path that is read -- a selected CHROM's, a round trip's -- once into a flat buffer;
//   write     the materialiser: a workgroup per POVU_HIP_C_TILE_BYTES of the output, a lane per 16 bytes and one 16-byte
//             store.  The tile's haplotype by bisection over the output offsets, the lane's from there; the tile's first and
//             last edit once by vh_locate, the lane's first edit between them (vc_seek_between), then linearly (vc_source).  Sixteen bytes inside one run of path bases are
//             two aligned 16-byte loads and a funnel shift (one load where the run is aligned); everything else -- bytes of
//             T, the bytes around an edit's or a haplotype's edge -- goes byte by byte;
//   compare   the round trip: a wave per 64 bytes of the output, a ballot of fold(consensus) != fold(path), the lowest
//             differing offset of a haplotype by atomicMin.
// Every shuffle and ballot runs with all 64 lanes (trip counts around them are wave-uniform).  What bounds the stores:
// records below nR, items below nI, tasks, haplotypes and kept edits below nV <= nT (a haplotype has a task, a kept edit is a
// task), flat bytes below NF (the buffer has 32 more for the funnel's second load), output bytes below `total` rounded up to
// 16 (the buffer has that and 16 more; the bytes from `total` on are written as 0).
#include "vcfcons_rules.hpp"
#include "vcfhap_edits.hpp"

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>

namespace povu_hip
{

namespace
{

constexpr uint64_t OUT_LIMIT = (1ull << 32) - 64;

__global__ void k_vc_chrom_placed(uint32_t nR, const uint8_t *__restrict__ placed, const uint32_t *__restrict__ chrom, uint32_t *__restrict__ n_placed)
{
	for (uint32_t r = blockIdx.x * Q_TPB + threadIdx.x; r < nR; r += gridDim.x * Q_TPB)
		if (placed[r])
			atomicAdd(n_placed + chrom[r], 1u);
}
// the bases of every listed path, from the scan over its steps
__global__ void k_vc_path_len(RefView R, uint64_t *__restrict__ plen)
{
	for (uint32_t l = blockIdx.x * Q_TPB + threadIdx.x; l < R.nR; l += gridDim.x * Q_TPB)
		plen[l] = R.roff[R.ref_base[l + 1]] - R.roff[R.ref_base[l]];
}
// the items' order by (s, insertion first, e descending, group): part `which` of vc_sort_key (an item without an edit sorts by
// the group number one past the last)
__global__ void k_vc_item_key(uint32_t n, int which, uint32_t nG, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ gid,
			      const uint64_t *__restrict__ bs, const uint64_t *__restrict__ be, uint32_t *__restrict__ key)
{
	for (uint32_t x = blockIdx.x * Q_TPB + threadIdx.x; x < n; x += gridDim.x * Q_TPB) {
		const uint32_t i = perm[x];
		key[x] = vc_sort_key(which, bs[i], be[i], min(gid[i], nG));
	}
}
__global__ void k_vc_inverse(uint32_t n, const uint32_t *__restrict__ perm, uint32_t *__restrict__ place)
{
	for (uint32_t x = blockIdx.x * Q_TPB + threadIdx.x; x < n; x += gridDim.x * Q_TPB)
		place[perm[x]] = x;
}

// ---- the tasks
struct VcTasks {
	uint32_t nT, nV; // tasks, those that take part (the first nV of the sorted list)
	const uint32_t *t_rec, *t_al, *t_col, *t_ph; // [nT] uploaded
	uint32_t *chrom, *item;			      // [nT] CHROM id (n_chroms: takes no part), item of a KIND_EDIT task
	uint8_t *kind;				      // [nT]
};
__global__ __launch_bounds__(Q_TPB) void k_vc_tasks(PairView A, VcTasks K, uint32_t n_chroms, const uint8_t *__restrict__ chrom_sel,
						     const uint8_t *__restrict__ col_sel, const uint8_t *__restrict__ placed,
						     const uint8_t *__restrict__ state, unsigned long long *__restrict__ cnt)
{
	const uint32_t lane = threadIdx.x & 63u;
	unsigned long long n = 0;
	for (uint64_t b = ((uint64_t)blockIdx.x * Q_TPB + threadIdx.x) & ~63ull; b < K.nT; b += (uint64_t)gridDim.x * Q_TPB) {
		const uint64_t t = b + lane;
		bool valid = false;
		if (t < K.nT) {
			const uint32_t r = K.t_rec[t], al = K.t_al[t], c = A.chrom[r];
			valid = placed[r] && chrom_sel[c] && col_sel[K.t_col[t]];
			uint32_t kind = KIND_REF, item = 0;
			if (al) {
				const uint32_t i0 = A.ioff[r], n_alts = A.ioff[r + 1] - i0;
				kind = al <= n_alts && state[i0 + al - 1] == POVU_HIP_H_EDIT ? KIND_EDIT : KIND_UNSPELLED;
				item = kind == KIND_EDIT ? i0 + al - 1 : 0;
			}
			K.chrom[t] = valid ? c : n_chroms, K.item[t] = item, K.kind[t] = (uint8_t)kind;
		}
		n += __popcll(__ballot(valid));
	}
	if (lane == 0 && n)
		atomicAdd(cnt + CN_TASKS, n);
}
// which = 0 the item's place in the order, 1 kind, 2 phase, 3 column, 4 CHROM
__global__ void k_vc_task_key(VcTasks K, int which, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ place, uint32_t *__restrict__ key)
{
	for (uint32_t x = blockIdx.x * Q_TPB + threadIdx.x; x < K.nT; x += gridDim.x * Q_TPB) {
		const uint32_t t = perm[x];
		key[x] = which == 0 ? (K.kind[t] == KIND_EDIT ? place[K.item[t]] : 0u) : which == 1 ? K.kind[t] : which == 2 ? K.t_ph[t] : which == 3 ? K.t_col[t] : K.chrom[t];
	}
}
// per sorted task x <= nV: does it open a haplotype?
__global__ void k_vc_heads(VcTasks K, const uint32_t *__restrict__ sorted, uint32_t *__restrict__ head)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x <= K.nV; x += (uint64_t)gridDim.x * Q_TPB) {
		uint32_t hd = 0;
		if (x < K.nV) {
			const uint32_t t = sorted[x], p = x ? sorted[x - 1] : 0;
			hd = !(x && K.chrom[t] == K.chrom[p] && K.t_col[t] == K.t_col[p] && K.t_ph[t] == K.t_ph[p]);
		}
		head[x] = hd;
	}
}
// the haplotypes: what the list kernel writes, [nH + 1] each but the kept edits, [nV]
struct VcHaps {
	uint32_t n;
	uint32_t *x0;			     // first sorted task
	uint32_t *chrom, *col, *phase, *e0;  // e0: where its kept edits begin in k_item / k_start
	uint32_t *n_applied, *n_duplicate, *n_enclosed, *n_overlap, *n_unspelled, *n_nocall;
	uint64_t *len, *fb;		     // bytes; where its path begins in the flat buffer
	uint32_t *k_item;		     // the kept edits of all haplotypes: the item, and
	uint64_t *k_start;		     // where it begins in its haplotype
};
__global__ void k_vc_open(VcTasks K, VcHaps H, const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ head, const uint32_t *__restrict__ hidx)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x <= K.nV; x += (uint64_t)gridDim.x * Q_TPB) {
		if (x == K.nV) {
			H.x0[H.n] = K.nV;
			continue;
		}
		if (head[x]) {
			const uint32_t t = sorted[x], h = hidx[x]; // (below the number of heads: H.n)
			H.x0[h] = (uint32_t)x, H.chrom[h] = K.chrom[t], H.col[h] = K.t_col[t], H.phase[h] = K.t_ph[t];
		}
	}
}
// ---- lists: a wave per haplotype
struct VcLists {
	const uint32_t *sorted;
	const uint8_t *kind;
	const uint32_t *item, *gid;
	const uint64_t *bs, *be;
	const uint32_t *t_len;
	const uint32_t *chrom_ref, *chrom_placed;
	const uint64_t *plen, *foff; // [listed paths] bases, flat offset
};
__global__ __launch_bounds__(Q_TPB) void k_vc_lists(VcHaps H, VcLists Y)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	const uint64_t below = lane ? (1ull << lane) - 1 : 0;
	for (uint32_t h = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); h < H.n; h += waves) {
		const uint32_t x0 = H.x0[h], x1 = H.x0[h + 1];
		const uint32_t a1 = first_not(x0, x1, [&](uint32_t k) { return Y.kind[Y.sorted[k]] < KIND_UNSPELLED; });
		const uint32_t a2 = first_not(a1, x1, [&](uint32_t k) { return Y.kind[Y.sorted[k]] < KIND_EDIT; });
		uint64_t carry_end = 0, carry_bs = 0, carry_be = 0, carry_d = 0; // of the chunks in front (an end is 1 at least)
		uint32_t carry_g = 0, n_keep = 0, n_dup = 0, n_enc = 0, n_ovl = 0;
		for (uint32_t c0 = a2; c0 < x1; c0 += 64) {
			const uint32_t x = c0 + lane;
			const bool in = x < x1;
			const uint32_t i = in ? Y.item[Y.sorted[x]] : 0, g = in ? Y.gid[i] : 0;
			const uint64_t bs = in ? Y.bs[i] : 0, be = in ? Y.be[i] : 0;
			const uint64_t incl = wave_inclusive_scan(be, ScanOp<1>{});
			uint64_t before = __shfl_up((unsigned long long)incl, 1, 64), pbs = __shfl_up((unsigned long long)bs, 1, 64),
				 pbe = __shfl_up((unsigned long long)be, 1, 64);
			uint32_t pg = __shfl_up(g, 1, 64);
			if (lane == 0)
				before = 0, pbs = carry_bs, pbe = carry_be, pg = carry_g;
			before = max(before, carry_end);
			const uint32_t verdict = in ? vc_decide(bs, be, g, x > a2, before, pbs, pbe, pg) : (uint32_t)VC_DUPLICATE;
			const bool keep = in && verdict == VC_KEEP;
			const uint64_t d = keep ? vc_delta(bs, be, Y.t_len[i]) : 0;
			const uint64_t dincl = wave_inclusive_scan(d, ScanOp<0>{});
			const unsigned long long km = __ballot(keep);
			if (keep) {
				const uint32_t at = a2 + n_keep + (uint32_t)__popcll(km & below); // (below x: the kept are no more than the seen)
				H.k_item[at] = i, H.k_start[at] = (bs - 1) + carry_d + (dincl - d);
			}
			n_keep += (uint32_t)__popcll(km);
			n_dup += (uint32_t)__popcll(__ballot(in && verdict == VC_DUPLICATE));
			n_enc += (uint32_t)__popcll(__ballot(in && verdict == VC_ENCLOSED));
			n_ovl += (uint32_t)__popcll(__ballot(in && verdict == VC_OVERLAP));
			carry_end = max(carry_end, (uint64_t)__shfl((unsigned long long)incl, 63, 64));
			carry_d += (uint64_t)__shfl((unsigned long long)dincl, 63, 64);
			carry_bs = __shfl((unsigned long long)bs, 63, 64), carry_be = __shfl((unsigned long long)be, 63, 64), carry_g = __shfl(g, 63, 64);
		}
		if (lane == 0) {
			const uint32_t c = H.chrom[h], l = Y.chrom_ref[c]; // (a placed record's CHROM names a path)
			H.e0[h] = a2, H.n_applied[h] = n_keep, H.n_duplicate[h] = n_dup, H.n_enclosed[h] = n_enc, H.n_overlap[h] = n_ovl;
			H.n_unspelled[h] = a2 - a1, H.n_nocall[h] = Y.chrom_placed[c] - (x1 - x0);
			H.len[h] = Y.plen[l] + carry_d, H.fb[h] = Y.foff[l];
		}
	}
}

// ---- the flat spelling of the listed paths that are read (foff: [nL + 1], an unread path has no bytes)
__global__ void k_vc_spell(uint64_t NF, RefView R, PathsView P, const uint64_t *__restrict__ foff, uint8_t *__restrict__ flat)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x < NF; x += (uint64_t)gridDim.x * Q_TPB) {
		const uint32_t l = span_of(foff, R.nR, x);
		uint32_t seg;
		flat[x] = ref_path_base(P, R.roff, ref_path_slice(R, P, l), x - foff[l], &seg);
	}
}

// ---- the materialiser
struct VcMat {
	uint32_t nH;
	uint64_t total;
	const uint64_t *hoff; // [nH + 1]
	const uint32_t *e0, *n_kept;
	const uint64_t *fb;
	const uint32_t *k_item;
	const uint64_t *k_start;
	const uint64_t *be, *t_at;
	const uint32_t *t_len;
	const char *text;
	const uint8_t *flat; // (16-byte aligned, 32 bytes of room behind the last base)
	uint8_t *out;
};
// the 16 bytes from p on: the two aligned 16-byte words they lie in, shifted together
__device__ __forceinline__ uint4 load16(const uint8_t *__restrict__ p)
{
	const uintptr_t a = reinterpret_cast<uintptr_t>(p);
	const uint32_t sh = (uint32_t)(a & 15u);
	const uint4 *__restrict__ q = reinterpret_cast<const uint4 *>(a - sh);
	const uint4 lo = q[0];
	if (sh == 0)
		return lo;
	const uint4 hi = q[1];
	const uint64_t w0 = lo.x | (uint64_t)lo.y << 32, w1 = lo.z | (uint64_t)lo.w << 32, w2 = hi.x | (uint64_t)hi.y << 32, w3 = hi.z | (uint64_t)hi.w << 32;
	const uint32_t b = (sh & 7u) * 8u;
	const bool up = sh >= 8;
	const uint64_t a0 = up ? w1 : w0, a1 = up ? w2 : w1, a2 = up ? w3 : w2;
	const uint64_t o0 = b ? (a0 >> b) | (a1 << (64 - b)) : a0, o1 = b ? (a1 >> b) | (a2 << (64 - b)) : a1;
	return make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
}
static_assert(Q_TPB * 16 == POVU_HIP_C_TILE_BYTES, "a workgroup writes a tile: a lane 16 bytes");
__global__ __launch_bounds__(Q_TPB) void k_vc_materialise(VcMat M)
{
	const uint64_t tile0 = (uint64_t)blockIdx.x * POVU_HIP_C_TILE_BYTES, g0 = tile0 + (uint64_t)threadIdx.x * 16;
	if (g0 >= M.total)
		return;
	const uint32_t ht = span_of(M.hoff, M.nH, tile0); // the tile's haplotype, the same in every lane
	uint32_t h = ht + span_of(M.hoff + ht, M.nH - ht, g0);
	uint64_t h_end = M.hoff[h + 1], o = g0 - M.hoff[h];
	uint32_t e0 = M.e0[h], n = M.n_kept[h];
	const uint8_t *__restrict__ path = M.flat + M.fb[h];
	auto edit = [&](uint32_t u) {
		const uint32_t i = M.k_item[e0 + u];
		return VcKept{M.k_start[e0 + u], M.t_len[i], M.be[i] - 1};
	};
	// the lane's first edit: in the tile's haplotype between the tile's first and last edit, found once (the same in every
	// lane); in a haplotype that begins inside the tile among all of its edits
	VcWalk w;
	if (h == ht) {
		const uint64_t ot = tile0 - M.hoff[ht];
		const auto start = [&](uint32_t u) { return M.k_start[e0 + u]; };
		w = vc_seek_between(o, vh_locate(ot, n, start), vh_locate(ot + (POVU_HIP_C_TILE_BYTES - 1), n, start), n, edit);
	} else {
		w = vc_seek(o, n, edit);
	}
	uint4 v;
	if (g0 + 16 <= h_end) { // sixteen bytes of one haplotype: one run of path bases?
		const VhSource src = vc_source(w, o, n, edit);
		if (!src.from_edit && vc_ref_run(w, o, n) >= 16) {
			v = load16(path + src.at);
			*reinterpret_cast<uint4 *>(M.out + g0) = v;
			return;
		}
	}
	uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll
	for (uint32_t b = 0; b < 16; b++) {
		const uint64_t g = g0 + b;
		uint32_t byte = 0;
		if (g < M.total) {
			while (g >= h_end) { // the next haplotype (an empty one is passed over) from its first byte
				h++;
				h_end = M.hoff[h + 1], o = 0, e0 = M.e0[h], n = M.n_kept[h], path = M.flat + M.fb[h];
				w = vc_seek(0, n, edit);
			}
			const VhSource src = vc_source(w, o, n, edit);
			byte = src.from_edit ? (uint8_t)M.text[M.t_at[M.k_item[e0 + w.k]] + src.at] : path[src.at];
			o++;
		}
		word[b >> 2] |= byte << ((b & 3u) * 8u);
	}
	*reinterpret_cast<uint4 *>(M.out + g0) = make_uint4(word[0], word[1], word[2], word[3]);
}

// ---- the round trip: a wave per 64 bytes of the output
struct VcRt {
	uint32_t nH;
	uint64_t total;
	const uint64_t *hoff;
	const uint32_t *rt_path; // [nH] NO_QUERY: nothing to compare with
	const uint64_t *rt_pb, *rt_plen; // [nH] where the path begins in the flat buffer, its bases
	const uint8_t *flat, *out;
	unsigned long long *first_diff; // [nH] set to ~0
};
__global__ __launch_bounds__(Q_TPB) void k_vc_roundtrip(VcRt Y)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t waves = (uint64_t)gridDim.x * (Q_TPB / 64);
	for (uint64_t c0 = ((uint64_t)blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6)) * 64; c0 < Y.total; c0 += waves * 64) {
		const uint64_t g = c0 + lane;
		const bool in = g < Y.total;
		const uint32_t h0 = span_of(Y.hoff, Y.nH, c0);
		const uint32_t h = in ? h0 + span_of(Y.hoff + h0, Y.nH - h0, g) : h0;
		const uint64_t o = g - Y.hoff[h];
		const bool ne = in && Y.rt_path[h] != NO_QUERY && o < Y.rt_plen[h] && vm_fold((char)Y.out[g]) != vm_fold((char)Y.flat[Y.rt_pb[h] + o]);
		const uint32_t ph = __shfl_up(h, 1, 64);
		const bool pne = __shfl_up((uint32_t)ne, 1, 64) != 0;
		if (__ballot(ne) == 0)
			continue;
		if (ne && (lane == 0 || !pne || ph != h)) // (the lowest of a haplotype's differing bytes in this wave)
			atomicMin(Y.first_diff + h, (unsigned long long)o);
	}
}

// the third field of a PanSN name `a#b#rest`, null when it has none
const char *third_field(const char *name)
{
	const char *a = strchr(name, '#');
	const char *b = a ? strchr(a + 1, '#') : nullptr;
	return b ? b + 1 : nullptr;
}

struct ConsOwner {
	povu_hip_vcf_cons view{}; // first member: the owner is recovered from it in povu_hip_vcf_cons_free
	PinnedVec<uint8_t> block; // every array of the view, in one page-locked block (HostSpans)
};
struct NamesFree {
	void operator()(povu_hip_call_names *n) const { povu_hip_call_names_free(n); }
};
} // namespace

static povu_hip_vcf_cons *vcf_consensus(povu_hip_ctx *ctx, const povu_hip_vcf_doc *doc, const char *const *path_name, uint32_t n_paths,
					const povu_hip_vcf_cons_opts *opts, CallTimer &timer)
{
	const uint32_t flags = opts ? opts->flags : 0u;
	const bool force = flags & POVU_HIP_V_FORCE_TIER2, roundtrip = flags & POVU_HIP_C_ROUNDTRIP, no_text = flags & POVU_HIP_C_NO_TEXT,
		   time_write = flags & POVU_HIP_C_TIME_WRITE;
	const char *who = "the consensus needs ";
	static const uint64_t no_off[1] = {0};
	povu_hip_vcf_doc none{}; // the pair's second document: empty
	none.allele_off = none.task_off = none.text_off = no_off;
	PairWant want{};
	want.t_rec = want.t_al = want.t_col = want.t_ph = true;
	PairUpload U = pair_build(ctx, doc, doc ? &none : nullptr, who, want, POS_LIMIT);
	if (!ctx->g.block || !ctx->paths_valid || ctx->paths_gen != ctx->g.gen)
		throw HipError("the consensus needs the paths of the graph now uploaded (povu_hip_paths_upload after povu_hip_graph_upload)");
	if (!ctx->seq_valid || ctx->seq_gen != ctx->g.gen)
		throw HipError("the consensus needs the sequences of the graph now uploaded (povu_hip_segments_upload after povu_hip_graph_upload)");
	if (n_paths != ctx->n_paths)
		throw HipError(std::to_string(n_paths) + " path names for " + std::to_string(ctx->n_paths) + " resident paths");
	for (uint32_t k = 0; k < n_paths; k++)
		if (!path_name || !path_name[k])
			throw HipError("null path name");
	const uint32_t nR = U.nR, nAl = U.nAl, nT = U.nT, nI = U.nI, n_chroms = U.n_chroms, n_cols = U.n_cols_a, max_phase = U.max_phase, hbits = hash_bits_hook();

	// ---- the selection
	std::vector<uint8_t> h_chrom_sel((size_t)n_chroms + 1, 1), h_col_sel((size_t)n_cols + 1, 1);
	if (opts && opts->n_select && opts->select_col) {
		std::fill(h_col_sel.begin(), h_col_sel.end(), 0);
		for (uint32_t k = 0; k < opts->n_select; k++) {
			if (opts->select_col[k] >= n_cols)
				throw HipError("selected sample column " + std::to_string(opts->select_col[k]) + ": the document has " + std::to_string(n_cols));
			h_col_sel[opts->select_col[k]] = 1;
		}
	}
	if (opts && opts->n_select && opts->select_chrom) {
		std::fill(h_chrom_sel.begin(), h_chrom_sel.end(), 0);
		for (uint32_t k = 0; k < opts->n_select; k++) {
			if (opts->select_chrom[k] >= doc->n_chroms || !doc->chrom[opts->select_chrom[k]])
				throw HipError("selected CHROM " + std::to_string(opts->select_chrom[k]) + ": the document has " + std::to_string(doc->n_chroms));
			const auto at = std::find(U.chrom_name.begin(), U.chrom_name.end(), doc->chrom[opts->select_chrom[k]]);
			if (at != U.chrom_name.end()) // (interned by pair_build; a CHROM without a record has no id and no haplotype)
				h_chrom_sel[at - U.chrom_name.begin()] = 1;
		}
	}
	// ---- the listed paths: those the CHROMs name (a "reference index" over them, as the haplotype comparison builds it), then
	// the paths a round trip may read
	std::vector<uint32_t> h_chrom_ref((size_t)n_chroms + 1, NO_QUERY), h_list;
	std::vector<uint8_t> read_it; // per listed path: spelled into the flat buffer
	std::unordered_map<uint32_t, uint32_t> listed; // path -> its first place in the list
	{
		std::unordered_map<std::string, uint32_t> path_of; // (of several paths of one name the first counts)
		for (uint32_t k = 0; k < n_paths; k++)
			path_of.emplace(path_name[k], k);
		for (uint32_t c = 0; c < n_chroms; c++) {
			const auto at = path_of.find(U.chrom_name[c]);
			if (at == path_of.end())
				continue;
			h_chrom_ref[c] = (uint32_t)h_list.size();
			listed.emplace(at->second, (uint32_t)h_list.size());
			h_list.push_back(at->second), read_it.push_back(h_chrom_sel[c]);
		}
	}
	// the round trip's candidates per (column, phase): the paths of the slot; narrowed per CHROM by the third field
	std::unique_ptr<povu_hip_call_names, NamesFree> names;
	std::vector<uint32_t> col_first((size_t)n_cols + 1), col_slots((size_t)n_cols + 1);
	std::vector<std::vector<uint32_t>> slot_paths;
	auto candidates = [&](uint32_t c, uint32_t col, uint32_t j, uint32_t *path) { // how many (2: more than one), the only one
		if (j >= col_slots[col])
			return 0u;
		const char *want3 = third_field(U.chrom_name[c].c_str());
		uint32_t n = 0;
		for (uint32_t p : slot_paths[col_first[col] + j])
			if (!want3 || (third_field(path_name[p]) && !strcmp(third_field(path_name[p]), want3))) {
				*path = p;
				if (++n == 2)
					break;
			}
		return n;
	};
	if (roundtrip) {
		char msg[256] = {0};
		names.reset(povu_hip_vcf_names_make(n_paths, path_name, msg, sizeof msg));
		if (!names || povu_hip_vcf_columns(doc, names.get(), col_first.data(), col_slots.data()))
			throw HipError(std::string("the consensus's round trip: ") + (msg[0] ? msg : "the sample columns and the path names do not belong together"));
		slot_paths.resize((size_t)names->refs.n_slots + 1);
		for (uint32_t p = 0; p < n_paths; p++)
			slot_paths[names->slot_of_path[p]].push_back(p);
		for (uint32_t c = 0; c < n_chroms; c++)
			for (uint32_t col = 0; h_chrom_sel[c] && h_chrom_ref[c] != NO_QUERY && col < n_cols; col++)
				for (uint32_t j = 0; h_col_sel[col] && j < col_slots[col]; j++) {
					uint32_t p = 0;
					if (candidates(c, col, j, &p) != 1)
						continue;
					const auto ins = listed.emplace(p, (uint32_t)h_list.size());
					if (ins.second)
						h_list.push_back(p), read_it.push_back(1);
					else
						read_it[ins.first->second] = 1;
				}
	}
	const uint32_t nL = (uint32_t)h_list.size();
	auto o = std::make_unique<ConsOwner>();

	HIP_CHECK(hipSetDevice(ctx->device));
	ctx->wait_tail();
	hipStream_t s = U.s = ctx->stream;
	std::vector<uint64_t> path_off((size_t)n_paths + 1), h_ref_base(1, 0);
	HIP_CHECK(copy_async(path_off.data(), ctx->path_off, ((size_t)n_paths + 1) * 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	for (uint32_t p : h_list)
		h_ref_base.push_back(h_ref_base.back() + path_off[p + 1] - path_off[p]);
	const uint64_t NRs = h_ref_base.back();

	// ---- the layout of the workspace (vc_ws): what is uploaded and worked on, the haplotypes' arrays ([nT + 1]: a haplotype has
	// a task)
	const size_t r1 = (size_t)nR + 1, i1 = (size_t)nI + 1, t1 = (size_t)nT + 1, big = std::max({r1, i1, t1}) + 1, l1 = (size_t)nL + 1;
	uint32_t *aoff, *ioff, *chrom, *t_rec, *t_al, *t_col, *t_ph, *chrom_ref, *chrom_placed, *ref_path, *it_rec, *it_k, *suffix, *prefix, *t_len, *rq, *rlen, *t2,
		*firstf, *gidx, *gid, *place, *tk_chrom, *tk_item, *hidx, *h_x0, *h_chrom, *h_col, *h_phase, *h_e0, *h_napp, *h_ndup, *h_nenc, *h_novl, *h_nuns,
		*h_nnoc, *k_item, *rt_path, *words;
	uint64_t *toff, *pos, *ref_base, *ref_len, *roff, *s64, *bs, *be, *t_at, *rhash, *sp_lo, *sp_hi, *plen, *foff, *h_len, *h_off, *h_fb, *k_start, *rt_pb, *rt_plen;
	unsigned long long *cnt, *splits, *rt_first;
	uint8_t *placed, *state, *keep, *tk_kind, *chrom_sel, *col_sel;
	char *text;
	GroupWs gw;
	gw.tmp_bytes = prim_tmp_bytes(big + 1, true) + 256;
	const size_t s64_words = scan_exclusive_u64_tmp(std::max<size_t>((size_t)NRs + 1, t1));
	timer.start(s);
	carve(ctx->vc_ws, [&](Spans &take) {
		take(r1, aoff, ioff, chrom);
		take(r1, pos, sp_lo, sp_hi);
		take(r1, placed);
		take((size_t)nAl + 1, toff);
		take(U.n_text + 1, text);
		take(t1, t_rec, t_al, t_col, t_ph, tk_chrom, tk_item, hidx, h_x0, h_chrom, h_col, h_phase, h_e0, h_napp, h_ndup, h_nenc, h_novl, h_nuns, h_nnoc, k_item,
		     rt_path);
		take(t1, h_len, h_off, h_fb, k_start, rt_pb, rt_plen);
		take(t1, rt_first);
		take(t1, tk_kind);
		take((size_t)n_cols + 1, col_sel);
		take((size_t)n_chroms + 1, chrom_sel);
		take((size_t)n_chroms + 1, chrom_ref, chrom_placed);
		take(l1, ref_path);
		take(l1, ref_base, plen, foff);
		take((size_t)NRs + 1, ref_len, roff);
		take(s64_words, s64);
		take(i1, it_rec, it_k, suffix, prefix, t_len, rq, rlen, t2, firstf, gid, place, gw.head, gw.rep, gw.blist);
		take(i1 + 1, gidx);
		take(i1, bs, be, t_at, rhash);
		take(i1, state, keep, gw.rbad);
		take(big, gw.pa, gw.pb, gw.key, gw.kout, gw.mark, gw.hmax);
		take(8, words);
		take(CN_WORDS, cnt);
		take(1, splits);
		take(gw.tmp_bytes, gw.tmp);
	});
	U.up(aoff, U.aoff), U.up(ioff, U.ioff), U.up(chrom, U.chrom), U.up(pos, U.pos), U.up(toff, U.toff);
	U.up_text(text);
	U.up(t_rec, U.t_rec), U.up(t_al, U.t_al), U.up(t_col, U.t_col), U.up(t_ph, U.t_ph);
	U.up(chrom_ref, h_chrom_ref), U.up(ref_path, h_list), U.up(ref_base, h_ref_base), U.up(chrom_sel, h_chrom_sel), U.up(col_sel, h_col_sel);
	HIP_CHECK(hipMemsetAsync(words, 0, 32, s));
	HIP_CHECK(hipMemsetAsync(cnt, 0, CN_WORDS * 8, s));
	HIP_CHECK(hipMemsetAsync(chrom_placed, 0, ((size_t)n_chroms + 1) * 4, s));

	// ---- the listed paths' base offsets and lengths; where each read path lies in the flat buffer; placement
	const PathsView P = paths_view(ctx);
	const RefView R{NRs, nL, nullptr, ref_path, ref_base, roff};
	const VhRef F{1u, chrom_ref, R, P};
	HIP_CHECK(hipMemsetAsync(ref_len + NRs, 0, 8, s));
	if (NRs)
		launch_ref_len(R, P, ref_len, s);
	scan_exclusive_u64(ref_len, roff, NRs + 1, s64, s);
	std::vector<uint64_t> h_plen(l1, 0), h_foff(l1, 0);
	if (nL) {
		KLAUNCH(k_vc_path_len, dim3(stride_blocks(nL)), dim3(Q_TPB), 0, s, R, plen);
		HIP_CHECK(copy_async(h_plen.data(), plen, (size_t)nL * 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
	}
	for (uint32_t l = 0; l < nL; l++)
		h_foff[l + 1] = h_foff[l] + (read_it[l] ? h_plen[l] : 0);
	const uint64_t NF = h_foff[nL];
	U.up(foff, h_foff);
	const PairView A{nR, nR, nI, nI, aoff, ioff, toff, text, pos, chrom, it_rec, it_k};
	const EditPolicy E{{state, keep, bs, be, t_at, t_len, suffix, prefix, rq, rlen, rhash, ((uint64_t)hash_mask_hi(hbits) << 32) | hash_mask_lo(hbits), n_chroms, placed}};
	uint32_t n_t2 = 0, nG = 0, nV = 0, nH = 0;
	uint64_t n_splits = 0, total = 0, n_placed = 0;
	if (nR) {
		KLAUNCH(k_vh_place, dim3(std::min(stride_blocks(nR), COUNT_BLOCKS)), dim3(Q_TPB), 0, s, A, F, placed, sp_lo, sp_hi, cnt);
		KLAUNCH(k_vc_chrom_placed, dim3(stride_blocks(nR)), dim3(Q_TPB), 0, s, nR, placed, chrom, chrom_placed);
	}
	// ---- items, edits, groups, the items' order
	if (nI) {
		n_t2 = launch_tiers(A, E, force, t2, words + 1, s);
		const uint32_t *sp = group_exact(nI, rq, rlen, rhash, hbits, bits_for(U.longest), bits_for(n_chroms), SameEdit{text, state, bs, be, t_at, t_len}, gw,
						 words + 2, splits, &n_splits, s);
		number_groups(nI, sp, gw.rep, firstf, gidx, keep, gw.tmp, gw.tmp_bytes, s);
		nG = read_back(gidx + nI, s);
		KLAUNCH(k_eg_group_of, dim3(stride_blocks(nI)), dim3(Q_TPB), 0, s, nI, sp, gw.rep, gidx, keep, gid);
		launch_iota(nI, gw.pa, s);
		LsdSort sort{gw.pa, gw.pb, gw.key, gw.kout, nI, gw.tmp, gw.tmp_bytes, s};
		auto key = [&](int which, const uint32_t *cur, uint32_t *k) {
			KLAUNCH(k_vc_item_key, dim3(stride_blocks(nI)), dim3(Q_TPB), 0, s, nI, which, nG, cur, gid, bs, be, k);
		};
		for (int which = 0; which < VC_SORT_PASSES; which++)
			sort.pass(which, vc_sort_bits(which, bits_for(nG)), key);
		KLAUNCH(k_vc_inverse, dim3(stride_blocks(nI)), dim3(Q_TPB), 0, s, nI, sort.cur, place);
	}
	// ---- the tasks that take part; the haplotypes
	VcTasks K{nT, 0, t_rec, t_al, t_col, t_ph, tk_chrom, tk_item, tk_kind};
	if (nT) {
		KLAUNCH(k_vc_tasks, dim3(std::min(stride_blocks(nT), COUNT_BLOCKS)), dim3(Q_TPB), 0, s, A, K, n_chroms, chrom_sel, col_sel, placed, state, cnt);
		nV = (uint32_t)read_back(cnt + CN_TASKS, s);
	}
	VcHaps H{0, h_x0, h_chrom, h_col, h_phase, h_e0, h_napp, h_ndup, h_nenc, h_novl, h_nuns, h_nnoc, h_len, h_fb, k_item, k_start};
	if (nV) {
		K.nV = nV;
		const size_t v1 = (size_t)nV + 1;
		launch_iota(nT, gw.pa, s);
		LsdSort sort{gw.pa, gw.pb, gw.key, gw.kout, nT, gw.tmp, gw.tmp_bytes, s};
		auto key = [&](int which, const uint32_t *cur, uint32_t *k) {
			KLAUNCH(k_vc_task_key, dim3(stride_blocks(nT)), dim3(Q_TPB), 0, s, K, which, cur, place, k);
		};
		sort.pass(0, bits_for(nI), key);
		sort.pass(1, 2, key);
		sort.pass(2, bits_for(max_phase), key);
		sort.pass(3, bits_for(n_cols), key);
		sort.pass(4, bits_for(n_chroms), key);
		const uint32_t *sorted = sort.cur;
		uint32_t *head = gw.key; // (the sort's key buffer is free again)
		KLAUNCH(k_vc_heads, dim3(stride_blocks(v1)), dim3(Q_TPB), 0, s, K, sorted, head);
		scan_exclusive_u32(head, hidx, v1, gw.tmp, gw.tmp_bytes, s);
		H.n = nH = read_back(hidx + nV, s);
		KLAUNCH(k_vc_open, dim3(stride_blocks(v1)), dim3(Q_TPB), 0, s, K, H, sorted, head, hidx);
		const VcLists Y{sorted, tk_kind, tk_item, gid, bs, be, t_len, chrom_ref, chrom_placed, plen, foff};
		KLAUNCH(k_vc_lists, dim3(wave_blocks(nH)), dim3(Q_TPB), 0, s, H, Y);
	}
	HIP_CHECK(hipMemsetAsync(h_len + nH, 0, 8, s));
	scan_exclusive_u64(h_len, h_off, (size_t)nH + 1, s64, s);
	total = read_back(h_off + nH, s);
	if (total >= OUT_LIMIT)
		throw HipError(std::string(who) + std::to_string(total) + " output bytes for " + std::to_string(nH) +
			       " haplotypes: 2^32 - 64 or more are refused; select fewer sample columns or CHROMs per call (povu_hip_vcf_cons_opts)");

	// ---- the round trip's paths, haplotype by haplotype
	const size_t n1 = (size_t)nH + 1;
	std::vector<uint32_t> v_chrom(n1), v_col(n1), v_phase(n1), v_path(n1, NO_QUERY);
	std::vector<uint64_t> v_pb(n1, 0), v_plen(n1, 0);
	std::vector<uint8_t> v_status(n1, POVU_HIP_C_RT_NONE);
	if (roundtrip && nH) {
		HIP_CHECK(copy_async(v_chrom.data(), h_chrom, (size_t)nH * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(v_col.data(), h_col, (size_t)nH * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(v_phase.data(), h_phase, (size_t)nH * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		for (uint32_t h = 0; h < nH; h++) {
			uint32_t p = 0;
			const uint32_t n = candidates(v_chrom[h], v_col[h], v_phase[h], &p);
			v_status[h] = n == 0 ? POVU_HIP_C_RT_NO_PATH : n > 1 ? POVU_HIP_C_RT_AMBIGUOUS : POVU_HIP_C_RT_EQUAL;
			if (n == 1) {
				const uint32_t l = listed.at(p); // (listed above: the haplotype's CHROM and column are selected)
				v_path[h] = p, v_pb[h] = h_foff[l], v_plen[h] = h_plen[l];
			}
		}
	}
	// ---- the second arena (vc_hit): the flat spelling and the output
	uint8_t *flat, *out;
	const uint64_t out_room = ((total + 15) & ~15ull) + 16;
	carve(ctx->vc_hit, [&](Spans &take) {
		take(NF + 32, flat);
		take(out_room, out);
	});
	if (NF)
		KLAUNCH(k_vc_spell, dim3(stride_blocks(NF)), dim3(Q_TPB), 0, s, NF, R, P, foff, flat);
	HIP_CHECK(hipMemsetAsync(flat + NF, 0, 32, s));
	float write_ms = 0;
	if (total) {
		CallTimer writing; // (the materialiser alone, on request: what tools/time_consensus.py holds against a device-to-device copy)
		if (time_write)
			writing.start(s);
		const VcMat M{nH, total, h_off, h_e0, h_napp, h_fb, k_item, k_start, be, t_at, t_len, text, flat, out};
		const uint64_t tiles = (total + POVU_HIP_C_TILE_BYTES - 1) / POVU_HIP_C_TILE_BYTES; // (below 2^20)
		KLAUNCH(k_vc_materialise, dim3((unsigned)tiles), dim3(Q_TPB), 0, s, M);
		if (time_write)
			write_ms = writing.stop(s); // (waits for the stream)
	}
	HIP_CHECK(hipMemsetAsync(rt_first, 0xFF, n1 * 8, s));
	if (roundtrip && total) {
		U.up(rt_path, v_path.data(), (size_t)nH * 4), U.up(rt_pb, v_pb.data(), (size_t)nH * 8), U.up(rt_plen, v_plen.data(), (size_t)nH * 8);
		const VcRt Y{nH, total, h_off, rt_path, rt_pb, rt_plen, flat, out, rt_first};
		KLAUNCH(k_vc_roundtrip, dim3(wave_blocks((total + 63) / 64)), dim3(Q_TPB), 0, s, Y);
	}

	// ---- to the host
	povu_hip_vcf_cons &v = o->view;
	uint64_t *r_first = nullptr, *r_plen = nullptr;
	const uint64_t *r_len = nullptr;
	uint8_t *r_status = nullptr;
	uint32_t *r_path = nullptr;
	uint64_t h_cnt[CN_WORDS] = {0};
	static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the arrays are read as uint64_t");
	auto results = [&](HostSpans &take) {
		v.hap_chrom = take(h_chrom, nH, n1), v.hap_col = take(h_col, nH, n1), v.hap_phase = take(h_phase, nH, n1);
		v.hap_len = r_len = take(h_len, nH, n1), v.hap_off = take(h_off, nH, n1);
		v.n_applied = take(h_napp, nH, n1), v.n_duplicate = take(h_ndup, nH, n1), v.n_enclosed = take(h_nenc, nH, n1);
		v.n_overlap = take(h_novl, nH, n1), v.n_unspelled = take(h_nuns, nH, n1), v.n_nocall = take(h_nnoc, nH, n1);
		v.rt_first_diff = r_first = take(reinterpret_cast<uint64_t *>(rt_first), nH, n1);
		v.rt_path_len = r_plen = take(static_cast<uint64_t *>(nullptr), 0, n1);
		v.rt_path = r_path = take(static_cast<uint32_t *>(nullptr), 0, n1);
		v.rt_status = r_status = take(static_cast<uint8_t *>(nullptr), 0, n1);
		v.text = no_text ? nullptr : reinterpret_cast<const char *>(take(out, total, total + 1));
	};
	hand_off_block(o->block, ctx, results);
	HIP_CHECK(copy_async(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, s));
	v.device_ms = timer.stop(s);
	n_placed = h_cnt[CN_PLACED_A];
	for (uint32_t h = 0; h < nH; h++) {
		r_path[h] = v_path[h] == NO_QUERY ? POVU_HIP_NIL : v_path[h], r_plen[h] = v_plen[h], r_status[h] = v_status[h];
		if (v_status[h] != POVU_HIP_C_RT_EQUAL) {
			r_first[h] = ~0ull;
			continue;
		}
		if (r_first[h] == ~0ull && r_len[h] != v_plen[h])
			r_first[h] = std::min(r_len[h], v_plen[h]); // (one is a prefix of the other)
		if (r_first[h] != ~0ull)
			r_status[h] = POVU_HIP_C_RT_DIFFER;
	}
	v.n_haps = nH, v.n_text_bytes = total, v.n_unplaced = nR - n_placed, v.n_tier2 = n_t2, v.roundtrip = roundtrip, v.write_ms = write_ms;
	return &o.release()->view;
}

} // namespace povu_hip

// ---- C ABI

extern "C" povu_hip_vcf_cons *povu_hip_vcf_consensus(povu_hip_ctx *ctx, const povu_hip_vcf_doc *doc, const char *const *path_name, uint32_t n_paths,
						     const povu_hip_vcf_cons_opts *opts, char *err, size_t errlen)
{
	using namespace povu_hip;
	CallTimer timer;
	return guarded_call(ctx, err, errlen, (povu_hip_vcf_cons *)nullptr, [&] { return vcf_consensus(ctx, doc, path_name, n_paths, opts, timer); });
}
extern "C" void povu_hip_vcf_cons_free(povu_hip_vcf_cons *c)
{
	delete reinterpret_cast<povu_hip::ConsOwner *>(c);
}
