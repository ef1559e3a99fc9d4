// vcfhap_kernels.hip -- povu_hip_vcf_haplotypes (include/povu_hip.h): per region, sample and phase, do two parsed VCFs spell
// the same bases?
//
// The definition is INTEGRATION.md "Haplotype comparison" (restated in tests/vcfhap_ref.py; the rules that are plain arithmetic
// are vcfhap_rules.hpp).  Both documents are uploaded as one (vcf_pair.hpp: the host builder, the view, the items).
// Coordinates on the device carry one more than the 0-based value (bs, be, lo, hi: POS names base POS), so that POS 0 has no
// negative start; the host takes the one off.
//   place    a lane per record: placed or not, its span [POS, POS + |REF|) (vcfhap_edits.hpp, shared with the consensus);
//   edits    the skip rule, the full trim and the hash of (s, e, T): the two tiers of vcf_pair.hpp over EditPolicy
//            (vcfhap_edits.hpp), which settles the items of unplaced records first, trims to vh_trim_limit, hashes T and
//            writes an edit or none;
//   reach    reference mode: a wave per indel edit, 64 reference bases a ballot to the right, then to the left, through a
//            RefView over the CHROM paths (launch_ref_len + scan_exclusive_u64); the record's span is widened by atomics;
//   groups   exact_groups.hpp over (CHROM id, |T|, hash), the comparison the bytes of T with s and e, the groups of the items
//            with an edit numbered in first-item order (number_groups); the items then sorted
//            by (s, e, group): an item's place in that order is what its tasks sort by;
//   windows  the records sorted by (CHROM, span start); every span bisects for the last span that starts at or before its end,
//            an exclusive running maximum of those marks the heads, scans give the window ids and the text offsets;
//   text     lanes over the bytes from the path, or a wave per record from its REF (the greatest folded byte of those that
//            cover a base: whichever writer comes last, the text is the same); a wave per record verifies and flags;
//   cells    the tasks sorted by (window, common sample, phase, side, kind, the item's place); heads give the cells, a scan of
//            |T| - (e - s) over the distinct edits gives every edit's place in its haplotype (sums modulo 2^64);
//   replay   a wave per cell: the conflicts by a chunked wave max-scan of the ends with a carry, then 64 haplotype bytes a
//            ballot on both sides, a lane finding its byte by bisection over the side's edit positions.  Nothing is materialised.
// Every shuffle and ballot runs with all 64 lanes (trip counts around them are wave-uniform); every store is inside the range
// the host carved: records below nR, items below nI, windows below nW <= nR, tasks, cells and distinct edits below nV <= nT.
#include "vcfhap_edits.hpp"

#include <unordered_map>

namespace povu_hip
{

namespace
{

// ---- reach: a wave per item (those that are no indel edit pass), reference mode only
__global__ __launch_bounds__(Q_TPB) void k_vh_reach(PairView A, VhEdits O, VhRef F, uint32_t max_reach, uint32_t *__restrict__ left,
						     uint32_t *__restrict__ right, unsigned long long *__restrict__ sp_lo,
						     unsigned long long *__restrict__ sp_hi, unsigned long long *__restrict__ cnt)
{
	const LaneWave w{threadIdx.x & 63u};
	const uint32_t lane = w.lane, waves = gridDim.x * (Q_TPB / 64);
	const uint64_t limit = (uint64_t)max_reach + 1; // (one step beyond the cap tells a capped reach from one that ends at it)
	for (uint32_t i = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); i < A.nI; i += waves) {
		if (O.state[i] != POVU_HIP_H_EDIT)
			continue;
		const uint64_t bs = O.bs[i], be = O.be[i], tl = O.t_len[i];
		if (!vh_has_reach(bs, be, tl))
			continue;
		const uint32_t r = A.record_of(i), c = F.chrom_ref[A.chrom[r]]; // (the record is placed: c is a reference)
		const uint64_t plen = F.path_len(c), s0 = bs - 1, e0 = be - 1;
		const char *unit = bs == be ? A.text + O.t_at[i] : A.text + A.toff[A.aoff[r]] + O.prefix[i];
		const uint64_t m = bs == be ? tl : be - bs;
		const uint64_t kr = wave_first(limit, w, [&](uint64_t x) { return !(e0 + x < plen && vh_reach_right_ok(unit, m, x, F.base(c, e0 + x))); });
		const uint64_t kl = wave_first(limit, w, [&](uint64_t x) { return !(x < s0 && vh_reach_left_ok(unit, m, x, F.base(c, s0 - 1 - x))); });
		if (lane == 0) {
			const uint32_t l = (uint32_t)min(kl, (uint64_t)max_reach), rt = (uint32_t)min(kr, (uint64_t)max_reach);
			left[i] = l, right[i] = rt;
			if (kl > max_reach || kr > max_reach)
				atomicAdd(cnt + CN_CAPPED, 1ull);
			if (l)
				atomicMin(sp_lo + r, (unsigned long long)(bs - l));
			if (rt)
				atomicMax(sp_hi + r, (unsigned long long)(be + rt));
		}
	}
}

// the items' order by (s, e, group): which = 0 group, 1 / 2 e's low and high word, 3 / 4 s's
__global__ void k_vh_item_key(uint32_t n, int which, uint32_t nG, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ gid,
			      const uint64_t *__restrict__ bs, const uint64_t *__restrict__ be, uint32_t *__restrict__ key)
{
	for (uint32_t x = blockIdx.x * Q_TPB + threadIdx.x; x < n; x += gridDim.x * Q_TPB) {
		const uint32_t i = perm[x];
		const uint64_t v = which >= 3 ? bs[i] : be[i];
		key[x] = which == 0 ? min(gid[i], nG) : (which & 1) ? (uint32_t)v : (uint32_t)(v >> 32);
	}
}
__global__ void k_vh_inverse(uint32_t n, const uint32_t *__restrict__ perm, uint32_t *__restrict__ place)
{
	for (uint32_t x = blockIdx.x * Q_TPB + threadIdx.x; x < n; x += gridDim.x * Q_TPB)
		place[perm[x]] = x;
}

// ---- windows
// the records' order by (CHROM, span start), the unplaced ones behind: which = 0 / 1 the start's low and high word, 2 CHROM
__global__ void k_vh_span_key(uint32_t n, int which, uint32_t n_chroms, const uint32_t *__restrict__ perm, const uint8_t *__restrict__ placed,
			      const uint32_t *__restrict__ chrom, const uint64_t *__restrict__ sp_lo, uint32_t *__restrict__ key)
{
	for (uint32_t x = blockIdx.x * Q_TPB + threadIdx.x; x < n; x += gridDim.x * Q_TPB) {
		const uint32_t r = perm[x];
		key[x] = which == 0 ? (uint32_t)sp_lo[r] : which == 1 ? (uint32_t)(sp_lo[r] >> 32) : placed[r] ? chrom[r] : n_chroms;
	}
}
// mark[k] = 1 + the last sorted span that starts at or before the end of span k, on its CHROM (touching spans share a window)
__global__ void k_vh_span_reach(uint32_t nP, const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ chrom, const uint64_t *__restrict__ sp_lo,
				const uint64_t *__restrict__ sp_hi, uint32_t *__restrict__ mark)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < nP; k += gridDim.x * Q_TPB) {
		const uint32_t r = sorted[k], c = chrom[r];
		const uint64_t end = sp_hi[r];
		// (span k itself starts before its end; behind k the CHROM ids ascend: another CHROM is a greater one)
		mark[k] = 1 + last_upto(k, nP, [=](uint32_t m) { return chrom[sorted[m]] == c && sp_lo[sorted[m]] <= end; });
	}
}
__global__ void k_vh_heads(uint32_t nP, const uint32_t *__restrict__ reached, uint32_t *__restrict__ headf)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k <= nP; k += gridDim.x * Q_TPB)
		headf[k] = k < nP && vh_window_head(reached[k], k);
}
struct VhWindows {
	uint32_t *chrom, *n_a, *n_b, *offender;
	unsigned long long *lo, *hi;
	uint8_t *bad;
};
// (hi, n_a, n_b cleared before the launch)
__global__ void k_vh_windows(uint32_t nP, uint32_t nRa, const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ widx,
			     const uint32_t *__restrict__ headf, const uint32_t *__restrict__ chrom, const uint64_t *__restrict__ sp_lo,
			     const uint64_t *__restrict__ sp_hi, uint32_t *__restrict__ rec_window, VhWindows W)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < nP; k += gridDim.x * Q_TPB) {
		const uint32_t r = sorted[k], w = widx[k] + headf[k] - 1; // (span 0 is a head: w >= 0)
		rec_window[r] = w;
		if (headf[k])
			W.chrom[w] = chrom[r], W.lo[w] = sp_lo[r];
		atomicMax(W.hi + w, (unsigned long long)sp_hi[r]);
		atomicAdd((r < nRa ? W.n_a : W.n_b) + w, 1u);
	}
}
__global__ void k_vh_window_len(uint32_t nW, VhWindows W, uint64_t *__restrict__ wlen)
{
	for (uint32_t w = blockIdx.x * Q_TPB + threadIdx.x; w <= nW; w += gridDim.x * Q_TPB)
		wlen[w] = w < nW ? W.hi[w] - W.lo[w] : 0;
}

// ---- the windows' text
__global__ void k_vh_fill_ref(uint64_t total, uint32_t nW, const uint64_t *__restrict__ woff, VhWindows W, VhRef F, uint8_t *__restrict__ wtext)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x < total; x += (uint64_t)gridDim.x * Q_TPB) {
		const uint32_t w = span_of(woff, nW, x);
		wtext[x] = F.base(F.chrom_ref[W.chrom[w]], W.lo[w] - 1 + (x - woff[w])); // (inside the path: every span of the window is)
	}
}
// a wave per placed record: its folded REF into the text, the greater byte standing (the text's words are cleared first)
__global__ __launch_bounds__(Q_TPB) void k_vh_fill_rec(PairView A, const uint8_t *__restrict__ placed, const uint32_t *__restrict__ rec_window,
							const uint64_t *__restrict__ woff, VhWindows W, uint32_t *__restrict__ words)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	for (uint32_t r = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); r < A.nR; r += waves) {
		if (!placed[r])
			continue;
		const uint32_t w = rec_window[r];
		const uint64_t nr = A.ref_len(r), at = woff[w] + (A.pos[r] - W.lo[w]);
		const char *ref = A.text + A.toff[A.aoff[r]];
		for (uint64_t i = lane; i < nr; i += 64) {
			const uint32_t v = vm_fold(ref[i]), shift = (uint32_t)((at + i) & 3u) * 8u;
			uint32_t *word = words + ((at + i) >> 2);
			uint32_t old = *word;
			while (((old >> shift) & 0xFFu) < v) {
				const uint32_t seen = atomicCAS(word, old, (old & ~(0xFFu << shift)) | (v << shift));
				if (seen == old)
					break;
				old = seen;
			}
		}
	}
}
// a wave per placed record: a REF field that differs from the text at its place makes the window inconsistent
__global__ __launch_bounds__(Q_TPB) void k_vh_verify(PairView A, const uint8_t *__restrict__ placed, const uint32_t *__restrict__ rec_window,
						      const uint64_t *__restrict__ woff, VhWindows W, const uint8_t *__restrict__ wtext)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	for (uint32_t r = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); r < A.nR; r += waves) {
		if (!placed[r])
			continue;
		const uint32_t w = rec_window[r];
		const uint64_t nr = A.ref_len(r), at = woff[w] + (A.pos[r] - W.lo[w]);
		const char *ref = A.text + A.toff[A.aoff[r]];
		bool differs = false;
		for (uint64_t c0 = 0; !differs && c0 < nr; c0 += 64)
			differs = __ballot(c0 + lane < nr && vm_fold(ref[c0 + lane]) != wtext[at + c0 + lane]) != 0;
		if (differs && lane == 0) {
			W.bad[w] = 1;
			atomicMin(W.offender + w, r);
		}
	}
}
__global__ __launch_bounds__(Q_TPB) void k_vh_count_bad(uint32_t nW, const uint8_t *__restrict__ bad, unsigned long long *__restrict__ cnt)
{
	const uint32_t lane = threadIdx.x & 63u;
	unsigned long long n = 0;
	for (uint64_t b = ((uint64_t)blockIdx.x * Q_TPB + threadIdx.x) & ~63ull; b < nW; b += (uint64_t)gridDim.x * Q_TPB)
		n += __popcll(__ballot(b + lane < nW && bad[b + lane]));
	if (lane == 0 && n)
		atomicAdd(cnt + CN_BAD_WINDOWS, n);
}

// ---- the tasks
struct VhTasks {
	uint32_t nT, nV; // tasks, those that take part (the first nV of the sorted list)
	const uint32_t *t_rec, *t_al, *t_col, *t_ph; // [nT] uploaded: the record over both documents, the allele, the column, the phase
	uint32_t *win, *smp, *item;		      // [nT] window (nW: takes no part), common sample, item of a KIND_EDIT task
	uint8_t *sk;				      // [nT] side << 2 | kind
};
__global__ __launch_bounds__(Q_TPB) void k_vh_tasks(PairView A, VhTasks K, uint32_t nW, uint32_t n_cols_a, const uint32_t *__restrict__ colmap,
						     const uint8_t *__restrict__ placed, const uint32_t *__restrict__ rec_window,
						     const uint8_t *__restrict__ state, unsigned long long *__restrict__ cnt)
{
	const uint32_t lane = threadIdx.x & 63u;
	unsigned long long n = 0;
	for (uint64_t b = ((uint64_t)blockIdx.x * Q_TPB + threadIdx.x) & ~63ull; b < K.nT; b += (uint64_t)gridDim.x * Q_TPB) {
		const uint64_t t = b + lane;
		bool valid = false;
		if (t < K.nT) {
			const uint32_t r = K.t_rec[t], side = r >= A.nRa, x = colmap[K.t_col[t] + (side ? n_cols_a : 0u)], al = K.t_al[t];
			valid = placed[r] && x != NO_QUERY;
			uint32_t kind = KIND_REF, item = 0;
			if (al) {
				const uint32_t i0 = A.ioff[r], n_alts = A.ioff[r + 1] - i0;
				kind = al <= n_alts && state[i0 + al - 1] == POVU_HIP_H_EDIT ? KIND_EDIT : KIND_UNSPELLED;
				item = kind == KIND_EDIT ? i0 + al - 1 : 0;
			}
			K.win[t] = valid ? rec_window[r] : nW, K.smp[t] = valid ? x : 0, K.item[t] = item, K.sk[t] = (uint8_t)(side << 2 | kind);
		}
		n += __popcll(__ballot(valid));
	}
	if (lane == 0 && n)
		atomicAdd(cnt + CN_TASKS, n);
}
// which = 0 the item's place in the (s, e, group) order, 1 side and kind, 2 phase, 3 common sample, 4 window
__global__ void k_vh_task_key(VhTasks K, int which, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ place, uint32_t *__restrict__ key)
{
	for (uint32_t x = blockIdx.x * Q_TPB + threadIdx.x; x < K.nT; x += gridDim.x * Q_TPB) {
		const uint32_t t = perm[x];
		key[x] = which == 0 ? ((K.sk[t] & 3u) == KIND_EDIT ? place[K.item[t]] : 0u) : which == 1 ? K.sk[t] : which == 2 ? K.t_ph[t] : which == 3 ? K.smp[t] : K.win[t];
	}
}
// per sorted task x <= nV: does it open a cell, is it the first of its edit on its side, and by how much that edit changes
// the length
__global__ void k_vh_task_heads(VhTasks K, const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ gid, const uint64_t *__restrict__ bs,
				const uint64_t *__restrict__ be, const uint32_t *__restrict__ t_len, uint32_t *__restrict__ chead,
				uint32_t *__restrict__ uniq, uint64_t *__restrict__ delta)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x <= K.nV; x += (uint64_t)gridDim.x * Q_TPB) {
		uint32_t head = 0, uq = 0;
		uint64_t d = 0;
		if (x < K.nV) {
			const uint32_t t = sorted[x], p = x ? sorted[x - 1] : 0;
			const bool same_cell = x && K.win[t] == K.win[p] && K.smp[t] == K.smp[p] && K.t_ph[t] == K.t_ph[p];
			head = !same_cell;
			if ((K.sk[t] & 3u) == KIND_EDIT) {
				const uint32_t i = K.item[t];
				uq = !(same_cell && K.sk[p] == K.sk[t] && gid[K.item[p]] == gid[i]);
				d = uq ? (uint64_t)t_len[i] - (be[i] - bs[i]) : 0; // (modulo 2^64)
			}
		}
		chead[x] = head, uniq[x] = uq, delta[x] = d;
	}
}
struct VhCells {
	uint32_t n, nV;
	uint32_t *x0;		       // [n + 1] first sorted task of a cell
	uint32_t *window, *sample, *phase, *edits_a, *edits_b;
	uint8_t *status;
	unsigned long long *len_a, *len_b, *first_diff;
	uint32_t *u_item;	       // [distinct edits] the item, and
	uint64_t *u_key;	       // the length changes in front of it over the whole list + its s
};
__global__ void k_vh_cells(VhTasks K, VhCells C, const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ chead, const uint32_t *__restrict__ cidx,
			   const uint32_t *__restrict__ uniq, const uint32_t *__restrict__ uidx, const uint64_t *__restrict__ dpos,
			   const uint64_t *__restrict__ bs)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x <= K.nV; x += (uint64_t)gridDim.x * Q_TPB) {
		if (x == K.nV) {
			C.x0[C.n] = K.nV;
			continue;
		}
		const uint32_t t = sorted[x];
		if (chead[x]) {
			const uint32_t c = cidx[x]; // (below the number of heads: C.n)
			C.x0[c] = (uint32_t)x, C.window[c] = K.win[t], C.sample[c] = K.smp[t], C.phase[c] = K.t_ph[t];
		}
		if (uniq[x]) {
			const uint32_t u = uidx[x];
			C.u_item[u] = K.item[t], C.u_key[u] = dpos[x] + bs[K.item[t]];
		}
	}
}

// ---- replay: a wave per cell
struct VhReplay {
	const uint32_t *sorted;
	const uint8_t *sk;
	const uint32_t *uidx;	// [nV + 1] distinct edits in front of a sorted task
	const uint64_t *dpos;	// [nV + 1] their length changes
	const uint64_t *bs, *be, *t_at;
	const uint32_t *t_len;
	const char *text;
	const uint64_t *woff;
	const uint8_t *wtext;
	unsigned long long *sample_status; // [nC * POVU_HIP_H_N_STATUS]
};
// the first sorted task of [lo, hi) whose (side, kind) is v or more
__device__ __forceinline__ uint32_t first_of_kind(const VhReplay &Y, uint32_t lo, uint32_t hi, uint32_t v)
{
	return first_not(lo, hi, [&](uint32_t k) { return Y.sk[Y.sorted[k]] < v; });
}
// the distinct edits [u0, u1) of a side, in (s, e) order: does one conflict with those in front of it?
__device__ __forceinline__ bool side_conflict(const VhCells &C, const VhReplay &Y, uint32_t u0, uint32_t u1, uint32_t lane)
{
	uint64_t carry_end = 0, carry_bs = 0, carry_be = 0; // of the chunks in front (an end is 1 at least: 0 is below all)
	bool conflict = false;
	for (uint32_t c0 = u0; !conflict && c0 < u1; c0 += 64) {
		const uint32_t u = c0 + lane;
		const bool in = u < u1;
		const uint32_t i = in ? C.u_item[u] : 0;
		const uint64_t bs = in ? Y.bs[i] : 0, be = in ? Y.be[i] : 0;
		const uint64_t incl = wave_inclusive_scan(be, ScanOp<1>{});
		uint64_t before = __shfl_up((unsigned long long)incl, 1, 64), pbs = __shfl_up((unsigned long long)bs, 1, 64),
			 pbe = __shfl_up((unsigned long long)be, 1, 64);
		if (lane == 0)
			before = 0, pbs = carry_bs, pbe = carry_be;
		before = max(before, carry_end);
		conflict = __ballot(in && vh_conflict(bs, be, u > u0, before, pbs, pbe)) != 0;
		carry_end = max(carry_end, (uint64_t)__shfl((unsigned long long)incl, 63, 64));
		carry_bs = __shfl((unsigned long long)bs, 63, 64), carry_be = __shfl((unsigned long long)be, 63, 64);
	}
	return conflict;
}
// a side's haplotype: the window's text [0, wl) with the distinct edits [u0, u0 + n) applied
struct VhSide {
	uint32_t u0, n;
	uint64_t base; // the length changes in front of the side's first edit + the window's lo: start(u) = u_key[u0 + u] - base
	uint64_t len;
};
__device__ __forceinline__ uint8_t side_byte(const VhCells &C, const VhReplay &Y, const VhSide &S, const uint8_t *__restrict__ wt, uint64_t wl, uint64_t blo,
					     uint64_t h)
{
	const uint32_t k = vh_locate(h, S.n, [&](uint32_t u) { return C.u_key[S.u0 + u] - S.base; });
	VhSource src{false, h};
	const char *t = nullptr;
	if (k != S.n) {
		const uint32_t i = C.u_item[S.u0 + k];
		src = vh_source(h, false, C.u_key[S.u0 + k] - S.base, Y.t_len[i], Y.be[i] - blo);
		t = Y.text + Y.t_at[i];
	}
	if (src.from_edit)
		return vm_fold(t[src.at]);
	return src.at < wl ? wt[src.at] : 0; // (always inside: the edits of a side without conflicts lie in the window, in order)
}
__global__ __launch_bounds__(Q_TPB) void k_vh_replay(VhCells C, VhReplay Y, VhWindows W)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	for (uint32_t c = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); c < C.n; c += waves) {
		const uint32_t x0 = C.x0[c], x1 = C.x0[c + 1], w = C.window[c];
		const uint32_t xb = first_of_kind(Y, x0, x1, 4u);
		const uint32_t a1 = first_of_kind(Y, x0, xb, KIND_UNSPELLED), a2 = first_of_kind(Y, a1, xb, KIND_EDIT);
		const uint32_t b1 = first_of_kind(Y, xb, x1, 4u | KIND_UNSPELLED), b2 = first_of_kind(Y, b1, x1, 4u | KIND_EDIT);
		VhSide sa{Y.uidx[a2], Y.uidx[xb] - Y.uidx[a2], 0, 0}, sb{Y.uidx[b2], Y.uidx[x1] - Y.uidx[b2], 0, 0};
		const bool bad = W.bad[w] != 0;
		bool conflict_a = false, conflict_b = false;
		uint8_t st = vh_status(bad, xb > x0, x1 > xb, a2 > a1, b2 > b1, false, false);
		if (st == VH_COMPARE) {
			conflict_a = side_conflict(C, Y, sa.u0, sa.u0 + sa.n, lane);
			if (!conflict_a)
				conflict_b = side_conflict(C, Y, sb.u0, sb.u0 + sb.n, lane);
			st = vh_status(false, true, true, false, false, conflict_a, conflict_b);
		}
		uint64_t diff = ~0ull;
		if (st == VH_COMPARE) {
			const uint64_t blo = W.lo[w], wl = W.hi[w] - blo;
			const uint8_t *wt = Y.wtext + Y.woff[w];
			sa.base = Y.dpos[a2] + blo, sa.len = wl + (Y.dpos[xb] - Y.dpos[a2]);
			sb.base = Y.dpos[b2] + blo, sb.len = wl + (Y.dpos[x1] - Y.dpos[b2]);
			const uint64_t n = min(sa.len, sb.len);
			for (uint64_t h0 = 0; h0 < n; h0 += 64) {
				const uint64_t h = h0 + lane;
				const bool ne = h < n && side_byte(C, Y, sa, wt, wl, blo, h) != side_byte(C, Y, sb, wt, wl, blo, h);
				const unsigned long long m = __ballot(ne);
				if (m) {
					diff = h0 + (uint64_t)(__ffsll((long long)m) - 1);
					break;
				}
			}
			if (diff == ~0ull && sa.len != sb.len)
				diff = n;
			st = vh_compared(diff == ~0ull, sa.n, sb.n);
		}
		if (lane == 0) {
			C.status[c] = st, C.edits_a[c] = sa.n, C.edits_b[c] = sb.n;
			C.len_a[c] = sa.len, C.len_b[c] = sb.len, C.first_diff[c] = diff;
			atomicAdd(Y.sample_status + (size_t)C.sample[c] * POVU_HIP_H_N_STATUS + st, 1ull);
		}
	}
}

struct HapOwner {
	povu_hip_vcf_hap view{}; // first member: the owner is recovered from it in povu_hip_vcf_hap_free
	PinnedVec<uint8_t> block; // every array of the view that came from the device, in one page-locked block (HostSpans)
	std::vector<uint32_t> col_a, col_b;
};
} // namespace

static povu_hip_vcf_hap *vcf_haplotypes(povu_hip_ctx *ctx, const povu_hip_vcf_doc *da, const povu_hip_vcf_doc *db, const char *const *path_name,
					uint32_t n_paths, const povu_hip_vcf_hap_opts *opts, CallTimer &timer)
{
	const bool force = opts && (opts->flags & POVU_HIP_V_FORCE_TIER2), reference = path_name != nullptr;
	const uint32_t max_reach = opts ? opts->max_reach : POVU_HIP_H_MAX_REACH_DEFAULT;
	const char *who = "the haplotype comparison needs ";
	if (ctx && da && db && max_reach > POVU_HIP_H_MAX_REACH_MOST) // (null arguments are the builder's to refuse, first)
		throw HipError("max_reach " + std::to_string(max_reach) + ": more than " + std::to_string(POVU_HIP_H_MAX_REACH_MOST) + " is refused");
	PairWant want{};
	want.t_rec = want.t_al = want.t_col = want.t_ph = want.colmap = true;
	PairUpload U = pair_build(ctx, da, db, who, want, POS_LIMIT);
	if (reference) {
		if (!ctx->g.block || !ctx->paths_valid || ctx->paths_gen != ctx->g.gen)
			throw HipError("reference mode needs the paths of the graph now uploaded (povu_hip_paths_upload after povu_hip_graph_upload)");
		if (!ctx->seq_valid || ctx->seq_gen != ctx->g.gen)
			throw HipError("reference mode needs the sequences of the graph now uploaded (povu_hip_segments_upload after povu_hip_graph_upload)");
		if (n_paths != ctx->n_paths)
			throw HipError(std::to_string(n_paths) + " path names for " + std::to_string(ctx->n_paths) + " resident paths");
		for (uint32_t k = 0; k < n_paths; k++)
			if (!path_name[k])
				throw HipError("null path name");
	}
	const uint32_t nRa = U.nRa, nR = U.nR, nAl = U.nAl, nT = U.nT, nI = U.nI, nIa = U.nIa, nC = U.nC, n_chroms = U.n_chroms, hbits = hash_bits_hook();
	const uint32_t n_cols_a = U.n_cols_a, n_cols = U.n_cols, max_phase = U.max_phase;
	auto o = std::make_unique<HapOwner>();

	HIP_CHECK(hipSetDevice(ctx->device));
	ctx->wait_tail();
	hipStream_t s = U.s = ctx->stream;
	// ---- the reference: the paths the CHROMs name, one after another (a "reference index" over them, as the calls build it)
	std::vector<uint32_t> h_chrom_ref((size_t)n_chroms + 1, NO_QUERY), h_ref_path;
	std::vector<uint64_t> h_ref_base(1, 0);
	if (reference) {
		std::unordered_map<std::string, uint32_t> path_of; // (of several paths of one name the first counts)
		for (uint32_t k = 0; k < n_paths; k++)
			path_of.emplace(path_name[k], k);
		std::vector<uint64_t> path_off((size_t)n_paths + 1);
		HIP_CHECK(copy_async(path_off.data(), ctx->path_off, ((size_t)n_paths + 1) * 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		for (uint32_t c = 0; c < n_chroms; c++) {
			const auto at = path_of.find(U.chrom_name[c]);
			if (at == path_of.end())
				continue;
			h_chrom_ref[c] = (uint32_t)h_ref_path.size();
			h_ref_path.push_back(at->second);
			h_ref_base.push_back(h_ref_base.back() + path_off[at->second + 1] - path_off[at->second]);
		}
	}
	const uint32_t nRef = (uint32_t)h_ref_path.size();
	const uint64_t NRs = h_ref_base.back();

	// ---- the layout of the workspace (vc_ws): what is uploaded and worked on, and the results whose sizes are known now
	const size_t r1 = (size_t)nR + 1, i1 = (size_t)nI + 1, t1 = (size_t)nT + 1, big = std::max({r1, i1, t1}) + 1;
	uint32_t *aoff, *ioff, *chrom, *t_rec, *t_al, *t_col, *t_ph, *colmap, *chrom_ref, *ref_path, *it_rec, *it_k, *suffix, *prefix, *left, *right, *t_len, *rq,
		*rlen, *t2, *firstf, *gidx, *gid, *place, *rec_window, *headf, *widx, *w_chrom, *w_na, *w_nb, *w_off, *tk_win, *tk_smp, *tk_item, *cidx, *uidx, *c_x0,
		*u_item, *words;
	uint64_t *toff, *pos, *ref_base, *ref_len, *roff, *s64, *bs, *be, *t_at, *rhash, *sp_lo, *sp_hi, *wlen, *woff, *dpos, *u_key;
	unsigned long long *w_lo, *w_hi, *cnt, *splits;
	uint8_t *placed, *state, *keep, *w_bad, *tk_sk;
	char *text;
	GroupWs gw;
	gw.tmp_bytes = prim_tmp_bytes(big + 1, true) + 256;
	const size_t s64_words = scan_exclusive_u64_tmp(std::max<size_t>({(size_t)NRs + 1, r1, t1}));
	timer.start(s);
	carve(ctx->vc_ws, [&](Spans &take) {
		take(r1, aoff, ioff, chrom, rec_window, headf, widx, w_chrom, w_na, w_nb, w_off);
		take(r1, pos, sp_lo, sp_hi, wlen, woff);
		take(r1, w_lo, w_hi);
		take(r1, placed, w_bad);
		take((size_t)nAl + 1, toff);
		take(U.n_text + 1, text);
		take(t1, t_rec, t_al, t_col, t_ph, tk_win, tk_smp, tk_item, cidx, uidx, c_x0, u_item);
		take(t1, dpos, u_key);
		take(t1, tk_sk);
		take((size_t)n_cols + 1, colmap);
		take((size_t)n_chroms + 1, chrom_ref);
		take((size_t)nRef + 1, ref_path);
		take((size_t)nRef + 1, ref_base);
		take((size_t)NRs + 1, ref_len, roff);
		take(s64_words, s64);
		take(i1, it_rec, it_k, suffix, prefix, left, right, t_len, rq, rlen, t2, firstf, gid, place, gw.head, gw.rep, gw.blist);
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
	U.up(t_rec, U.t_rec), U.up(t_al, U.t_al), U.up(t_col, U.t_col), U.up(t_ph, U.t_ph), U.up(colmap, U.colmap);
	U.up(chrom_ref, h_chrom_ref), U.up(ref_path, h_ref_path), U.up(ref_base, h_ref_base);
	HIP_CHECK(hipMemsetAsync(words, 0, 32, s));
	HIP_CHECK(hipMemsetAsync(cnt, 0, CN_WORDS * 8, s));
	HIP_CHECK(hipMemsetAsync(rec_window, 0xFF, r1 * 4, s));
	HIP_CHECK(hipMemsetAsync(left, 0, i1 * 4, s));
	HIP_CHECK(hipMemsetAsync(right, 0, i1 * 4, s));

	// ---- the reference's base offsets; placement
	const PathsView P = paths_view(ctx);
	const RefView R{NRs, nRef, nullptr, ref_path, ref_base, roff};
	const VhRef F{reference ? 1u : 0u, chrom_ref, R, P};
	if (reference) {
		HIP_CHECK(hipMemsetAsync(ref_len + NRs, 0, 8, s));
		if (NRs)
			launch_ref_len(R, P, ref_len, s);
		scan_exclusive_u64(ref_len, roff, NRs + 1, s64, s);
	}
	const PairView A{nR, nRa, nI, nIa, aoff, ioff, toff, text, pos, chrom, it_rec, it_k};
	const EditPolicy E{{state, keep, bs, be, t_at, t_len, suffix, prefix, rq, rlen, rhash, ((uint64_t)hash_mask_hi(hbits) << 32) | hash_mask_lo(hbits), n_chroms, placed}};
	const VhWindows W{w_chrom, w_na, w_nb, w_off, w_lo, w_hi, w_bad};
	uint64_t h_cnt[CN_WORDS] = {0};
	uint32_t n_t2 = 0, nG = 0, nW = 0, nV = 0, nCells = 0;
	uint64_t n_splits = 0, total_text = 0;
	if (nR)
		KLAUNCH(k_vh_place, dim3(std::min(stride_blocks(nR), COUNT_BLOCKS)), dim3(Q_TPB), 0, s, A, F, placed, sp_lo, sp_hi, cnt);
	// ---- items, edits, reaches, groups, the items' order
	if (nI) {
		n_t2 = launch_tiers(A, E, force, t2, words + 1, s);
		if (reference)
			KLAUNCH(k_vh_reach, dim3(wave_blocks(nI)), dim3(Q_TPB), 0, s, A, E.O, F, max_reach, left, right, reinterpret_cast<unsigned long long *>(sp_lo),
				reinterpret_cast<unsigned long long *>(sp_hi), cnt);
		// (T has at most `longest` bytes, a CHROM id is at most n_chroms: an item's without an edit)
		const uint32_t *sp = group_exact(nI, rq, rlen, rhash, hbits, bits_for(U.longest), bits_for(n_chroms), SameEdit{text, state, bs, be, t_at, t_len}, gw,
						 words + 2, splits, &n_splits, s);
		number_groups(nI, sp, gw.rep, firstf, gidx, keep, gw.tmp, gw.tmp_bytes, s);
		nG = read_back(gidx + nI, s); // (waits for the stream: n_splits has arrived)
		KLAUNCH(k_eg_group_of, dim3(stride_blocks(nI)), dim3(Q_TPB), 0, s, nI, sp, gw.rep, gidx, keep, gid);
		launch_iota(nI, gw.pa, s);
		LsdSort sort{gw.pa, gw.pb, gw.key, gw.kout, nI, gw.tmp, gw.tmp_bytes, s};
		auto key = [&](int which, const uint32_t *cur, uint32_t *k) {
			KLAUNCH(k_vh_item_key, dim3(stride_blocks(nI)), dim3(Q_TPB), 0, s, nI, which, nG, cur, gid, bs, be, k);
		};
		sort.pass(0, bits_for(nG), key);
		sort.pass(1, 32, key); // (s and e are below 2^42: a POS below 2^40 and a text below 2^32)
		sort.pass(2, 10, key);
		sort.pass(3, 32, key);
		sort.pass(4, 10, key);
		KLAUNCH(k_vh_inverse, dim3(stride_blocks(nI)), dim3(Q_TPB), 0, s, nI, sort.cur, place);
	}
	// ---- windows
	uint32_t nP = 0;
	if (nR) {
		HIP_CHECK(copy_async(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		nP = (uint32_t)(h_cnt[CN_PLACED_A] + h_cnt[CN_PLACED_B]);
	}
	const uint32_t *span_order = nullptr;
	if (nP) {
		launch_iota(nR, gw.pa, s);
		LsdSort sort{gw.pa, gw.pb, gw.key, gw.kout, nR, gw.tmp, gw.tmp_bytes, s};
		auto key = [&](int which, const uint32_t *cur, uint32_t *k) {
			KLAUNCH(k_vh_span_key, dim3(stride_blocks(nR)), dim3(Q_TPB), 0, s, nR, which, n_chroms, cur, placed, chrom, sp_lo, k);
		};
		sort.pass(0, 32, key);
		sort.pass(1, 10, key);
		sort.pass(2, bits_for(n_chroms), key);
		span_order = sort.cur;
		KLAUNCH(k_vh_span_reach, dim3(stride_blocks(nP)), dim3(Q_TPB), 0, s, nP, span_order, chrom, sp_lo, sp_hi, gw.mark);
		scan_exclusive_max_u32(gw.mark, gw.hmax, nP, gw.tmp, gw.tmp_bytes, s);
		KLAUNCH(k_vh_heads, dim3(stride_blocks((size_t)nP + 1)), dim3(Q_TPB), 0, s, nP, gw.hmax, headf);
		scan_exclusive_u32(headf, widx, (size_t)nP + 1, gw.tmp, gw.tmp_bytes, s);
		nW = read_back(widx + nP, s);
		HIP_CHECK(hipMemsetAsync(w_hi, 0, r1 * 8, s));
		HIP_CHECK(hipMemsetAsync(w_na, 0, r1 * 4, s));
		HIP_CHECK(hipMemsetAsync(w_nb, 0, r1 * 4, s));
		HIP_CHECK(hipMemsetAsync(w_off, 0xFF, r1 * 4, s));
		HIP_CHECK(hipMemsetAsync(w_bad, 0, r1, s));
		KLAUNCH(k_vh_windows, dim3(stride_blocks(nP)), dim3(Q_TPB), 0, s, nP, nRa, span_order, widx, headf, chrom, sp_lo, sp_hi, rec_window, W);
		KLAUNCH(k_vh_window_len, dim3(stride_blocks((size_t)nW + 1)), dim3(Q_TPB), 0, s, nW, W, wlen);
		scan_exclusive_u64(wlen, woff, (size_t)nW + 1, s64, s);
		total_text = read_back(woff + nW, s);
		refuse_2_32(total_text + 64, who, "window-text bytes");
	}
	// ---- the tasks that take part, counted: they bound the cells and the distinct edits
	const VhTasks K0{nT, 0, t_rec, t_al, t_col, t_ph, tk_win, tk_smp, tk_item, tk_sk};
	if (nT && nW && nC) {
		KLAUNCH(k_vh_tasks, dim3(std::min(stride_blocks(nT), COUNT_BLOCKS)), dim3(Q_TPB), 0, s, A, K0, nW, n_cols_a, colmap, placed, rec_window, state, cnt);
		nV = (uint32_t)read_back(cnt + CN_TASKS, s);
	}
	// ---- the second arena (vc_hit): the windows' text and the results per cell and per sample
	uint8_t *wtext, *c_status;
	uint32_t *c_window, *c_sample, *c_phase, *c_ea, *c_eb;
	unsigned long long *c_la, *c_lb, *c_fd, *s_status;
	const size_t v1 = (size_t)nV + 1, n_ss = (size_t)nC * POVU_HIP_H_N_STATUS + 1;
	carve(ctx->vc_hit, [&](Spans &take) {
		take(total_text + 8, wtext);
		take(v1, c_window, c_sample, c_phase, c_ea, c_eb);
		take(v1, c_la, c_lb, c_fd);
		take(v1, c_status);
		take(n_ss, s_status);
	});
	HIP_CHECK(hipMemsetAsync(s_status, 0, n_ss * 8, s));
	// ---- the windows' text and verdicts
	if (nW) {
		if (reference) {
			KLAUNCH(k_vh_fill_ref, dim3(stride_blocks(total_text)), dim3(Q_TPB), 0, s, total_text, nW, woff, W, F, wtext);
		} else {
			HIP_CHECK(hipMemsetAsync(wtext, 0, total_text + 8, s));
			KLAUNCH(k_vh_fill_rec, dim3(wave_blocks(nR)), dim3(Q_TPB), 0, s, A, placed, rec_window, woff, W, reinterpret_cast<uint32_t *>(wtext));
		}
		KLAUNCH(k_vh_verify, dim3(wave_blocks(nR)), dim3(Q_TPB), 0, s, A, placed, rec_window, woff, W, wtext);
		KLAUNCH(k_vh_count_bad, dim3(std::min(stride_blocks(nW), COUNT_BLOCKS)), dim3(Q_TPB), 0, s, nW, w_bad, cnt);
	}
	// ---- cells
	if (nV) {
		VhTasks K = K0;
		K.nV = nV;
		launch_iota(nT, gw.pa, s);
		LsdSort sort{gw.pa, gw.pb, gw.key, gw.kout, nT, gw.tmp, gw.tmp_bytes, s};
		auto key = [&](int which, const uint32_t *cur, uint32_t *k) {
			KLAUNCH(k_vh_task_key, dim3(stride_blocks(nT)), dim3(Q_TPB), 0, s, K, which, cur, place, k);
		};
		sort.pass(0, bits_for(nI), key);
		sort.pass(1, 3, key);
		sort.pass(2, bits_for(max_phase), key);
		sort.pass(3, bits_for(nC), key);
		sort.pass(4, bits_for(nW), key);
		const uint32_t *sorted = sort.cur;
		uint32_t *chead = gw.key, *uniq = gw.kout; // (the sort's key buffers are free again)
		KLAUNCH(k_vh_task_heads, dim3(stride_blocks(v1)), dim3(Q_TPB), 0, s, K, sorted, gid, bs, be, t_len, chead, uniq, dpos);
		scan_exclusive_u32_pair(chead, cidx, v1, uniq, uidx, v1, gw.tmp, gw.tmp_bytes, s);
		scan_exclusive_u64(dpos, dpos, v1, s64, s);
		nCells = read_back(cidx + nV, s);
		const VhCells C{nCells, nV, c_x0, c_window, c_sample, c_phase, c_ea, c_eb, c_status, c_la, c_lb, c_fd, u_item, u_key};
		KLAUNCH(k_vh_cells, dim3(stride_blocks(v1)), dim3(Q_TPB), 0, s, K, C, sorted, chead, cidx, uniq, uidx, dpos, bs);
		const VhReplay Y{sorted, tk_sk, uidx, dpos, bs, be, t_at, t_len, text, woff, wtext, s_status};
		KLAUNCH(k_vh_replay, dim3(wave_blocks(nCells)), dim3(Q_TPB), 0, s, C, Y, W);
	}

	// ---- to the host
	const size_t w1 = (size_t)nW + 1, c1 = (size_t)nCells + 1;
	povu_hip_vcf_hap &v = o->view;
	uint64_t *h_bs = nullptr, *h_be = nullptr, *h_lo = nullptr, *h_hi = nullptr;
	const uint8_t *h_state = nullptr;
	const unsigned long long *h_ss = nullptr;
	static_assert(sizeof(unsigned long long) == sizeof(uint64_t) && sizeof(int64_t) == sizeof(uint64_t), "the arrays are read as (u)int64_t");
	auto results = [&](HostSpans &take) {
		const uint8_t *h_placed = take(placed, nR, r1);
		const uint32_t *h_window = take(rec_window, nR, r1), *h_rec = take(it_rec, nI, i1), *h_k = take(it_k, nI, i1);
		h_state = take(state, nI, i1);
		h_bs = take(bs, nI, i1), h_be = take(be, nI, i1);
		const uint32_t *h_suffix = take(suffix, nI, i1), *h_prefix = take(prefix, nI, i1), *h_left = take(left, nI, i1), *h_right = take(right, nI, i1),
			       *h_gid = take(gid, nI, i1);
		v.win_chrom = take(w_chrom, nW, w1);
		h_lo = take(reinterpret_cast<uint64_t *>(w_lo), nW, w1), h_hi = take(reinterpret_cast<uint64_t *>(w_hi), nW, w1);
		v.win_n_a = take(w_na, nW, w1), v.win_n_b = take(w_nb, nW, w1), v.win_inconsistent = take(w_bad, nW, w1), v.win_offender = take(w_off, nW, w1);
		v.cell_window = take(c_window, nCells, c1), v.cell_sample = take(c_sample, nCells, c1), v.cell_phase = take(c_phase, nCells, c1);
		v.cell_status = take(c_status, nCells, c1), v.cell_edits_a = take(c_ea, nCells, c1), v.cell_edits_b = take(c_eb, nCells, c1);
		v.cell_len_a = reinterpret_cast<const uint64_t *>(take(c_la, nCells, c1)), v.cell_len_b = reinterpret_cast<const uint64_t *>(take(c_lb, nCells, c1));
		v.cell_first_diff = reinterpret_cast<const uint64_t *>(take(c_fd, nCells, c1));
		h_ss = take(s_status, n_ss - 1, n_ss);
		v.rec_placed_a = h_placed, v.rec_placed_b = h_placed + nRa, v.rec_window_a = h_window, v.rec_window_b = h_window + nRa;
		v.item_record_a = h_rec, v.item_record_b = h_rec + nIa, v.item_alt_a = h_k, v.item_alt_b = h_k + nIa;
		v.item_state_a = h_state, v.item_state_b = h_state + nIa;
		v.item_s_a = reinterpret_cast<const int64_t *>(h_bs), v.item_s_b = v.item_s_a + nIa;
		v.item_e_a = reinterpret_cast<const int64_t *>(h_be), v.item_e_b = v.item_e_a + nIa;
		v.item_suffix_a = h_suffix, v.item_suffix_b = h_suffix + nIa, v.item_prefix_a = h_prefix, v.item_prefix_b = h_prefix + nIa;
		v.item_left_a = h_left, v.item_left_b = h_left + nIa, v.item_right_a = h_right, v.item_right_b = h_right + nIa;
		v.item_group_a = h_gid, v.item_group_b = h_gid + nIa;
		v.win_lo = reinterpret_cast<const int64_t *>(h_lo), v.win_hi = reinterpret_cast<const int64_t *>(h_hi);
		v.sample_status = reinterpret_cast<const uint64_t *>(h_ss);
	};
	hand_off_block(o->block, ctx, results);
	HIP_CHECK(copy_async(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, s));
	v.device_ms = timer.stop(s);
	// (the coordinates carried one more than their 0-based value; an item without an edit has 0 in both)
	for (uint32_t i = 0; i < nI; i++)
		if (h_state[i] == POVU_HIP_H_EDIT)
			h_bs[i] -= 1, h_be[i] -= 1;
	for (uint32_t w = 0; w < nW; w++)
		h_lo[w] -= 1, h_hi[w] -= 1;
	v.n_records_a = nRa, v.n_records_b = nR - nRa, v.n_items_a = nIa, v.n_items_b = nI - nIa, v.n_groups = nG, v.n_windows = nW, v.n_cells = nCells;
	v.n_common_samples = nC;
	o->col_a = std::move(U.col_a), o->col_b = std::move(U.col_b);
	v.sample_col_a = o->col_a.data(), v.sample_col_b = o->col_b.data();
	for (uint32_t x = 0; x < nC; x++)
		for (uint32_t k = 0; k < POVU_HIP_H_N_STATUS; k++)
			v.n_status[k] += h_ss[(size_t)x * POVU_HIP_H_N_STATUS + k];
	v.n_inconsistent = h_cnt[CN_BAD_WINDOWS];
	v.n_unplaced_a = nRa - h_cnt[CN_PLACED_A], v.n_unplaced_b = (nR - nRa) - h_cnt[CN_PLACED_B];
	v.n_reach_capped = h_cnt[CN_CAPPED], v.n_tier2 = n_t2, v.n_splits = n_splits, v.reference = reference;
	return &o.release()->view;
}

} // namespace povu_hip

// ---- C ABI

extern "C" povu_hip_vcf_hap *povu_hip_vcf_haplotypes(povu_hip_ctx *ctx, const povu_hip_vcf_doc *doc_a, const povu_hip_vcf_doc *doc_b,
						     const char *const *path_name, uint32_t n_paths, const povu_hip_vcf_hap_opts *opts, char *err,
						     size_t errlen)
{
	CallTimer timer;
	return guarded_call(ctx, err, errlen, (povu_hip_vcf_hap *)nullptr, [&] { return vcf_haplotypes(ctx, doc_a, doc_b, path_name, n_paths, opts, timer); });
}
extern "C" void povu_hip_vcf_hap_free(povu_hip_vcf_hap *h)
{
	delete reinterpret_cast<HapOwner *>(h);
}
