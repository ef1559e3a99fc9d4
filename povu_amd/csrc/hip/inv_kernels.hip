// inv_kernels.hip -- the inversion (SUBR) records of povu_hip_call with POVU_HIP_T_INVERSIONS (include/povu_hip.h).
//
// The definition is this project's own ("Inversion calls"; restated in tests/inversions_ref.py): step j of
// another path matches step i of a reference path when it is the same segment the other way round (path words differ in
// bit 0 only), a run is a maximal anti-diagonal of matches, a run of 2 .. max_steps steps that spells a base supports the
// record (reference, first step, steps).  All of it runs on the paths resident in the context:
//   step index   the global positions of the path steps, stable-sorted by step value, and a CSR over the 2 V values
//                (build_step_index, which the VCF checks of vcfcheck_kernels.hip call too);
//   run heads    per reference step the entries of the opposite value's list on another path whose predecessor
//                (i - 1, j + 1) is no match: a lane per reference step for lists below 64 entries, a wave per step (lanes
//                across the list, a ballot per 64) for the others; count, u64 scan, 2^32 check, emit;
//   extension    a lane per head up to 64 steps, the runs that go on to a wave each (64 comparisons a ballot);
//   records      the reported runs stable-sorted by (reference index, steps, slot): the first run of every (index, steps)
//                group is a record;
//   rows         the records' rows in one list with the flubble records (two binary searches), their fields, GT rows,
//                AC / AN / NS, and their two spelled alleles (call_common.hpp's emit_steps).
#include "call_common.hpp"

namespace povu_hip
{

static constexpr uint32_t TIER1_STEPS = 64, LONG_LIST = 64;

// what the kernels read of the references and the resident paths
struct InvView {
	RefView ref;
	PathsView paths;
	const uint32_t *ioff, *occ; // the step index: positions occ[ioff[x] .. ioff[x + 1]) hold step value x, ascending
};
// reference step i: its path, its global position, its path's end
struct RefStep {
	uint32_t r, path;
	uint64_t g, begin, end;
};
__device__ __forceinline__ RefStep ref_step(const InvView &A, uint64_t i)
{
	RefStep x;
	x.r = span_of(A.ref.ref_base, A.ref.nR, i);
	x.path = A.ref.ref_path[x.r];
	x.begin = A.paths.path_off[x.path];
	x.end = A.paths.path_off[x.path + 1];
	x.g = x.begin + (i - A.ref.ref_base[x.r]);
	return x;
}
// is (x, y) the head of a run: y on another path, and (x - 1, y + 1) no match
__device__ __forceinline__ bool is_head(const InvView &A, const RefStep &x, uint32_t y)
{
	const uint32_t pa = span_of(A.paths.path_off, A.paths.n_paths, y);
	if (pa == x.path)
		return false;
	if (x.g == x.begin || (uint64_t)y + 1 >= A.paths.path_off[pa + 1])
		return true;
	return A.paths.steps[y + 1] != (A.paths.steps[x.g - 1] ^ 1u);
}

__global__ void k_inv_hist(uint32_t N, const uint32_t *__restrict__ steps, uint32_t *__restrict__ cnt)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < N; i += gridDim.x * Q_TPB)
		atomicAdd(cnt + steps[i], 1u);
}

// ---- run heads.  EMIT false: cnt[i] = heads of reference step i, the steps with a list of long_min entries or more appended
// to `longs` instead; EMIT true: the heads of step i written from hoff[i] on
template <bool EMIT>
__global__ void k_inv_heads(InvView A, uint32_t long_min, uint64_t *__restrict__ cnt, const uint64_t *__restrict__ hoff,
			    uint32_t *__restrict__ hx, uint32_t *__restrict__ hy, uint32_t *__restrict__ longs, uint32_t *__restrict__ n_longs)
{
	for (uint64_t i = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; i < A.ref.NR; i += (uint64_t)gridDim.x * Q_TPB) {
		const RefStep x = ref_step(A, i);
		const uint32_t v = A.paths.steps[x.g] ^ 1u, e0 = A.ioff[v], e1 = A.ioff[v + 1];
		if (e1 - e0 >= long_min) {
			if (!EMIT)
				longs[atomicAdd(n_longs, 1u)] = (uint32_t)i;
			continue;
		}
		uint64_t c = 0;
		for (uint32_t e = e0; e < e1; e++) {
			const uint32_t y = A.occ[e];
			if (!is_head(A, x, y))
				continue;
			if (EMIT) {
				hx[hoff[i] + c] = (uint32_t)i;
				hy[hoff[i] + c] = y;
			}
			c++;
		}
		if (!EMIT)
			cnt[i] = c;
	}
}
// ... of the reference steps in `longs`, a wave each, lanes across the list
template <bool EMIT>
__global__ __launch_bounds__(Q_TPB) void k_inv_heads_wave(InvView A, const uint32_t *__restrict__ longs, uint32_t n_longs,
							  uint64_t *__restrict__ cnt, const uint64_t *__restrict__ hoff,
							  uint32_t *__restrict__ hx, uint32_t *__restrict__ hy)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	for (uint32_t w = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); w < n_longs; w += waves) {
		const uint64_t i = longs[w];
		const RefStep x = ref_step(A, i);
		const uint32_t v = A.paths.steps[x.g] ^ 1u, e0 = A.ioff[v], e1 = A.ioff[v + 1];
		uint64_t c = 0;
		for (uint32_t b = e0; b < e1; b += 64) { // (e1 + 64 < 2^32: inv_find refuses more steps)
			const uint32_t e = b + lane;
			const uint32_t y = e < e1 ? A.occ[e] : 0;
			const bool head = e < e1 && is_head(A, x, y);
			const unsigned long long m = __ballot(head);
			if (EMIT && head) {
				const uint64_t at = hoff[i] + c + __popcll(m & ((1ull << lane) - 1));
				hx[at] = (uint32_t)i;
				hy[at] = y;
			}
			c += __popcll(m);
		}
		if (!EMIT && lane == 0)
			cnt[i] = c;
	}
}

// ---- extension.  The run of head h goes on while both paths do, the steps match and it has fewer than max_steps + 1 steps
struct RunView {
	uint64_t gx, y, lim; // lim: the steps the run can have at most
	uint32_t pa;
};
__device__ __forceinline__ RunView run_view(const InvView &A, uint32_t i, uint32_t y, uint32_t max_steps)
{
	const RefStep x = ref_step(A, i);
	RunView r;
	r.gx = x.g;
	r.y = y;
	r.pa = span_of(A.paths.path_off, A.paths.n_paths, y);
	const uint64_t lx = x.end - x.g, ly = (uint64_t)y - A.paths.path_off[r.pa] + 1;
	r.lim = min(min(lx, ly), (uint64_t)max_steps + 1);
	return r;
}
// tier 1: a lane per head, up to TIER1_STEPS steps; a run that has more (or every run, with force) goes to `t2`
__global__ void k_inv_extend(uint32_t H, InvView A, uint32_t max_steps, uint32_t force, const uint32_t *__restrict__ hx,
			     const uint32_t *__restrict__ hy, uint32_t *__restrict__ hL, uint32_t *__restrict__ hslot,
			     const uint32_t *__restrict__ slot_of_path, uint32_t *__restrict__ t2, uint32_t *__restrict__ n_t2)
{
	for (uint32_t h = blockIdx.x * Q_TPB + threadIdx.x; h < H; h += gridDim.x * Q_TPB) {
		const RunView r = run_view(A, hx[h], hy[h], max_steps);
		hslot[h] = slot_of_path[r.pa];
		const uint64_t cap = min(r.lim, (uint64_t)TIER1_STEPS + 1);
		uint64_t n = 1;
		if (!force)
			while (n < cap && A.paths.steps[r.gx + n] == (A.paths.steps[r.y - n] ^ 1u))
				n++;
		if (force || n > TIER1_STEPS)
			t2[atomicAdd(n_t2, 1u)] = h;
		else
			hL[h] = (uint32_t)n;
	}
}
// tier 2: a wave per run of `t2`, taken from *next (zeroed before the launch); 64 comparisons a ballot
__global__ __launch_bounds__(Q_TPB) void k_inv_extend_wave(const uint32_t *__restrict__ t2, uint32_t n2, uint32_t *__restrict__ next, InvView A,
							   uint32_t max_steps, const uint32_t *__restrict__ hx, const uint32_t *__restrict__ hy,
							   uint32_t *__restrict__ hL)
{
	const uint32_t lane = threadIdx.x & 63u;
	for (uint32_t it = 0; it < n2; it++) { // (a wave takes at most all n2 runs: the loop is bounded whatever the counter says)
		uint32_t w = 0;
		if (lane == 0)
			w = atomicAdd(next, 1u);
		w = __shfl(w, 0);
		if (w >= n2)
			break;
		const uint32_t h = t2[w];
		const RunView r = run_view(A, hx[h], hy[h], max_steps);
		uint64_t n = r.lim;
		for (uint64_t base = 1; base < r.lim; base += 64) {
			const uint64_t k = base + lane;
			const bool stop = k < r.lim && A.paths.steps[r.gx + k] != (A.paths.steps[r.y - k] ^ 1u);
			const unsigned long long m = __ballot(stop);
			if (m) {
				n = base + (uint64_t)(__ffsll((long long)m) - 1);
				break;
			}
		}
		if (lane == 0)
			hL[h] = (uint32_t)n;
	}
}

// ---- reported runs: 2 .. max_steps steps and a base; the longer ones are counted
// With `marked` (region calls) a run whose first and last step both lie on unmarked segments is left out: every run of a
// (reference index, steps) group shares them, so whole groups go, before the records are numbered
__global__ void k_inv_report(uint32_t H, uint32_t max_steps, InvView A, const uint32_t *__restrict__ marked, const uint32_t *__restrict__ hx,
			     const uint32_t *__restrict__ hL, const uint64_t *__restrict__ roff, uint8_t *__restrict__ flag,
			     unsigned long long *__restrict__ n_long)
{
	for (uint32_t h = blockIdx.x * Q_TPB + threadIdx.x; h < H; h += gridDim.x * Q_TPB) {
		const uint32_t L = hL[h];
		bool keep = false;
		if (L > max_steps)
			atomicAdd(n_long, 1ull);
		else if (L >= 2)
			keep = roff[(uint64_t)hx[h] + L] > roff[hx[h]];
		if (keep && marked) {
			const uint64_t g = ref_step(A, hx[h]).g;
			const uint32_t a = A.paths.steps[g] >> 1, z = A.paths.steps[g + L - 1] >> 1;
			keep = ((marked[a >> 5] >> (a & 31)) | (marked[z >> 5] >> (z & 31))) & 1u;
		}
		flag[h] = keep;
	}
}
// sort key of run perm[t]: 0 = slot, 1 = steps, 2 = reference index
__global__ void k_inv_key(uint32_t n, int which, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ hx,
			  const uint32_t *__restrict__ hL, const uint32_t *__restrict__ hslot, uint32_t *__restrict__ key)
{
	for (uint32_t t = blockIdx.x * Q_TPB + threadIdx.x; t < n; t += gridDim.x * Q_TPB) {
		const uint32_t h = perm[t];
		key[t] = which == 0 ? hslot[h] : which == 1 ? hL[h] : hx[h];
	}
}
__global__ void k_inv_group(uint32_t n, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ hx, const uint32_t *__restrict__ hL,
			    uint32_t *__restrict__ first)
{
	for (uint32_t t = blockIdx.x * Q_TPB + threadIdx.x; t <= n; t += gridDim.x * Q_TPB)
		first[t] = t < n && (t == 0 || hx[perm[t]] != hx[perm[t - 1]] || hL[perm[t]] != hL[perm[t - 1]]);
}
__global__ void k_inv_records(uint32_t n, InvView A, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ hx,
			      const uint32_t *__restrict__ hL, const uint32_t *__restrict__ hslot, const uint32_t *__restrict__ first,
			      const uint32_t *__restrict__ rank, const uint64_t *__restrict__ roff, uint32_t *__restrict__ run_rec,
			      uint32_t *__restrict__ run_slot, uint32_t *__restrict__ v_ref, uint32_t *__restrict__ v_at,
			      uint32_t *__restrict__ v_steps, uint64_t *__restrict__ v_pos)
{
	for (uint32_t t = blockIdx.x * Q_TPB + threadIdx.x; t < n; t += gridDim.x * Q_TPB) {
		const uint32_t h = perm[t], b = rank[t] + first[t] - 1;
		run_rec[t] = b;
		run_slot[t] = hslot[h];
		if (first[t]) {
			const uint32_t i = hx[h], r = span_of(A.ref.ref_base, A.ref.nR, i);
			v_ref[b] = r;
			v_at[b] = i;
			v_steps[b] = hL[h];
			v_pos[b] = roff[(uint64_t)i + 1] - roff[A.ref.ref_base[r]] + 1; // the locus of the run's second step
		}
	}
}

// ---- rows of the merged list.  Both lists ascend by (reference, POS); at one POS the flubble records come first
__device__ __forceinline__ bool key_less(uint32_t r0, uint64_t p0, uint32_t r1, uint64_t p1) { return r0 < r1 || (r0 == r1 && p0 < p1); }
__global__ void k_inv_rows_flubble(uint32_t nrec, const uint32_t *__restrict__ f_ref, const uint64_t *__restrict__ f_pos, uint32_t ninv,
				   const uint32_t *__restrict__ v_ref, const uint64_t *__restrict__ v_pos, uint32_t *__restrict__ f_dst)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < nrec; i += gridDim.x * Q_TPB) {
		// the inversion records in front: those with a smaller key
		f_dst[i] = i + first_not(0u, ninv, [=](uint32_t k) { return key_less(v_ref[k], v_pos[k], f_ref[i], f_pos[i]); });
	}
}
__global__ void k_inv_rows(uint32_t ninv, const uint32_t *__restrict__ v_ref, const uint64_t *__restrict__ v_pos, uint32_t nrec,
			   const uint32_t *__restrict__ f_ref, const uint64_t *__restrict__ f_pos, uint32_t *__restrict__ v_dst)
{
	for (uint32_t b = blockIdx.x * Q_TPB + threadIdx.x; b < ninv; b += gridDim.x * Q_TPB) {
		// the flubble records in front: those whose key is not larger
		v_dst[b] = b + first_not(0u, nrec, [=](uint32_t k) { return !key_less(v_ref[b], v_pos[b], f_ref[k], f_pos[k]); });
	}
}

__global__ void k_inv_fields(uint32_t ninv, InvView A, const uint32_t *__restrict__ v_ref, const uint32_t *__restrict__ v_at,
			     const uint32_t *__restrict__ v_steps, const uint64_t *__restrict__ v_pos, const uint32_t *__restrict__ v_dst,
			     InvRows o)
{
	for (uint32_t b = blockIdx.x * Q_TPB + threadIdx.x; b < ninv; b += gridDim.x * Q_TPB) {
		const uint32_t d = v_dst[b], r = v_ref[b];
		o.o_q[d] = NO_QUERY;
		o.o_path[d] = A.ref.ref_path[r];
		o.o_first[d] = (uint32_t)(v_at[b] - A.ref.ref_base[r]);
		o.o_ref[d] = 0;
		o.o_nal[d] = 2;
		o.o_pos[d] = v_pos[b];
		o.o_nsteps[d] = v_steps[b];
		o.nalt[d] = 1;
	}
}
__global__ void k_inv_gt_init(uint64_t n, uint32_t S, uint32_t nb, InvView A, const uint32_t *__restrict__ v_ref,
			      const uint32_t *__restrict__ v_dst, const uint32_t *__restrict__ slot_of_path, uint16_t *__restrict__ gt,
			      uint32_t *__restrict__ o_block, uint64_t *__restrict__ bcnt)
{
	for (uint64_t e = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; e < n; e += (uint64_t)gridDim.x * Q_TPB) {
		const uint32_t b = (uint32_t)(e / S), sl = (uint32_t)(e % S);
		gt[(uint64_t)v_dst[b] * S + sl] = sl == slot_of_path[A.ref.ref_path[v_ref[b]]] ? 0 : POVU_HIP_GT_MISSING;
		if (sl == 0) {
			o_block[v_dst[b]] = nb + b;
			bcnt[nb + b] = 2;
		}
	}
}
// every slot that holds a supporting path but the reference's own: allele 1 (equal values from several runs)
__global__ void k_inv_gt_mark(uint32_t n_runs, uint32_t S, InvView A, const uint32_t *__restrict__ run_rec, const uint32_t *__restrict__ run_slot,
			      const uint32_t *__restrict__ v_ref, const uint32_t *__restrict__ v_dst, const uint32_t *__restrict__ slot_of_path,
			      uint16_t *__restrict__ gt)
{
	for (uint32_t t = blockIdx.x * Q_TPB + threadIdx.x; t < n_runs; t += gridDim.x * Q_TPB) {
		const uint32_t b = run_rec[t], sl = run_slot[t];
		if (sl != slot_of_path[A.ref.ref_path[v_ref[b]]])
			gt[(uint64_t)v_dst[b] * S + sl] = 1;
	}
}
// AC, AN, NS and flags: one wave per record, a lane per sample (as k_cl_records)
__global__ __launch_bounds__(Q_TPB) void k_inv_gt_count(uint32_t ninv, uint32_t S, uint32_t n_samples, const uint32_t *__restrict__ slot_first,
							const uint32_t *__restrict__ v_dst, const uint16_t *__restrict__ gt,
							const uint64_t *__restrict__ ac_off, uint32_t *__restrict__ ac, uint32_t *__restrict__ an,
							uint32_t *__restrict__ ns, uint8_t *__restrict__ flags)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	for (uint32_t b = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); b < ninv; b += waves) {
		const uint32_t d = v_dst[b];
		uint32_t n_an = 0, n_ns = 0, n_ac = 0;
		for (uint32_t sm = lane; sm < n_samples; sm += 64) {
			bool any = false;
			for (uint32_t sl = slot_first[sm]; sl < slot_first[sm + 1]; sl++) {
				const uint32_t code = gt[(uint64_t)d * S + sl];
				if (code != POVU_HIP_GT_MISSING) {
					any = true;
					n_an++;
					n_ac += code;
				}
			}
			n_ns += any;
		}
		n_an = wave_sum(n_an);
		n_ns = wave_sum(n_ns);
		n_ac = wave_sum(n_ac);
		if (lane == 0) {
			an[d] = n_an;
			ns[d] = n_ns;
			ac[ac_off[d]] = n_ac;
			flags[d] = POVU_HIP_CALL_SUBR;
		}
	}
}

// ---- spelling: REF = the run's steps, ALT = the flipped steps backwards; a wave per record / per spelled allele
__global__ __launch_bounds__(Q_TPB) void k_inv_spell_len(uint32_t ninv, InvView A, const uint32_t *__restrict__ v_at, const uint32_t *__restrict__ v_steps,
							 const uint64_t *__restrict__ roff, const uint32_t *__restrict__ vid, uint64_t *__restrict__ slen,
							 uint64_t *__restrict__ alen)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	for (uint32_t b = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); b < ninv; b += waves) {
		const uint64_t i = v_at[b], g = ref_step(A, i).g;
		const uint32_t L = v_steps[b];
		uint32_t w = 0;
		for (uint32_t k = lane; k < L; k += 64)
			w += 1 + ndig(vid[A.paths.steps[g + k] >> 1]);
		w = wave_sum(w);
		if (lane < 2) {
			slen[2 * (uint64_t)b + lane] = roff[i + L] - roff[i];
			alen[2 * (uint64_t)b + lane] = w;
		}
	}
}
__global__ __launch_bounds__(Q_TPB) void k_inv_emit(uint64_t n, InvView A, const uint32_t *__restrict__ v_at, const uint32_t *__restrict__ v_steps,
						    const uint64_t *__restrict__ seq_off, const char *__restrict__ seq, const uint32_t *__restrict__ vid,
						    const uint64_t *__restrict__ s_off, const uint64_t *__restrict__ a_off, char *__restrict__ o_seq,
						    char *__restrict__ o_at, unsigned long long *__restrict__ bad)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t waves = (uint64_t)gridDim.x * (Q_TPB / 64);
	for (uint64_t j = (uint64_t)blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); j < n; j += waves) {
		const uint32_t b = (uint32_t)(j >> 1), L = v_steps[b];
		const bool alt = j & 1u;
		const uint64_t g = ref_step(A, v_at[b]).g;
		const uint32_t *steps = A.paths.steps;
		emit_steps(
			lane, L, [&](uint32_t k) { return alt ? steps[g + L - 1 - k] ^ 1u : steps[g + k]; }, seq_off, seq, vid, s_off[j], a_off[j],
			o_seq, o_at, bad);
	}
}

static InvView view_of(const InvIn &in, const InvDevice &v)
{
	return InvView{in.ref, in.paths, v.ioff, v.occ};
}

namespace
{
// iv_ws: the step index, the head counts and offsets of every reference step
struct InvIndex {
	uint32_t *longs, *words; // the reference steps with a long list; words: [0] their number, [1] tier-2 runs, [2] tier 2's work counter, [3] reported runs
	uint64_t *hcnt, *hoff, *s64;
	unsigned long long *n_long;
	uint32_t long_min, n_longs = 0;
};
// iv_heads: the run heads (x: reference index, y: the other path's global position), their runs
struct InvHeads {
	uint32_t H = 0;
	uint32_t *hx, *hy, *hL, *hslot, *t2, *rlist, *perm2, *key, *key2, *first, *rank;
	uint8_t *flag;
	void *tmp;
	size_t tmp_bytes;
};
} // namespace

// The step index of the resident paths, carved from `A` in front of the caller's own spans (`more`) and built on the context's
// stream: the global positions of the path steps stable-sorted by step value, and a CSR over the 2 V values
StepIndex build_step_index(povu_hip_ctx *ctx, Arena &A, const std::function<void(Spans &)> &more)
{
	hipStream_t s = ctx->stream;
	const uint64_t N = ctx->n_path_steps;
	const size_t nval = 2 * (size_t)ctx->g.V + 1;
	const size_t tmp_bytes = std::max(sort_tmp_bytes(N + 1), prim_tmp_bytes(nval + 1, false)) + 256;
	uint32_t *iota, *skey, *occ, *cnt, *ioff;
	void *tmp;
	carve(A, [&](Spans &take) {
		take(N + 1, iota, skey, occ);
		take(nval + 1, cnt, ioff);
		more(take);
		take(tmp_bytes, tmp);
	});
	HIP_CHECK(hipMemsetAsync(cnt, 0, (nval + 1) * 4, s));
	launch_iota((uint32_t)N, iota, s);
	KLAUNCH(k_inv_hist, dim3(stride_blocks(N)), dim3(Q_TPB), 0, s, (uint32_t)N, ctx->path_steps, cnt);
	scan_exclusive_u32(cnt, ioff, nval, tmp, tmp_bytes, s);
	sort_pairs_u32(ctx->path_steps, skey, iota, occ, N, bits_for(2 * (uint64_t)ctx->g.V), tmp, tmp_bytes, s);
	return StepIndex{ioff, occ};
}

static InvIndex step_index(povu_hip_ctx *ctx, const InvIn &in, InvDevice &v)
{
	hipStream_t s = ctx->stream;
	const uint64_t NR = in.ref.NR;
	InvIndex x;
	const StepIndex ix = build_step_index(ctx, ctx->iv_ws, [&](Spans &take) {
		take(NR + 1, x.hcnt, x.hoff, x.longs);
		take(scan_exclusive_u64_tmp(NR + 1), x.s64);
		take(8, x.words);
		take(1, x.n_long);
	});
	HIP_CHECK(hipMemsetAsync(x.words, 0, 32, s));
	HIP_CHECK(hipMemsetAsync(x.n_long, 0, 8, s));
	HIP_CHECK(hipMemsetAsync(x.hcnt, 0, (NR + 1) * 8, s));
	v.ioff = ix.ioff;
	v.occ = ix.occ;
	x.long_min = in.force_tier2 ? 0 : LONG_LIST;
	return x;
}

// count, scan, check, emit
static InvHeads run_heads(povu_hip_ctx *ctx, const InvView &A, InvIndex &x, InvDevice &v)
{
	hipStream_t s = ctx->stream;
	const uint64_t NR = A.ref.NR;
	InvHeads h;
	KLAUNCH(k_inv_heads<false>, dim3(stride_blocks(NR)), dim3(Q_TPB), 0, s, A, x.long_min, x.hcnt, x.hoff, (uint32_t *)nullptr, (uint32_t *)nullptr, x.longs,
		x.words);
	x.n_longs = read_back(x.words, s);
	if (x.n_longs)
		KLAUNCH(k_inv_heads_wave<false>, dim3(wave_blocks(x.n_longs)), dim3(Q_TPB), 0, s, A, x.longs, x.n_longs, x.hcnt, x.hoff, (uint32_t *)nullptr,
			(uint32_t *)nullptr);
	scan_exclusive_u64(x.hcnt, x.hoff, NR + 1, x.s64, s);
	const uint64_t H64 = read_back(x.hoff + NR, s);
	refuse_2_32(H64, "the call needs ", "inversion run heads");
	const uint32_t H = h.H = (uint32_t)H64;
	v.n_heads = H;
	if (!H)
		return h;
	const size_t h1 = (size_t)H + 1;
	h.tmp_bytes = prim_tmp_bytes(h1, true) + 256;
	carve(ctx->iv_heads, [&](Spans &take) {
		take(h1, h.hx, h.hy, h.hL, h.hslot, h.t2, h.rlist, h.perm2, h.key, h.key2, h.first, h.rank, h.flag);
		take(h1, v.run_rec, v.run_slot, v.ref, v.at, v.steps, v.dst, v.pos);
		take(h.tmp_bytes, h.tmp);
	});
	KLAUNCH(k_inv_heads<true>, dim3(stride_blocks(NR)), dim3(Q_TPB), 0, s, A, x.long_min, x.hcnt, x.hoff, h.hx, h.hy, x.longs, x.words);
	if (x.n_longs)
		KLAUNCH(k_inv_heads_wave<true>, dim3(wave_blocks(x.n_longs)), dim3(Q_TPB), 0, s, A, x.longs, x.n_longs, x.hcnt, x.hoff, h.hx, h.hy);
	return h;
}

static void extend(povu_hip_ctx *ctx, const InvIn &in, const InvView &A, const InvIndex &x, const InvHeads &h, InvDevice &v)
{
	hipStream_t s = ctx->stream;
	KLAUNCH(k_inv_extend, dim3(stride_blocks(h.H)), dim3(Q_TPB), 0, s, h.H, A, in.max_steps, in.force_tier2 ? 1u : 0u, h.hx, h.hy, h.hL, h.hslot,
		in.slots.slot_of_path, h.t2, x.words + 1);
	const uint32_t n_t2 = read_back(x.words + 1, s);
	v.n_tier2 = n_t2;
	if (n_t2)
		KLAUNCH(k_inv_extend_wave, dim3(wave_blocks(n_t2)), dim3(Q_TPB), 0, s, h.t2, n_t2, x.words + 2, A, in.max_steps, h.hx, h.hy, h.hL);
}

// the reported runs, sorted by (reference index, steps, slot); the first run of every (index, steps) group is a record
static void records(povu_hip_ctx *ctx, const InvIn &in, const InvView &A, const InvIndex &x, const InvHeads &h, InvDevice &v)
{
	hipStream_t s = ctx->stream;
	const uint32_t H = h.H;
	KLAUNCH(k_inv_report, dim3(stride_blocks(H)), dim3(Q_TPB), 0, s, H, in.max_steps, A, in.marked, h.hx, h.hL, in.ref.roff, h.flag, x.n_long);
	compact_flagged_u8(h.flag, H, h.rlist, x.words + 3, h.tmp, h.tmp_bytes, s);
	uint32_t n_runs = 0;
	unsigned long long h_long = 0;
	HIP_CHECK(copy_async(&n_runs, x.words + 3, 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(copy_async(&h_long, x.n_long, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	v.n_long = h_long;
	v.n_runs = n_runs;
	if (!n_runs)
		return;
	LsdSort sort{h.rlist, h.perm2, h.key, h.key2, n_runs, h.tmp, h.tmp_bytes, s};
	auto write_key = [&](int which, const uint32_t *perm, uint32_t *k) {
		KLAUNCH(k_inv_key, dim3(stride_blocks(n_runs)), dim3(Q_TPB), 0, s, n_runs, which, perm, h.hx, h.hL, h.hslot, k);
	};
	if (in.slots.S > 1)
		sort.pass(0, bits_for(in.slots.S - 1), write_key);
	sort.pass(1, bits_for(in.max_steps), write_key);
	sort.pass(2, bits_for(A.ref.NR), write_key);
	const uint32_t *cur = sort.cur;
	KLAUNCH(k_inv_group, dim3(stride_blocks((size_t)H + 1)), dim3(Q_TPB), 0, s, n_runs, cur, h.hx, h.hL, h.first);
	scan_exclusive_u32(h.first, h.rank, (size_t)n_runs + 1, h.tmp, h.tmp_bytes, s);
	HIP_CHECK(copy_async(&v.n, h.rank + n_runs, 4, hipMemcpyDeviceToHost, s));
	KLAUNCH(k_inv_records, dim3(stride_blocks(n_runs)), dim3(Q_TPB), 0, s, n_runs, A, cur, h.hx, h.hL, h.hslot, h.first, h.rank, in.ref.roff, v.run_rec,
		v.run_slot, v.ref, v.at, v.steps, v.pos);
	HIP_CHECK(hipStreamSynchronize(s));
}

InvDevice inv_find(povu_hip_ctx *ctx, const InvIn &in)
{
	const uint64_t N = ctx->n_path_steps;
	if (N >= 0xFFFFFFFFull - 4096) // (the sort of the step index takes fewer)
		throw HipError("inversion calls index every path step: " + std::to_string(N) + " steps, 2^32 or more are refused");
	InvDevice v;
	if (!N || !in.ref.NR)
		return v;
	InvIndex x = step_index(ctx, in, v);
	const InvView A = view_of(in, v);
	const InvHeads h = run_heads(ctx, A, x, v);
	if (!h.H)
		return v;
	extend(ctx, in, A, x, h, v);
	records(ctx, in, A, x, h, v);
	return v;
}

void inv_merge(povu_hip_ctx *ctx, InvDevice &v, uint32_t nrec, const uint32_t *f_ref, const uint64_t *f_pos, uint32_t *f_dst)
{
	hipStream_t s = ctx->stream;
	if (nrec)
		KLAUNCH(k_inv_rows_flubble, dim3(stride_blocks(nrec)), dim3(Q_TPB), 0, s, nrec, f_ref, f_pos, v.n, v.ref, v.pos, f_dst);
	if (v.n)
		KLAUNCH(k_inv_rows, dim3(stride_blocks(v.n)), dim3(Q_TPB), 0, s, v.n, v.ref, v.pos, nrec, f_ref, f_pos, v.dst);
}

void inv_fields(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, const InvRows &o)
{
	if (v.n)
		KLAUNCH(k_inv_fields, dim3(stride_blocks(v.n)), dim3(Q_TPB), 0, ctx->stream, v.n, view_of(in, v), v.ref, v.at, v.steps, v.pos, v.dst, o);
}

void inv_genotypes(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, const InvRows &o, uint32_t first_block, uint64_t *bcnt)
{
	if (!v.n)
		return;
	hipStream_t s = ctx->stream;
	const InvView A = view_of(in, v);
	KLAUNCH(k_inv_gt_init, dim3(stride_blocks((size_t)v.n * in.slots.S)), dim3(Q_TPB), 0, s, (uint64_t)v.n * in.slots.S, in.slots.S, first_block, A, v.ref, v.dst, in.slots.slot_of_path, o.gt,
		o.o_block, bcnt);
	KLAUNCH(k_inv_gt_mark, dim3(stride_blocks(v.n_runs)), dim3(Q_TPB), 0, s, v.n_runs, in.slots.S, A, v.run_rec, v.run_slot, v.ref, v.dst, in.slots.slot_of_path, o.gt);
}

void inv_counts(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, const InvRows &o, const uint64_t *ac_off, uint32_t *ac)
{
	if (v.n)
		KLAUNCH(k_inv_gt_count, dim3(wave_blocks(v.n)), dim3(Q_TPB), 0, ctx->stream, v.n, in.slots.S, in.slots.NS, in.slots.slot_first, v.dst, o.gt, ac_off, ac, o.o_an,
			o.o_ns, o.o_flags);
}

void inv_spell_len(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, const BlockLayout &L, uint64_t *slen, uint64_t *alen)
{
	const uint64_t s0 = L.inversion().s0;
	if (v.n)
		KLAUNCH(k_inv_spell_len, dim3(wave_blocks(v.n)), dim3(Q_TPB), 0, ctx->stream, v.n, view_of(in, v), v.at, v.steps, in.ref.roff, in.paths.vid,
			slen + s0, alen + s0);
}

void inv_emit(povu_hip_ctx *ctx, const InvIn &in, const InvDevice &v, const BlockLayout &L, const uint64_t *s_off, const uint64_t *a_off, char *o_seq,
	      char *o_at, unsigned long long *bad)
{
	const uint64_t s0 = L.inversion().s0;
	if (v.n)
		KLAUNCH(k_inv_emit, dim3(wave_blocks(2 * (size_t)v.n)), dim3(Q_TPB), 0, ctx->stream, 2 * (uint64_t)v.n, view_of(in, v), v.at, v.steps,
			in.paths.seq_off, in.paths.seq, in.paths.vid, s_off + s0, a_off + s0, o_seq, o_at, bad);
}

} // namespace povu_hip
