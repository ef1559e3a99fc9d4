// norm_kernels.hip -- left-normalisation of the flubble records of a call (POVU_HIP_PROFILE_LEFT_NORMALIZED).
//
// The definition is this project's own (INTEGRATION.md "Left-normalised calls"; restated in tests/norm_ref.py).  With A_0 the
// REF and A_1 .. A_n the ALTs a record writes, P its raw POS, C the bases of its reference path in front of P and
// E_i = C + A_i, compared after upper-casing:
//   chop    one wave per (record, ALT) walks E_0 and E_i backwards, 64 bases a step: a lane's base comes from the allele's steps
//           (a cursor over the steps, lanes across a segment's bytes) and, behind the allele's first base, from the
//           context (the step of the reference path that holds the base: a binary search in the path's slice of `roff`).
//           One ballot of "differs" ends the walk; atomicMin joins the ALTs of a record into its common suffix.  An ALT as
//           long as REF reads the same context bases as REF: its walk ends with the allele, and one that did not differ is
//           REF's text and takes no part;
//   record  one wave per record: the shortest allele (lanes across alleles), r and s from the closed form, and when s is 0
//           the common prefix of the chopped alleles (the same walk forwards over the allele heads), the new POS;
//   rows    the per-record arrays in sorted order, a block of spelled alleles per changed record;
//   emit    one wave per normalised allele: s context bases, then the allele cut to s + len - r, less its first u.
// Every index into `roff`, the path steps and the sequences is one the raw call reads too: a context base lies in front of
// P on the record's own reference path (P - 1 - s >= 0 by the cap on r), an allele base inside a traversal's steps.
#include "norm_kernels.hpp"

namespace povu_hip
{

namespace
{

__device__ __forceinline__ uint8_t nm_upper(uint8_t c) { return c >= 'a' && c <= 'z' ? (uint8_t)(c - 32) : c; }

// where a walk over an allele's inner steps stands: a step and a count of bases (what they mean: each walk's own)
struct NmCursor {
	uint32_t k;
	uint64_t cum;
};
// the bases at distances c0 .. c0 + 63 from the last base of the allele's text of alen bases, a lane each (0 where the allele
// has none).  `k` inner steps are not yet left behind, those left behind hold `cum` bases; called with ascending c0, by the whole wave
__device__ __forceinline__ uint8_t nm_back_chunk(const PathsView &P, const WrittenAllele &a, uint64_t alen, NmCursor &cur, uint64_t c0, uint32_t lane)
{
	const uint64_t d = c0 + lane;
	uint8_t c = 0;
	while (cur.k > 0) {
		const uint32_t x = a.inner_step(P.steps, cur.k - 1);
		const uint64_t n = path_step_len(P, x);
		if (d >= cur.cum && d < cur.cum + n)
			c = path_step_base(P, x, n - 1 - (d - cur.cum));
		if (cur.cum + n > c0 + 64)
			break; // (the step reaches into the next chunk)
		cur.cum += n;
		cur.k--;
	}
	if (cur.k == 0 && a.anchor_base && d + 1 == alen)
		c = path_step_base(P, a.anchor, path_step_len(P, a.anchor) - 1);
	return c;
}
// ... at indices x0 .. x0 + 63 from the allele's first base: `k` the next inner step, `cum` the index of its first base
__device__ __forceinline__ uint8_t nm_fwd_chunk(const PathsView &P, const WrittenAllele &a, NmCursor &cur, uint64_t x0, uint32_t lane)
{
	const uint64_t idx = x0 + lane;
	uint8_t c = 0;
	if (a.anchor_base && idx == 0)
		c = path_step_base(P, a.anchor, path_step_len(P, a.anchor) - 1);
	while (cur.k < a.inner_steps()) {
		const uint32_t x = a.inner_step(P.steps, cur.k);
		const uint64_t n = path_step_len(P, x);
		if (idx >= cur.cum && idx < cur.cum + n)
			c = path_step_base(P, x, idx - cur.cum);
		if (cur.cum + n > x0 + 64)
			break;
		cur.cum += n;
		cur.k++;
	}
	return c;
}

// the reference path of record j
__device__ __forceinline__ RefPathSlice nm_ref(const CallView &V, uint32_t j)
{
	return ref_path_slice(V.ref, V.paths, V.ref.ref_of_path[V.trav.op[V.rlist[j]]]);
}
// ALTs of every record (the tasks of k_nm_chop); none for a record with an empty allele text, which stays as it is: none of
// its comparisons is made or counted
__global__ void k_nm_tasks(CallView V, uint64_t *__restrict__ cnt)
{
	const uint32_t nfl = V.nfl;
	for (uint32_t j = blockIdx.x * Q_TPB + threadIdx.x; j <= nfl; j += gridDim.x * Q_TPB) {
		if (j == nfl) {
			cnt[j] = 0;
			continue;
		}
		const uint32_t q = V.trav.rq[V.rlist[j]], nal = V.aoff[q + 1] - V.aoff[q];
		bool empty = false;
		for (uint32_t i = 0; i < nal && !empty; i++)
			empty = allele_of_record(V, j, i).text_len() == 0;
		cnt[j] = empty ? 0 : nal - 1;
	}
}

// one wave per (record, ALT): the common suffix of E_0 and E_i into rmin[record]; words[0] += bases compared
__global__ __launch_bounds__(Q_TPB) void k_nm_chop(uint64_t ntask, CallView V, const uint64_t *__restrict__ toff,
						   unsigned long long *__restrict__ rmin, unsigned long long *__restrict__ words)
{
	const uint32_t lane = threadIdx.x & 63u, nfl = V.nfl;
	const PathsView P = V.paths; // (what the walk reads, out of the view)
	const uint64_t *__restrict__ roff = V.ref.roff;
	const uint64_t waves = (uint64_t)gridDim.x * (Q_TPB / 64);
	for (uint64_t task = (uint64_t)blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); task < ntask; task += waves) {
		const uint32_t j = span_of(toff, nfl, task), i = (uint32_t)(task - toff[j]) + 1;
		const WrittenAllele A = allele_of_record(V, j, 0), B = allele_of_record(V, j, i);
		const uint64_t la = A.text_len(), lb = B.text_len();
		if (!la || !lb)
			continue; // (an empty text: the record stays as it is)
		const RefPathSlice R = nm_ref(V, j);
		const uint64_t pos = V.raw_pos[j], ta = pos - 1 + la, tb = pos - 1 + lb;
		// behind `end` nothing is compared: alleles of one length read the same context base from there on, else the shorter
		// string has ended (and that is a difference)
		const uint64_t end = la == lb ? la : min(ta, tb) + 1;
		NmCursor ca{A.inner_steps(), 0}, cb{B.inner_steps(), 0};
		uint64_t L = end;
		uint32_t seg;
		for (uint64_t c0 = 0; c0 < end; c0 += 64) {
			const uint64_t d = c0 + lane;
			uint8_t x = 0, y = 0;
			if (c0 < la)
				x = nm_back_chunk(P, A, la, ca, c0, lane);
			if (c0 < lb)
				y = nm_back_chunk(P, B, lb, cb, c0, lane);
			if (d < end && d >= la && d < ta)
				x = ref_path_base(P, roff, R, pos - 2 - (d - la), &seg);
			if (d < end && d >= lb && d < tb)
				y = ref_path_base(P, roff, R, pos - 2 - (d - lb), &seg);
			const bool differs = d < end && (d >= ta || d >= tb || nm_upper(x) != nm_upper(y));
			const unsigned long long mask = __ballot(differs);
			if (mask) {
				L = c0 + (uint64_t)(__ffsll((long long)mask) - 1);
				break;
			}
		}
		if (lane == 0) {
			if (L == end) { // (alleles of one length that never differed: REF's text)
				atomicAdd(words, (unsigned long long)la);
			} else {
				atomicMin(rmin + j, (unsigned long long)L);
				atomicAdd(words, (unsigned long long)L + 1);
			}
		}
	}
}

// one wave per record: r, s, u and the new POS from the closed form; words[1] += changed, words[2] max shift, words[3] max chop
__global__ __launch_bounds__(Q_TPB) void k_nm_record(CallView V, const unsigned long long *__restrict__ rmin, uint8_t *__restrict__ rstate,
						     uint64_t *__restrict__ pos, uint64_t *__restrict__ raw_pos, uint64_t *__restrict__ chop,
						     uint64_t *__restrict__ shift, uint64_t *__restrict__ trim, unsigned long long *__restrict__ words)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64), nfl = V.nfl;
	const PathsView P = V.paths;
	for (uint32_t j = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); j < nfl; j += waves) {
		const uint32_t q = V.trav.rq[V.rlist[j]], nal = V.aoff[q + 1] - V.aoff[q];
		const WrittenAllele A = allele_of_record(V, j, 0);
		const uint64_t P0 = V.raw_pos[j];
		uint64_t mn = ~0ull;
		for (uint32_t i = lane; i < nal; i += 64)
			mn = min(mn, (i ? V.ilen[other_allele(V, j, i)] : V.xilen[j]) + (A.anchor_base ? 1 : 0));
		mn = wave_all_reduce(mn, MinOp{});
		const uint64_t rm = rmin[j];
		uint64_t r = 0, s = 0, u = 0;
		if (mn && rm != ~0ull) {
			r = min(rm, P0 + mn - 2);
			s = r + 1 > mn ? r + 1 - mn : 0;
			if (s == 0 && mn - r > 1) {
				u = mn - r - 1; // (every chopped allele keeps a base)
				for (uint32_t i = 1; i < nal && u; i++) {
					const WrittenAllele B = allele_of_record(V, j, i);
					NmCursor ca{0, A.anchor_base ? 1u : 0u}, cb{0, B.anchor_base ? 1u : 0u};
					for (uint64_t x0 = 0; x0 < u; x0 += 64) {
						const uint8_t x = nm_fwd_chunk(P, A, ca, x0, lane), y = nm_fwd_chunk(P, B, cb, x0, lane);
						const unsigned long long mask = __ballot(x0 + lane < u && nm_upper(x) != nm_upper(y));
						if (mask) {
							u = x0 + (uint64_t)(__ffsll((long long)mask) - 1);
							break;
						}
					}
				}
			}
		}
		if (lane == 0) {
			raw_pos[j] = P0;
			chop[j] = r;
			shift[j] = s;
			trim[j] = u;
			if (r || u) {
				rstate[j] |= RS_NORMALIZED;
				pos[j] = P0 - s + u;
				atomicAdd(words + 1, 1ull);
				atomicMax(words + 2, (unsigned long long)s);
				atomicMax(words + 3, (unsigned long long)r);
			}
		}
	}
}

__global__ void k_nm_rows(uint32_t nrec, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ dst, const uint8_t *__restrict__ rstate,
			  const uint64_t *__restrict__ raw_pos, const uint64_t *__restrict__ chop, const uint64_t *__restrict__ shift,
			  const uint64_t *__restrict__ trim, NormRows o)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i <= nrec; i += gridDim.x * Q_TPB) {
		if (i == nrec) {
			o.need[i] = 0;
			continue;
		}
		const uint32_t j = perm[i], d = dst ? dst[i] : i;
		o.o_raw_pos[d] = raw_pos[j];
		o.o_chop[d] = (uint32_t)chop[j];
		o.o_shift[d] = (uint32_t)shift[j];
		o.o_trim[d] = (uint32_t)trim[j];
		o.need[i] = (rstate[j] & RS_NORMALIZED) ? 1 : 0;
	}
}
__global__ void k_nm_blocks(uint32_t nrec, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ dst, NormRows o, uint32_t nb0,
			    CallView V, uint64_t *__restrict__ bcnt)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < nrec; i += gridDim.x * Q_TPB) {
		if (!o.need[i])
			continue;
		const uint32_t j = perm[i], q = V.trav.rq[V.rlist[j]], k = o.off[i];
		o.o_block[dst ? dst[i] : i] = nb0 + k;
		o.list[k] = j;
		bcnt[nb0 + k] = V.aoff[q + 1] - V.aoff[q];
	}
}

// the record and the written allele of spelled allele g of the normalised family
__device__ __forceinline__ uint32_t nm_spelled(uint64_t g, const BlockLayout::Family &F, const uint64_t *__restrict__ block_off,
					       const uint32_t *__restrict__ list, uint32_t *i)
{
	const uint32_t b = span_of(block_off + F.b0, F.nb, g);
	*i = (uint32_t)(g - block_off[F.b0 + b]);
	return list[b];
}
__global__ void k_nm_spell_len(BlockLayout::Family F, CallView V, const uint64_t *__restrict__ block_off, const uint32_t *__restrict__ list,
			       const uint64_t *__restrict__ chop, const uint64_t *__restrict__ shift, const uint64_t *__restrict__ trim,
			       uint64_t *__restrict__ slen, uint64_t *__restrict__ alen)
{
	for (uint64_t x = F.s0 + (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x < F.s0 + F.ns; x += (uint64_t)gridDim.x * Q_TPB) {
		uint32_t i;
		const uint32_t j = nm_spelled(x, F, block_off, list, &i);
		slen[x] = shift[j] + allele_of_record(V, j, i).text_len() - chop[j] - trim[j];
		alen[x] = 0;
	}
}
// one wave per normalised allele
__global__ __launch_bounds__(Q_TPB) void k_nm_emit(BlockLayout::Family F, CallView V, const uint64_t *__restrict__ block_off,
						   const uint32_t *__restrict__ list, const uint64_t *__restrict__ chop,
						   const uint64_t *__restrict__ shift, const uint64_t *__restrict__ trim,
						   const uint64_t *__restrict__ s_off, char *__restrict__ o_seq, unsigned long long *__restrict__ bad)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t waves = (uint64_t)gridDim.x * (Q_TPB / 64);
	const PathsView P = V.paths;
	const uint64_t *__restrict__ roff = V.ref.roff;
	for (uint64_t x = F.s0 + (uint64_t)blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); x < F.s0 + F.ns; x += waves) {
		uint32_t i;
		const uint32_t j = nm_spelled(x, F, block_off, list, &i);
		const WrittenAllele A = allele_of_record(V, j, i);
		const RefPathSlice R = nm_ref(V, j);
		const uint64_t pos = V.raw_pos[j], la = A.text_len(), r = chop[j], s = shift[j], u = trim[j], w = s_off[x];
		// (u > 0 only where s == 0: the context bases are never trimmed; an allele shorter than the chop ends inside them)
		const uint64_t nctx = la < r ? s + la - r : s;
		for (uint64_t z = lane; z < nctx; z += 64) {
			uint32_t seg;
			const uint8_t c = ref_path_base(P, roff, R, pos - 1 - s + z, &seg);
			if (!comp(c))
				atomicMin(bad, (unsigned long long)seg);
			o_seq[w + z] = (char)c;
		}
		if (la > r) {
			const uint64_t cut = la - r;
			NmCursor cur{0, A.anchor_base ? 1u : 0u};
			for (uint64_t x0 = 0; x0 < cut; x0 += 64) {
				const uint8_t c = nm_fwd_chunk(P, A, cur, x0, lane);
				const uint64_t idx = x0 + lane;
				if (idx < cut && idx >= u)
					o_seq[w + s + idx - u] = (char)c;
			}
		}
	}
}

} // namespace

NormRecs norm_records(povu_hip_ctx *ctx, const CallView &v, uint8_t *rstate, uint64_t *pos)
{
	hipStream_t s = ctx->stream;
	const uint32_t nfl = v.nfl;
	NormRecs n;
	uint64_t *cnt, *toff, *s64;
	unsigned long long *rmin, *words;
	carve(ctx->nm_ws, [&](Spans &take) {
		take((size_t)nfl + 1, cnt, toff, rmin, n.raw_pos, n.chop, n.shift, n.trim);
		take(4, words);
		take(scan_exclusive_u64_tmp((size_t)nfl + 1), s64);
	});
	HIP_CHECK(hipMemsetAsync(rmin, 0xFF, ((size_t)nfl + 1) * 8, s));
	HIP_CHECK(hipMemsetAsync(words, 0, 32, s));
	KLAUNCH(k_nm_tasks, dim3(stride_blocks((size_t)nfl + 1)), dim3(Q_TPB), 0, s, v, cnt);
	scan_exclusive_u64(cnt, toff, (size_t)nfl + 1, s64, s);
	const uint64_t ntask = read_back(toff + nfl, s);
	if (ntask)
		KLAUNCH(k_nm_chop, dim3(wave_blocks(ntask)), dim3(Q_TPB), 0, s, ntask, v, toff, rmin, words);
	KLAUNCH(k_nm_record, dim3(wave_blocks(nfl)), dim3(Q_TPB), 0, s, v, rmin, rstate, pos, n.raw_pos, n.chop, n.shift, n.trim, words);
	unsigned long long h[4] = {0, 0, 0, 0};
	HIP_CHECK(copy_async(h, words, 32, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	n.n_compared = h[0], n.n_changed = h[1], n.max_shift = h[2];
	refuse_2_32(std::max(h[2], h[3]), "left-normalisation moves a record by ", "bases");
	return n;
}

void norm_row_fields(povu_hip_ctx *ctx, const CallView &v, const NormRecs &n, uint32_t nrec, const uint32_t *perm, const uint32_t *dst, const NormRows &o)
{
	KLAUNCH(k_nm_rows, dim3(stride_blocks((size_t)nrec + 1)), dim3(Q_TPB), 0, ctx->stream, nrec, perm, dst, v.rstate, n.raw_pos, n.chop, n.shift, n.trim, o);
}

void norm_blocks(povu_hip_ctx *ctx, const CallView &v, uint32_t nrec, const uint32_t *perm, const uint32_t *dst, const NormRows &o, uint32_t first_block,
		 uint64_t *bcnt)
{
	if (nrec)
		KLAUNCH(k_nm_blocks, dim3(stride_blocks(nrec)), dim3(Q_TPB), 0, ctx->stream, nrec, perm, dst, o, first_block, v, bcnt);
}

void norm_spell_len(povu_hip_ctx *ctx, const CallView &v, const NormRecs &n, const NormRows &o, const BlockLayout &L, const uint64_t *block_off,
		    uint64_t *slen, uint64_t *alen)
{
	const BlockLayout::Family F = L.normalised();
	if (F.ns)
		KLAUNCH(k_nm_spell_len, dim3(stride_blocks(F.ns)), dim3(Q_TPB), 0, ctx->stream, F, v, block_off, o.list, n.chop, n.shift, n.trim, slen, alen);
}

void norm_emit(povu_hip_ctx *ctx, const CallView &v, const NormRecs &n, const NormRows &o, const BlockLayout &L, const uint64_t *block_off,
	       const uint64_t *s_off, char *o_seq, unsigned long long *bad)
{
	const BlockLayout::Family F = L.normalised();
	if (F.ns)
		KLAUNCH(k_nm_emit, dim3(wave_blocks(F.ns)), dim3(Q_TPB), 0, ctx->stream, F, v, block_off, o.list, n.chop, n.shift, n.trim, s_off, o_seq, bad);
}

} // namespace povu_hip
