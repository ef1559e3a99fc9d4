// call_kernels.hip -- the variant calls of a set of PVST vertices by reference paths (povu_hip_segments_upload,
// povu_hip_call; include/povu_hip.h).
//
// The definition is this project's own ("Variant calls"; restated in tests/vcf_ref.py).  A call runs the
// traversal pipeline (trav_kernels.hip) on the sites given and keeps its arrays on the device, then:
//   reference offsets  the segment lengths of the reference paths' steps, one exclusive u64 scan (a path's offsets are the
//                      scan minus its value at the path's first step);
//   callability        a CSR over the segments lists (site, boundary) pairs; a pass over the reference steps marks the
//                      (site, reference, boundary) bits it meets; presence per (tree, reference) is the OR over the tree's
//                      sites; a site is callable when no subflubble lies on its way to the root, some reference is present
//                      and every present reference has both bits; a callable site clears its parent's "called" flag;
//   slot table         per called site of two alleles or more and per genotype slot, the min and max allele (atomics);
//   records            the reference traversals of those sites, compacted, radix-sorted by (reference, POS) (stable, so
//                      ties keep (site, first step) order); per record one wave, a lane per sample: GT codes, AC, AN, NS,
//                      TANGLED;
//   spelling           per (site, orientation) a record needs, every allele: lengths, u64 scans, then one wave per allele
//                      copies the bases (reverse-complemented on '<' steps, lanes across a segment's bytes) and writes the
//                      AT step string (lanes across steps, a wave prefix sum of their decimal widths).
#include "call_common.hpp"

namespace povu_hip
{

static constexpr int SC_E = 4, SC_N = C_TPB * SC_E; // u64 scan: elements per thread / per block
static constexpr uint32_t MAX_ALLELES = 65534;
static constexpr uint64_t ROLE = 1ull << 63; // (trav_kernels.hip: reverse traversals carry it in rpos)
// step k (S -> Z) of a traversal at path words [pos, pos + len), reversed and flipped when rev (as trav_kernels.hip reads it)
__device__ __forceinline__ uint32_t tstep(const uint32_t *__restrict__ steps, uint64_t pos, uint32_t len, bool rev, uint32_t k)
{
	return rev ? steps[pos + len - 1 - k] ^ 1u : steps[pos + k];
}

// ---- exclusive u64 scan: per block of SC_N an LDS scan, the block sums scanned recursively, then added
__global__ __launch_bounds__(C_TPB) void k_c64_scan(const uint64_t *in, uint64_t *out, size_t n, uint64_t *__restrict__ sums)
{
	__shared__ uint64_t sh[C_TPB];
	const size_t base = (size_t)blockIdx.x * SC_N + (size_t)threadIdx.x * SC_E;
	uint64_t v[SC_E], t = 0;
	for (int k = 0; k < SC_E; k++) {
		v[k] = base + k < n ? in[base + k] : 0;
		t += v[k];
	}
	sh[threadIdx.x] = t;
	__syncthreads();
	for (int d = 1; d < C_TPB; d <<= 1) {
		const uint64_t x = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
		__syncthreads();
		sh[threadIdx.x] += x;
		__syncthreads();
	}
	uint64_t run = sh[threadIdx.x] - t;
	for (int k = 0; k < SC_E; k++) {
		if (base + k < n)
			out[base + k] = run;
		run += v[k];
	}
	if (threadIdx.x == C_TPB - 1)
		sums[blockIdx.x] = sh[C_TPB - 1];
}
__global__ __launch_bounds__(C_TPB) void k_c64_add(uint64_t *out, size_t n, const uint64_t *__restrict__ offs)
{
	const size_t base = (size_t)blockIdx.x * SC_N;
	const uint64_t o = offs[blockIdx.x];
	for (size_t i = base + threadIdx.x; i < n && i < base + SC_N; i += C_TPB)
		out[i] += o;
}
size_t scan64_tmp(size_t n)
{
	size_t t = 2;
	while (n > 1) {
		n = (n + SC_N - 1) / SC_N;
		t += n + 1;
	}
	return t;
}
void scan64(const uint64_t *in, uint64_t *out, size_t n, uint64_t *tmp, hipStream_t s)
{
	if (!n)
		return;
	const size_t nb = (n + SC_N - 1) / SC_N;
	KLAUNCH(k_c64_scan, dim3((unsigned)nb), dim3(C_TPB), 0, s, in, out, n, tmp);
	if (nb > 1) {
		scan64(tmp, tmp, nb, tmp + nb + 1, s);
		KLAUNCH(k_c64_add, dim3((unsigned)nb), dim3(C_TPB), 0, s, out, n, tmp);
	}
}

// ---- reference offsets: length of every reference step (ref_base: first step of every reference in the concatenation)
__global__ void k_cl_ref_len(uint64_t NR, const uint64_t *__restrict__ ref_base, uint32_t nR, const uint32_t *__restrict__ ref_path,
			     const uint64_t *__restrict__ path_off, const uint32_t *__restrict__ steps, const uint64_t *__restrict__ seq_off,
			     uint64_t *__restrict__ len)
{
	for (uint64_t i = (uint64_t)blockIdx.x * C_TPB + threadIdx.x; i < NR; i += (uint64_t)gridDim.x * C_TPB) {
		const uint32_t r = seg_of(ref_base, nR, i);
		const uint32_t x = steps[path_off[ref_path[r]] + (i - ref_base[r])];
		len[i] = seq_off[(x >> 1) + 1] - seq_off[x >> 1];
	}
}

// ---- segment -> (site, boundary) CSR
__global__ void k_cl_seg_count(uint32_t n, const uint32_t *__restrict__ qa, const uint32_t *__restrict__ qz, const uint32_t *__restrict__ vid,
			       uint32_t V, uint32_t *__restrict__ cnt, uint32_t *__restrict__ qv)
{
	for (uint32_t q = blockIdx.x * C_TPB + threadIdx.x; q < n; q += gridDim.x * C_TPB) {
		const uint32_t a = find_vertex(vid, V, qa[q]), z = find_vertex(vid, V, qz[q]);
		qv[2 * (size_t)q] = a;
		qv[2 * (size_t)q + 1] = z;
		if (a != NO_QUERY)
			atomicAdd(cnt + a, 1u);
		if (z != NO_QUERY)
			atomicAdd(cnt + z, 1u);
	}
}
__global__ void k_cl_seg_fill(uint32_t n, const uint32_t *__restrict__ qv, const uint32_t *__restrict__ off, uint32_t *__restrict__ cur,
			      uint32_t *__restrict__ val)
{
	for (uint64_t e = (uint64_t)blockIdx.x * C_TPB + threadIdx.x; e < 2 * (uint64_t)n; e += (uint64_t)gridDim.x * C_TPB) {
		const uint32_t v = qv[e];
		if (v != NO_QUERY)
			val[off[v] + atomicAdd(cur + v, 1u)] = (uint32_t)e; // (site << 1 | boundary)
	}
}

// ---- (site, reference, boundary) bits met by the reference steps
__global__ void k_cl_hits(uint64_t NR, const uint64_t *__restrict__ ref_base, uint32_t nR, const uint32_t *__restrict__ ref_path,
			  const uint64_t *__restrict__ path_off, const uint32_t *__restrict__ steps, const uint32_t *__restrict__ off,
			  const uint32_t *__restrict__ val, uint32_t *__restrict__ hit)
{
	for (uint64_t i = (uint64_t)blockIdx.x * C_TPB + threadIdx.x; i < NR; i += (uint64_t)gridDim.x * C_TPB) {
		const uint32_t r = seg_of(ref_base, nR, i);
		const uint32_t v = steps[path_off[ref_path[r]] + (i - ref_base[r])] >> 1;
		for (uint32_t e = off[v]; e < off[v + 1]; e++) {
			const uint32_t qr = val[e];
			const uint64_t bit = ((uint64_t)(qr >> 1) * nR + r) * 2 + (qr & 1u);
			atomicOr(hit + (bit >> 5), 1u << (bit & 31));
		}
	}
}
__device__ __forceinline__ uint32_t hits_of(const uint32_t *__restrict__ hit, uint64_t q, uint32_t nR, uint32_t r)
{
	const uint64_t bit = (q * nR + r) * 2;
	return (hit[bit >> 5] >> (bit & 31)) & 3u;
}
__device__ __forceinline__ bool bit_of(const uint32_t *__restrict__ w, uint64_t b) { return (w[b >> 5] >> (b & 31)) & 1u; }

__global__ void k_cl_present(uint64_t nq, uint32_t nR, const uint32_t *__restrict__ hit, const uint32_t *__restrict__ tree,
			     uint32_t *__restrict__ present)
{
	for (uint64_t i = (uint64_t)blockIdx.x * C_TPB + threadIdx.x; i < nq * nR; i += (uint64_t)gridDim.x * C_TPB) {
		const uint64_t q = i / nR;
		const uint32_t r = (uint32_t)(i % nR);
		if (hits_of(hit, q, nR, r)) {
			const uint64_t b = (uint64_t)tree[q] * nR + r;
			atomicOr(present + (b >> 5), 1u << (b & 31));
		}
	}
}

__device__ __forceinline__ bool is_sub(uint8_t f) { return f == 'T' || f == 'O' || f == 'C' || f == 'M' || f == 'S'; }

__global__ void k_cl_callable(uint32_t n, uint32_t nR, const uint32_t *__restrict__ hit, const uint32_t *__restrict__ present,
			      const uint32_t *__restrict__ tree, const uint32_t *__restrict__ parent, const uint8_t *__restrict__ fam,
			      uint8_t *__restrict__ callable, uint8_t *__restrict__ called)
{
	for (uint32_t q = blockIdx.x * C_TPB + threadIdx.x; q < n; q += gridDim.x * C_TPB) {
		bool skip = false;
		for (uint32_t v = q, k = 0; v != NO_QUERY && k <= n; v = parent[v], k++)
			skip |= is_sub(fam[v]);
		bool any = false, ok = true;
		for (uint32_t r = 0; r < nR && !skip; r++) {
			if (bit_of(present, (uint64_t)tree[q] * nR + r)) {
				any = true;
				ok &= hits_of(hit, q, nR, r) == 3u;
			}
		}
		callable[q] = called[q] = !skip && any && ok;
	}
}
__global__ void k_cl_unparent(uint32_t n, const uint8_t *__restrict__ callable, const uint32_t *__restrict__ parent, uint8_t *__restrict__ called)
{
	for (uint32_t q = blockIdx.x * C_TPB + threadIdx.x; q < n; q += gridDim.x * C_TPB)
		if (callable[q] && parent[q] != NO_QUERY)
			called[parent[q]] = 0;
}
// kept sites: called, two alleles or more
__global__ void k_cl_keep(uint32_t n, const uint8_t *__restrict__ called, const uint32_t *__restrict__ aoff, uint32_t *__restrict__ keep,
			  uint32_t *__restrict__ maxal)
{
	for (uint32_t q = blockIdx.x * C_TPB + threadIdx.x; q <= n; q += gridDim.x * C_TPB) {
		const uint32_t nal = q < n ? aoff[q + 1] - aoff[q] : 0;
		keep[q] = q < n && called[q] && nal >= 2;
		if (keep[q])
			atomicMax(maxal, nal);
	}
}

// inner bases and AT width of every allele (of a kept site), S -> Z
__global__ void k_cl_inner(uint32_t n_al, const uint32_t *__restrict__ afirst, const uint32_t *__restrict__ rq, const uint32_t *__restrict__ keep,
			   const uint64_t *__restrict__ rpos, const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ steps,
			   const uint64_t *__restrict__ seq_off, const uint32_t *__restrict__ vid, uint64_t *__restrict__ ilen,
			   uint64_t *__restrict__ atl)
{
	for (uint32_t a = blockIdx.x * C_TPB + threadIdx.x; a < n_al; a += gridDim.x * C_TPB) {
		const uint32_t t = afirst[a];
		uint64_t b = 0, w = 0;
		if (keep[rq[t]]) {
			const uint64_t p = rpos[t] & ~ROLE;
			const bool rev = (rpos[t] & ROLE) != 0;
			const uint32_t len = rlen[t];
			for (uint32_t k = 1; k + 1 < len; k++) {
				const uint32_t v = tstep(steps, p, len, rev, k) >> 1;
				b += seq_off[v + 1] - seq_off[v];
				w += 1 + ndig(vid[v]);
			}
		}
		ilen[a] = b;
		atl[a] = w;
	}
}
__global__ void k_cl_anchored(uint32_t n, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ aoff, const uint64_t *__restrict__ ilen,
			      uint8_t *__restrict__ anchored)
{
	for (uint32_t q = blockIdx.x * C_TPB + threadIdx.x; q < n; q += gridDim.x * C_TPB) {
		bool e = false;
		if (keep[q])
			for (uint32_t a = aoff[q]; a < aoff[q + 1]; a++)
				e |= ilen[a] == 0;
		anchored[q] = e;
	}
}

// min / max allele of every (kept site, slot)
__global__ void k_cl_slots(uint32_t R, const uint32_t *__restrict__ rq, const uint32_t *__restrict__ op, const uint32_t *__restrict__ oa,
			   const uint32_t *__restrict__ keep, const uint32_t *__restrict__ qidx, const uint32_t *__restrict__ slot_of_path,
			   uint32_t S, uint32_t *__restrict__ smin, uint32_t *__restrict__ smax)
{
	for (uint32_t t = blockIdx.x * C_TPB + threadIdx.x; t < R; t += gridDim.x * C_TPB) {
		const uint32_t q = rq[t];
		if (!keep[q])
			continue;
		const uint64_t i = (uint64_t)qidx[q] * S + slot_of_path[op[t]];
		atomicMin(smin + i, oa[t]);
		atomicMax(smax + i, oa[t]);
	}
}
__global__ void k_cl_rec_flag(uint32_t R, const uint32_t *__restrict__ rq, const uint32_t *__restrict__ op, const uint32_t *__restrict__ keep,
			      const uint32_t *__restrict__ ref_of_path, uint8_t *__restrict__ flag)
{
	for (uint32_t t = blockIdx.x * C_TPB + threadIdx.x; t < R; t += gridDim.x * C_TPB)
		flag[t] = keep[rq[t]] && ref_of_path[op[t]] != NO_QUERY;
}
__global__ void k_cl_pos(uint32_t nrec, const uint32_t *__restrict__ rlist, const uint32_t *__restrict__ rq, const uint32_t *__restrict__ op,
			 const uint32_t *__restrict__ of, const uint32_t *__restrict__ ref_of_path, const uint64_t *__restrict__ ref_base,
			 const uint64_t *__restrict__ roff, const uint8_t *__restrict__ anchored, uint64_t *__restrict__ pos,
			 uint32_t *__restrict__ perm)
{
	for (uint32_t i = blockIdx.x * C_TPB + threadIdx.x; i < nrec; i += gridDim.x * C_TPB) {
		const uint32_t t = rlist[i];
		const uint64_t b = ref_base[ref_of_path[op[t]]];
		pos[i] = roff[b + of[t] + 1] - roff[b] + (anchored[rq[t]] ? 0 : 1);
		perm[i] = i;
	}
}
// sort key of record perm[i]: 0 = POS low word, 1 = POS high word, 2 = reference
__global__ void k_cl_key(uint32_t nrec, int which, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ rlist,
			 const uint32_t *__restrict__ op, const uint32_t *__restrict__ ref_of_path, const uint64_t *__restrict__ pos,
			 uint32_t *__restrict__ key)
{
	for (uint32_t i = blockIdx.x * C_TPB + threadIdx.x; i < nrec; i += gridDim.x * C_TPB) {
		const uint32_t j = perm[i];
		key[i] = which == 0 ? (uint32_t)pos[j] : which == 1 ? (uint32_t)(pos[j] >> 32) : ref_of_path[op[rlist[j]]];
	}
}

// per record (sorted; row dst[i] of the record list when inversion records are merged in, else row i): its fields, the ALT count for the AC offsets, the (site, orientation) it needs spelled
__global__ void k_cl_rec_fields(uint32_t nrec, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ rlist, const uint64_t *__restrict__ pos,
				const uint32_t *__restrict__ rq, const uint32_t *__restrict__ op, const uint32_t *__restrict__ of,
				const uint32_t *__restrict__ oa, const uint8_t *__restrict__ orv, const uint32_t *__restrict__ aoff,
				uint32_t *__restrict__ o_q, uint32_t *__restrict__ o_path, uint32_t *__restrict__ o_first,
				uint32_t *__restrict__ o_ref, uint32_t *__restrict__ o_nal, uint64_t *__restrict__ o_pos, uint64_t *__restrict__ nalt,
				uint32_t *__restrict__ need, const uint32_t *__restrict__ dst)
{
	for (uint32_t i = blockIdx.x * C_TPB + threadIdx.x; i < nrec; i += gridDim.x * C_TPB) {
		const uint32_t j = perm[i], t = rlist[j], q = rq[t], d = dst ? dst[i] : i;
		o_q[d] = q;
		o_path[d] = op[t];
		o_first[d] = of[t];
		o_ref[d] = oa[t];
		o_nal[d] = aoff[q + 1] - aoff[q];
		o_pos[d] = pos[j];
		nalt[d] = aoff[q + 1] - aoff[q] - 1;
		need[2 * (size_t)q + orv[t]] = 1;
	}
}
// reference number and POS of the sorted records (the inversion records are merged in by them)
__global__ void k_cl_sorted_keys(uint32_t nrec, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ rlist, const uint32_t *__restrict__ op,
				 const uint32_t *__restrict__ ref_of_path, const uint64_t *__restrict__ pos, uint32_t *__restrict__ f_ref,
				 uint64_t *__restrict__ f_pos)
{
	for (uint32_t i = blockIdx.x * C_TPB + threadIdx.x; i < nrec; i += gridDim.x * C_TPB) {
		f_ref[i] = ref_of_path[op[rlist[perm[i]]]];
		f_pos[i] = pos[perm[i]];
	}
}

// GT codes, AC, AN, NS and flags: one wave per record, a lane per sample (its slots are consecutive)
__global__ __launch_bounds__(C_TPB) void k_cl_records(uint32_t nrec, const uint32_t *__restrict__ o_q, const uint32_t *__restrict__ o_path,
						      const uint32_t *__restrict__ o_ref, const uint32_t *__restrict__ qidx,
						      const uint32_t *__restrict__ slot_of_path, const uint32_t *__restrict__ slot_first,
						      uint32_t n_samples, uint32_t S, const uint32_t *__restrict__ smin,
						      const uint32_t *__restrict__ smax, const uint64_t *__restrict__ ac_off,
						      const uint32_t *__restrict__ qstatus, const uint8_t *__restrict__ anchored,
						      const uint32_t *__restrict__ aoff, const uint64_t *__restrict__ ilen, uint16_t *__restrict__ gt,
						      uint32_t *__restrict__ ac, uint32_t *__restrict__ an, uint32_t *__restrict__ ns,
						      uint8_t *__restrict__ flags, const uint32_t *__restrict__ dst)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (C_TPB / 64);
	for (uint32_t i0 = blockIdx.x * (C_TPB / 64) + (threadIdx.x >> 6); i0 < nrec; i0 += waves) {
		const uint32_t i = dst ? dst[i0] : i0;
		const uint32_t q = o_q[i], ra = o_ref[i], own = slot_of_path[o_path[i]];
		const uint64_t base = (uint64_t)qidx[q] * S;
		uint32_t n_an = 0, n_ns = 0, amb = 0;
		for (uint32_t sm = lane; sm < n_samples; sm += 64) {
			bool any = false;
			for (uint32_t sl = slot_first[sm]; sl < slot_first[sm + 1]; sl++) {
				uint32_t code = POVU_HIP_GT_MISSING;
				if (sl == own) {
					code = 0;
				} else {
					const uint32_t mn = smin[base + sl], mx = smax[base + sl];
					if (mn != 0xFFFFFFFFu && mn == mx)
						code = mn == ra ? 0 : mn < ra ? mn + 1 : mn;
					else if (mn != 0xFFFFFFFFu)
						amb = 1;
				}
				gt[(uint64_t)i * S + sl] = (uint16_t)code;
				if (code != POVU_HIP_GT_MISSING) {
					any = true;
					n_an++;
					if (code)
						atomicAdd(ac + ac_off[i] + code - 1, 1u);
				}
			}
			n_ns += any;
		}
		n_an = wave_sum(n_an);
		n_ns = wave_sum(n_ns);
		amb = wave_sum(amb);
		if (lane == 0) {
			an[i] = n_an;
			ns[i] = n_ns;
			uint8_t f = 0;
			if (anchored[q])
				f |= POVU_HIP_CALL_ANCHORED | (ilen[aoff[q] + ra] == 0 ? POVU_HIP_CALL_INS : POVU_HIP_CALL_DEL);
			if (qstatus[q] || amb)
				f |= POVU_HIP_CALL_TANGLED;
			flags[i] = f;
		}
	}
}

__global__ void k_cl_blocks(uint64_t n2, const uint32_t *__restrict__ need, const uint32_t *__restrict__ boff, uint32_t *__restrict__ blist)
{
	for (uint64_t x = (uint64_t)blockIdx.x * C_TPB + threadIdx.x; x < n2; x += (uint64_t)gridDim.x * C_TPB)
		if (need[x])
			blist[boff[x]] = (uint32_t)x;
}
__global__ void k_cl_rec_block(uint32_t nrec, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ rlist,
			       const uint32_t *__restrict__ rq, const uint8_t *__restrict__ orv, const uint32_t *__restrict__ boff,
			       uint32_t *__restrict__ o_block, const uint32_t *__restrict__ dst)
{
	for (uint32_t i = blockIdx.x * C_TPB + threadIdx.x; i < nrec; i += gridDim.x * C_TPB) {
		const uint32_t t = rlist[perm[i]];
		o_block[dst ? dst[i] : i] = boff[2 * (size_t)rq[t] + orv[t]];
	}
}
__global__ void k_cl_block_cnt(uint32_t nb, const uint32_t *__restrict__ blist, const uint32_t *__restrict__ aoff, uint64_t *__restrict__ cnt)
{
	for (uint32_t b = blockIdx.x * C_TPB + threadIdx.x; b < nb; b += gridDim.x * C_TPB) {
		const uint32_t q = blist[b] >> 1;
		cnt[b] = aoff[q + 1] - aoff[q];
	}
}

// what spelled allele j is: its block's site and orientation, its global allele, the first step in the reference's
// direction (the anchor step)
struct Spelled {
	uint32_t q, o, a, t, len, first;
	uint64_t p;
	bool rev;
};
__device__ __forceinline__ Spelled spelled(uint64_t j, uint32_t nb, const uint64_t *__restrict__ block_off, const uint32_t *__restrict__ blist,
					   const uint32_t *__restrict__ aoff, const uint32_t *__restrict__ afirst, const uint64_t *__restrict__ rpos,
					   const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ steps)
{
	Spelled s;
	const uint32_t b = seg_of(block_off, nb, j);
	s.q = blist[b] >> 1;
	s.o = blist[b] & 1u;
	s.a = aoff[s.q] + (uint32_t)(j - block_off[b]);
	s.t = afirst[s.a];
	s.p = rpos[s.t] & ~ROLE;
	s.rev = (rpos[s.t] & ROLE) != 0;
	s.len = rlen[s.t];
	s.first = s.o ? tstep(steps, s.p, s.len, s.rev, s.len - 1) ^ 1u : tstep(steps, s.p, s.len, s.rev, 0);
	return s;
}
// inner step k (0-based) in the reference's direction
__device__ __forceinline__ uint32_t inner_step(const Spelled &s, const uint32_t *__restrict__ steps, uint32_t k)
{
	return s.o ? tstep(steps, s.p, s.len, s.rev, s.len - 2 - k) ^ 1u : tstep(steps, s.p, s.len, s.rev, k + 1);
}

__global__ void k_cl_spell_len(uint64_t nsp, uint32_t nb, const uint64_t *__restrict__ block_off, const uint32_t *__restrict__ blist,
			       const uint32_t *__restrict__ aoff, const uint32_t *__restrict__ afirst, const uint64_t *__restrict__ rpos,
			       const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ steps, const uint64_t *__restrict__ seq_off,
			       const uint32_t *__restrict__ vid, const uint64_t *__restrict__ ilen, const uint64_t *__restrict__ atl,
			       const uint8_t *__restrict__ anchored, uint64_t *__restrict__ slen, uint64_t *__restrict__ alen)
{
	for (uint64_t j = (uint64_t)blockIdx.x * C_TPB + threadIdx.x; j < nsp; j += (uint64_t)gridDim.x * C_TPB) {
		const Spelled s = spelled(j, nb, block_off, blist, aoff, afirst, rpos, rlen, steps);
		const uint32_t v = s.first >> 1;
		const bool an = anchored[s.q];
		slen[j] = ilen[s.a] + (an && seq_off[v + 1] > seq_off[v] ? 1 : 0);
		alen[j] = atl[s.a] + (an ? 1 + ndig(vid[v]) : 0);
	}
}

// one wave per spelled allele: the bases, then the AT string
__global__ __launch_bounds__(C_TPB) void k_cl_emit(uint64_t nsp, uint32_t nb, const uint64_t *__restrict__ block_off,
						   const uint32_t *__restrict__ blist, const uint32_t *__restrict__ aoff,
						   const uint32_t *__restrict__ afirst, const uint64_t *__restrict__ rpos,
						   const uint32_t *__restrict__ rlen, const uint32_t *__restrict__ steps,
						   const uint64_t *__restrict__ seq_off, const char *__restrict__ seq, const uint32_t *__restrict__ vid,
						   const uint8_t *__restrict__ anchored, const uint64_t *__restrict__ s_off,
						   const uint64_t *__restrict__ a_off, char *__restrict__ o_seq, char *__restrict__ o_at,
						   unsigned long long *__restrict__ bad)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t waves = (uint64_t)gridDim.x * (C_TPB / 64);
	for (uint64_t j = (uint64_t)blockIdx.x * (C_TPB / 64) + (threadIdx.x >> 6); j < nsp; j += waves) {
		const Spelled s = spelled(j, nb, block_off, blist, aoff, afirst, rpos, rlen, steps);
		const bool an = anchored[s.q];
		uint64_t w = s_off[j], wa = a_off[j];
		const uint32_t m = s.len - 2; // inner steps
		// the anchor: last base of the first step, and its step text
		if (an) {
			const uint32_t v = s.first >> 1;
			const uint64_t b0 = seq_off[v], b1 = seq_off[v + 1];
			if (b1 > b0) {
				if (lane == 0) {
					const uint8_t c = (uint8_t)seq[(s.first & 1u) ? b0 : b1 - 1], r = comp(c);
					if (!r)
						atomicMin(bad, (unsigned long long)v);
					o_seq[w] = (char)((s.first & 1u) ? r : c);
				}
				w++;
			}
			const uint32_t width = 1 + ndig(vid[v]);
			if (lane == 0)
				put_step(o_at, vid, s.first, wa, width);
			wa += width;
		}
		emit_steps(lane, m, [&](uint32_t k) { return inner_step(s, steps, k); }, seq_off, seq, vid, w, wa, o_seq, o_at, bad);
	}
}

static void check_call_32(uint64_t v, const char *what)
{
	if (v >= 0xFFFFFFFFull)
		throw HipError(std::string("the call needs ") + std::to_string(v) + " " + what + ": 2^32 or more are refused");
}

} // namespace povu_hip

// ---- C ABI

extern "C" int povu_hip_segments_upload(povu_hip_ctx *ctx, uint32_t n_vtx, const uint64_t *seq_off, const char *seq, char *err,
					size_t errlen)
{
	return guarded_call(ctx, err, errlen, 1, [&] {
		if (!ctx)
			throw HipError("null context");
		if (!ctx->g.block)
			throw HipError("sequences need a resident graph (povu_hip_graph_upload first)");
		ctx->seq_valid = false;
		if (n_vtx != ctx->g.V)
			throw HipError("sequences of " + std::to_string(n_vtx) + " segments for a resident graph of " + std::to_string(ctx->g.V));
		if (!seq_off || seq_off[0] != 0)
			throw HipError("seq_off[0] must be 0");
		for (uint32_t v = 0; v < n_vtx; v++)
			if (seq_off[v + 1] < seq_off[v])
				throw HipError("sequence offsets of vertex " + std::to_string(v) + " decrease");
		const uint64_t B = seq_off[n_vtx];
		if (B && !seq)
			throw HipError("null sequence bytes");
		HIP_CHECK(hipSetDevice(ctx->device));
		ctx->wait_tail();
		carve(
			ctx->seq_buf,
			[&](Spans &take) {
				take((size_t)n_vtx + 1, ctx->seq_off);
				take(B + 8, ctx->seq);
			},
			false);
		hipStream_t s = ctx->stream;
		HIP_CHECK(copy_async(ctx->seq_off, seq_off, ((size_t)n_vtx + 1) * 8, hipMemcpyHostToDevice, s));
		if (B)
			HIP_CHECK(copy_async(ctx->seq, seq, B, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipStreamSynchronize(s));
		ctx->seq_gen = ctx->g.gen;
		ctx->seq_valid = true;
		return 0;
	});
}

namespace
{
struct CallsOwner {
	povu_hip_calls view{}; // first member: the owner is recovered from it in povu_hip_calls_free
	PinnedVec<uint32_t> query, path, first, ref_allele, n_alleles, an, ns, block, ac, n_steps;
	PinnedVec<uint64_t> pos, ac_off, block_off, seq_off, at_off;
	PinnedVec<uint8_t> flags;
	PinnedVec<uint16_t> gt;
	PinnedVec<char> seq, at;
	std::vector<uint64_t> contig_len;
};
} // namespace

extern "C" povu_hip_calls *povu_hip_call(povu_hip_ctx *ctx, const povu_hip_sites *sites, const povu_hip_call_refs *refs,
					 const uint32_t *slot_of_path, const povu_hip_trav_opts *opts, char *err, size_t errlen)
{
	using namespace povu_hip;
	CallTimer timer;
	return guarded_call(ctx, err, errlen, (povu_hip_calls *)nullptr, [&] {
		if (!ctx || !sites || !refs)
			throw HipError("null context, sites or references");
		if (!ctx->g.block)
			throw HipError("a call needs a resident graph (povu_hip_graph_upload first)");
		if (!ctx->seq_valid || ctx->seq_gen != ctx->g.gen)
			throw HipError("no sequences are resident for the graph now uploaded (povu_hip_segments_upload after povu_hip_graph_upload)");
		if (!ctx->paths_valid || ctx->paths_gen != ctx->g.gen)
			throw HipError("no paths are resident for the graph now uploaded (povu_hip_paths_upload after povu_hip_graph_upload)");
		const uint32_t n = sites->n, P = ctx->n_paths, nR = refs->n_refs, S = refs->n_slots, NS = refs->n_samples;
		if (n >= 0x7FFFFFFFu)
			throw HipError("too many sites");
		if (n && (!sites->id1 || !sites->id2 || !sites->or1 || !sites->or2 || !sites->parent || !sites->family || !sites->tree))
			throw HipError("null site arrays");
		if (!nR || !refs->ref_path)
			throw HipError("no reference path");
		if (!slot_of_path || !S || !NS || !refs->sample_of_slot)
			throw HipError("no genotype slots");
		std::vector<uint32_t> ref_of_path(P, NO_QUERY), slot_first(NS + 1, 0);
		for (uint32_t r = 0; r < nR; r++) {
			if (refs->ref_path[r] >= P || (r && refs->ref_path[r] <= refs->ref_path[r - 1]))
				throw HipError("reference paths must be ascending indices of resident paths");
			ref_of_path[refs->ref_path[r]] = r;
		}
		for (uint32_t k = 0; k < P; k++)
			if (slot_of_path[k] >= S)
				throw HipError("path " + std::to_string(k) + " has no genotype slot");
		for (uint32_t sl = 0; sl < S; sl++) {
			const uint32_t sm = refs->sample_of_slot[sl];
			if (sm >= NS || (sl && sm < refs->sample_of_slot[sl - 1]) || (sl && sm > refs->sample_of_slot[sl - 1] + 1) || (!sl && sm))
				throw HipError("the slots of a sample must be consecutive, samples in order");
			slot_first[sm + 1] = sl + 1;
		}
		uint32_t n_trees = 0;
		std::vector<uint32_t> qa(n), qz(n);
		std::vector<uint8_t> qor(n);
		for (uint32_t q = 0; q < n; q++) {
			if (sites->parent[q] != POVU_HIP_NIL && sites->parent[q] >= n)
				throw HipError("site " + std::to_string(q) + " has a parent that is no site");
			n_trees = std::max(n_trees, sites->tree[q] + 1);
			qa[q] = sites->id1[q];
			qz[q] = sites->id2[q];
			qor[q] = (uint8_t)((sites->or1[q] & 1u) | ((sites->or2[q] & 1u) << 1));
		}
		const ResidentGraph &g = ctx->g;
		hipStream_t s = ctx->stream;
		const TravDevice d = trav_pipeline(
			ctx,
			[&](CallTimer &tm, const QueryLayout &more) { return query_front(ctx, qa, qz, qor, ctx->tr_ws, tm, more); },
			opts, timer);
		const uint32_t R = d.R, n_al = d.n_al;
		const bool inversions = opts && (opts->flags & POVU_HIP_T_INVERSIONS);

		// ---- the reference steps
		std::vector<uint64_t> path_off((size_t)P + 1), ref_base((size_t)nR + 1, 0);
		HIP_CHECK(copy_async(path_off.data(), ctx->path_off, ((size_t)P + 1) * 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		for (uint32_t r = 0; r < nR; r++)
			ref_base[r + 1] = ref_base[r] + path_off[refs->ref_path[r] + 1] - path_off[refs->ref_path[r]];
		const uint64_t NR = ref_base[nR];
		const size_t n1 = (size_t)n + 1, hit_words = ((uint64_t)n * nR * 2 + 31) / 32 + 1,
			     pres_words = ((uint64_t)n_trees * nR + 31) / 32 + 1;
		const size_t scan32 = scan_tmp_bytes(std::max<size_t>({(size_t)g.V + 1, n1, 2 * (size_t)n + 1})) + 256;
		const size_t comp_a = compact_tmp_bytes((size_t)R + 1) + 256, sort_a = sort_tmp_bytes((size_t)R + 1) + 256;
		uint64_t *d_ref_base, *rlen64, *roff, *ilen, *atl, *s64;
		uint32_t *d_ref_path, *d_ref_of_path, *d_slot, *d_slot_first, *d_parent, *d_tree, *scnt, *soffv, *scur, *sval, *qv, *hit, *pres,
			*keep, *qidx, *words;
		uint8_t *d_fam, *callable, *called, *anchored, *rflag;
		uint32_t *rlist, *perm, *perm2, *key, *key2;
		uint64_t *pos;
		void *scan_tmp, *comp_tmp, *sort_tmp;
		carve(ctx->cl_ws, [&](Spans &take) {
			take((size_t)nR + 1, d_ref_base, d_ref_path);
			take((size_t)P + 1, d_ref_of_path, d_slot);
			take((size_t)NS + 1, d_slot_first);
			take(n1, d_parent, d_tree, d_fam, callable, called, anchored, keep, qidx);
			take(NR + 1, rlen64, roff);
			take((size_t)g.V + 1, scnt, soffv, scur);
			take(2 * n1, sval, qv);
			take(hit_words, hit);
			take(pres_words, pres);
			take((size_t)n_al + 1, ilen, atl);
			take((size_t)R + 1, rflag, rlist, perm, perm2, key, key2, pos);
			take(scan64_tmp(std::max<uint64_t>(NR + 1, 1)), s64);
			take(8, words);
			take(scan32, scan_tmp);
			take(comp_a, comp_tmp);
			take(sort_a, sort_tmp);
		});
		HIP_CHECK(copy_async(d_ref_base, ref_base.data(), ((size_t)nR + 1) * 8, hipMemcpyHostToDevice, s));
		HIP_CHECK(copy_async(d_ref_path, refs->ref_path, (size_t)nR * 4, hipMemcpyHostToDevice, s));
		if (P) {
			HIP_CHECK(copy_async(d_ref_of_path, ref_of_path.data(), (size_t)P * 4, hipMemcpyHostToDevice, s));
			HIP_CHECK(copy_async(d_slot, slot_of_path, (size_t)P * 4, hipMemcpyHostToDevice, s));
		}
		HIP_CHECK(copy_async(d_slot_first, slot_first.data(), ((size_t)NS + 1) * 4, hipMemcpyHostToDevice, s));
		if (n) {
			HIP_CHECK(copy_async(d_parent, sites->parent, (size_t)n * 4, hipMemcpyHostToDevice, s));
			HIP_CHECK(copy_async(d_tree, sites->tree, (size_t)n * 4, hipMemcpyHostToDevice, s));
			HIP_CHECK(copy_async(d_fam, sites->family, n, hipMemcpyHostToDevice, s));
		}
		HIP_CHECK(hipMemsetAsync(words, 0, 32, s));
		HIP_CHECK(hipMemsetAsync(scnt, 0, ((size_t)g.V + 1) * 4, s));
		HIP_CHECK(hipMemsetAsync(scur, 0, ((size_t)g.V + 1) * 4, s));
		HIP_CHECK(hipMemsetAsync(hit, 0, hit_words * 4, s));
		HIP_CHECK(hipMemsetAsync(pres, 0, pres_words * 4, s));

		// ---- reference offsets
		HIP_CHECK(hipMemsetAsync(rlen64 + NR, 0, 8, s));
		if (NR)
			KLAUNCH(k_cl_ref_len, dim3(cblk(NR)), dim3(C_TPB), 0, s, NR, d_ref_base, nR, d_ref_path, ctx->path_off, ctx->path_steps,
				ctx->seq_off, rlen64);
		scan64(rlen64, roff, NR + 1, s64, s);

		// ---- callability
		if (n) {
			KLAUNCH(k_cl_seg_count, dim3(cblk(n)), dim3(C_TPB), 0, s, n, d.q.qa, d.q.qz, g.vid, g.V, scnt, qv);
			scan_exclusive_u32(scnt, soffv, (size_t)g.V + 1, scan_tmp, scan32, s);
			KLAUNCH(k_cl_seg_fill, dim3(cblk(2 * (size_t)n)), dim3(C_TPB), 0, s, n, qv, soffv, scur, sval);
			if (NR)
				KLAUNCH(k_cl_hits, dim3(cblk(NR)), dim3(C_TPB), 0, s, NR, d_ref_base, nR, d_ref_path, ctx->path_off, ctx->path_steps,
					soffv, sval, hit);
			KLAUNCH(k_cl_present, dim3(cblk((size_t)n * nR)), dim3(C_TPB), 0, s, (uint64_t)n, nR, hit, d_tree, pres);
			KLAUNCH(k_cl_callable, dim3(cblk(n)), dim3(C_TPB), 0, s, n, nR, hit, pres, d_tree, d_parent, d_fam, callable, called);
			KLAUNCH(k_cl_unparent, dim3(cblk(n)), dim3(C_TPB), 0, s, n, callable, d_parent, called);
		}
		KLAUNCH(k_cl_keep, dim3(cblk(n1)), dim3(C_TPB), 0, s, n, called, d.aoff, keep, words + 1);
		scan_exclusive_u32(keep, qidx, n1, scan_tmp, scan32, s);
		uint32_t hw[2] = {0, 0};
		HIP_CHECK(copy_async(hw, qidx + n, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(hw + 1, words + 1, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		const uint32_t nQ = hw[0];
		if (hw[1] > MAX_ALLELES)
			throw HipError("a called site has " + std::to_string(hw[1]) + " alleles: more than 65534 in one record are refused");
		if (n_al) {
			KLAUNCH(k_cl_inner, dim3(cblk(n_al)), dim3(C_TPB), 0, s, n_al, d.afirst, d.rq, keep, d.rpos, d.rlen, ctx->path_steps,
				ctx->seq_off, g.vid, ilen, atl);
		}
		if (n)
			KLAUNCH(k_cl_anchored, dim3(cblk(n)), dim3(C_TPB), 0, s, n, keep, d.aoff, ilen, anchored);

		// ---- slot table and records
		uint32_t *smin, *smax;
		carve(ctx->cl_slot, [&](Spans &take) { take((size_t)nQ * S + 1, smin, smax); });
		HIP_CHECK(hipMemsetAsync(smin, 0xFF, ((size_t)nQ * S + 1) * 4, s));
		HIP_CHECK(hipMemsetAsync(smax, 0, ((size_t)nQ * S + 1) * 4, s));
		uint32_t nrec = 0;
		if (R && nQ) {
			KLAUNCH(k_cl_slots, dim3(cblk(R)), dim3(C_TPB), 0, s, R, d.rq, d.op, d.oa, keep, qidx, d_slot, S, smin, smax);
			KLAUNCH(k_cl_rec_flag, dim3(cblk(R)), dim3(C_TPB), 0, s, R, d.rq, d.op, keep, d_ref_of_path, rflag);
			compact_flagged_u8(rflag, R, rlist, words + 2, comp_tmp, comp_a, s);
			HIP_CHECK(copy_async(&nrec, words + 2, 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipStreamSynchronize(s));
		}
		check_call_32(nrec, "records");
		uint64_t ref_bases = 0;
		HIP_CHECK(copy_async(&ref_bases, roff + NR, 8, hipMemcpyDeviceToHost, s));
		const uint32_t nfl = nrec; // the flubble records; nrec: all records
		// the per-record arrays and the spelling's inputs (cl_rec)
		uint32_t *o_q, *o_path, *o_first, *o_ref, *o_nal, *o_an, *o_ns, *o_block, *o_nsteps, *need, *boff, *blist;
		uint64_t *o_pos, *nalt, *ac_off, *bcnt, *block_off;
		uint8_t *o_flags;
		uint16_t *gt;
		const size_t n2 = 2 * (size_t)n + 1;
		HIP_CHECK(hipStreamSynchronize(s));
		if (nfl) {
			KLAUNCH(k_cl_pos, dim3(cblk(nfl)), dim3(C_TPB), 0, s, nfl, rlist, d.rq, d.op, d.of, d_ref_of_path, d_ref_base, roff, anchored,
				pos, perm);
			uint32_t *cur = perm, *nxt = perm2;
			auto pass = [&](int which, unsigned bits) {
				KLAUNCH(k_cl_key, dim3(cblk(nfl)), dim3(C_TPB), 0, s, nfl, which, cur, rlist, d.op, d_ref_of_path, pos, key);
				sort_pairs_u32(key, key2, cur, nxt, nfl, bits, sort_tmp, sort_a, s);
				std::swap(cur, nxt);
			};
			pass(0, 32);
			if (ref_bases + 1 >= (1ull << 32))
				pass(1, 32);
			if (nR > 1)
				pass(2, bits_for(nR));
			perm = cur;
		}
		// ---- the inversion records, and every record's row in the one list
		InvIn iin;
		InvDevice iv;
		uint32_t *f_dst = nullptr;
		if (inversions) {
			iin.NR = NR, iin.nR = nR, iin.S = S, iin.NS = NS;
			iin.ref_base = d_ref_base, iin.ref_path = d_ref_path, iin.slot_of_path = d_slot, iin.slot_first = d_slot_first, iin.roff = roff;
			iin.max_steps = opts->max_steps ? opts->max_steps : 65536;
			iin.force_tier2 = (opts->flags & POVU_HIP_T_FORCE_TIER2) != 0;
			iv = inv_find(ctx, iin);
			check_call_32((uint64_t)nfl + iv.n, "records");
			if (iv.n) {
				uint32_t *f_ref;
				uint64_t *f_pos;
				carve(ctx->iv_rows, [&](Spans &take) { take((size_t)nfl + 1, f_ref, f_dst, f_pos); });
				if (nfl)
					KLAUNCH(k_cl_sorted_keys, dim3(cblk(nfl)), dim3(C_TPB), 0, s, nfl, perm, rlist, d.op, d_ref_of_path, pos, f_ref, f_pos);
				inv_merge(ctx, iv, nfl, f_ref, f_pos, f_dst);
				nrec = nfl + iv.n;
			}
		}
		const size_t r1 = (size_t)nrec + 1;
		carve(ctx->cl_rec, [&](Spans &take) {
			take(r1, o_q, o_path, o_first, o_ref, o_nal, o_an, o_ns, o_block, o_nsteps, o_pos, nalt, ac_off, o_flags);
			take((size_t)nrec * S + 1, gt);
			take(n2, need, boff, blist);
			take(n2 + iv.n, bcnt, block_off);
			take(scan64_tmp(std::max(r1, n2 + iv.n)), s64);
		});
		HIP_CHECK(hipMemsetAsync(o_nsteps, 0, r1 * 4, s));
		const InvRows rows{o_q, o_path, o_first, o_ref, o_nal, o_an, o_ns, o_block, o_nsteps, o_pos, nalt, o_flags, gt};
		HIP_CHECK(hipMemsetAsync(need, 0, n2 * 4, s));
		HIP_CHECK(hipMemsetAsync(nalt + nrec, 0, 8, s));
		if (nfl)
			KLAUNCH(k_cl_rec_fields, dim3(cblk(nfl)), dim3(C_TPB), 0, s, nfl, perm, rlist, pos, d.rq, d.op, d.of, d.oa, d.orv, d.aoff, o_q,
				o_path, o_first, o_ref, o_nal, o_pos, nalt, need, f_dst);
		inv_fields(ctx, iin, iv, rows);
		scan64(nalt, ac_off, r1, s64, s);
		uint64_t n_ac = 0;
		HIP_CHECK(copy_async(&n_ac, ac_off + nrec, 8, hipMemcpyDeviceToHost, s));
		scan_exclusive_u32(need, boff, n2, scan_tmp, scan32, s);
		uint32_t nb = 0;
		HIP_CHECK(copy_async(&nb, boff + 2 * (size_t)n, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		if (n)
			KLAUNCH(k_cl_blocks, dim3(cblk(2 * (size_t)n)), dim3(C_TPB), 0, s, 2 * (uint64_t)n, need, boff, blist);
		const uint32_t nfb = nb; // the flubble blocks; the inversion records' blocks follow them, one each: REF, then ALT
		check_call_32((uint64_t)nfb + iv.n, "blocks");
		nb = nfb + iv.n;
		HIP_CHECK(hipMemsetAsync(bcnt + nb, 0, 8, s));
		if (nfb)
			KLAUNCH(k_cl_block_cnt, dim3(cblk(nfb)), dim3(C_TPB), 0, s, nfb, blist, d.aoff, bcnt);
		inv_genotypes(ctx, iin, iv, rows, nfb, bcnt);
		scan64(bcnt, block_off, (size_t)nb + 1, s64, s);
		uint64_t nsp = 0, nfsp = 0; // spelled alleles: all, those of the flubble blocks
		HIP_CHECK(copy_async(&nsp, block_off + nb, 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(&nfsp, block_off + nfb, 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));

		// ---- spelling: lengths, offsets, bytes
		uint32_t *ac;
		uint64_t *slen, *alen, *sp_off, *at_off, *s64b;
		unsigned long long *bad;
		carve(ctx->cl_spell, [&](Spans &take) {
			take(n_ac + 1, ac);
			take(nsp + 1, slen, alen, sp_off, at_off);
			take(scan64_tmp(nsp + 1), s64b);
			take(1, bad);
		});
		HIP_CHECK(hipMemsetAsync(ac, 0, (n_ac + 1) * 4, s));
		HIP_CHECK(hipMemsetAsync(bad, 0xFF, 8, s));
		if (nfl) {
			const unsigned wg = wblk(nfl);
			KLAUNCH(k_cl_records, dim3(wg), dim3(C_TPB), 0, s, nfl, o_q, o_path, o_ref, qidx, d_slot, d_slot_first, NS, S, smin, smax, ac_off,
				d.qstatus, anchored, d.aoff, ilen, gt, ac, o_an, o_ns, o_flags, f_dst);
			KLAUNCH(k_cl_rec_block, dim3(cblk(nfl)), dim3(C_TPB), 0, s, nfl, perm, rlist, d.rq, d.orv, boff, o_block, f_dst);
		}
		inv_counts(ctx, iin, iv, rows, ac_off, ac);
		HIP_CHECK(hipMemsetAsync(slen + nsp, 0, 8, s));
		HIP_CHECK(hipMemsetAsync(alen + nsp, 0, 8, s));
		if (nfsp)
			KLAUNCH(k_cl_spell_len, dim3(cblk(nfsp)), dim3(C_TPB), 0, s, nfsp, nfb, block_off, blist, d.aoff, d.afirst, d.rpos, d.rlen,
				ctx->path_steps, ctx->seq_off, g.vid, ilen, atl, anchored, slen, alen);
		inv_spell_len(ctx, iin, iv, slen + nfsp, alen + nfsp);
		scan64(slen, sp_off, nsp + 1, s64b, s);
		scan64(alen, at_off, nsp + 1, s64b, s);
		uint64_t nbytes[2] = {0, 0};
		HIP_CHECK(copy_async(nbytes, sp_off + nsp, 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(copy_async(nbytes + 1, at_off + nsp, 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		char *o_seq, *o_at;
		carve(ctx->cl_bytes, [&](Spans &take) { take(nbytes[0] + 1, o_seq), take(nbytes[1] + 1, o_at); });
		if (nfsp)
			KLAUNCH(k_cl_emit, dim3(wblk(nfsp)), dim3(C_TPB), 0, s, nfsp, nfb, block_off, blist, d.aoff, d.afirst, d.rpos, d.rlen,
				ctx->path_steps, ctx->seq_off, ctx->seq, g.vid, anchored, sp_off, at_off, o_seq, o_at, bad);
		inv_emit(ctx, iin, iv, sp_off + nfsp, at_off + nfsp, o_seq, o_at, bad);
		uint64_t hbad = 0;
		HIP_CHECK(copy_async(&hbad, bad, 8, hipMemcpyDeviceToHost, s));
		std::vector<uint64_t> h_roff(nR ? nR + 1 : 1);
		for (uint32_t r = 0; r <= nR; r++)
			HIP_CHECK(copy_async(h_roff.data() + r, roff + ref_base[r], 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		if (hbad != ~0ull) {
			uint32_t id = 0;
			HIP_CHECK(copy_async(&id, g.vid + hbad, 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipStreamSynchronize(s));
			throw HipError("segment " + std::to_string(id) + " holds a byte that is no nucleotide code (ACGTN, lower case, IUPAC)");
		}

		// ---- to the host
		auto o = std::make_unique<CallsOwner>();
		hand_off(o->query, nrec, o_q, nrec, ctx);
		hand_off(o->path, nrec, o_path, nrec, ctx);
		hand_off(o->first, nrec, o_first, nrec, ctx);
		hand_off(o->ref_allele, nrec, o_ref, nrec, ctx);
		hand_off(o->n_alleles, nrec, o_nal, nrec, ctx);
		hand_off(o->an, nrec, o_an, nrec, ctx);
		hand_off(o->ns, nrec, o_ns, nrec, ctx);
		hand_off(o->block, nrec, o_block, nrec, ctx);
		hand_off(o->n_steps, nrec, o_nsteps, nrec, ctx);
		hand_off(o->pos, nrec, o_pos, nrec, ctx);
		hand_off(o->flags, nrec, o_flags, nrec, ctx);
		hand_off(o->ac_off, r1, ac_off, r1, ctx);
		hand_off(o->ac, n_ac, ac, n_ac, ctx);
		hand_off(o->gt, (size_t)nrec * S, gt, (size_t)nrec * S, ctx);
		hand_off(o->block_off, (size_t)nb + 1, block_off, (size_t)nb + 1, ctx);
		hand_off(o->seq_off, nsp + 1, sp_off, nsp + 1, ctx);
		hand_off(o->at_off, nsp + 1, at_off, nsp + 1, ctx);
		hand_off(o->seq, nbytes[0], o_seq, nbytes[0], ctx);
		hand_off(o->at, nbytes[1], o_at, nbytes[1], ctx);
		o->view.device_ms = timer.stop(s);
		o->contig_len.resize(nR);
		for (uint32_t r = 0; r < nR; r++)
			o->contig_len[r] = h_roff[r + 1] - h_roff[r];
		povu_hip_calls &v = o->view;
		v.n_records = nrec;
		v.n_slots = S;
		v.n_blocks = nb;
		v.n_spelled = nsp;
		v.n_seq_bytes = nbytes[0];
		v.n_at_bytes = nbytes[1];
		v.n_refs = nR;
		v.n_steps = o->n_steps.data();
		v.n_inv_records = iv.n, v.n_inv_heads = iv.n_heads, v.n_inv_long = iv.n_long, v.n_inv_tier2 = iv.n_tier2;
		v.query = o->query.data(), v.path = o->path.data(), v.first = o->first.data(), v.ref_allele = o->ref_allele.data();
		v.n_alleles = o->n_alleles.data(), v.an = o->an.data(), v.ns = o->ns.data(), v.block = o->block.data();
		v.pos = o->pos.data(), v.flags = o->flags.data(), v.ac_off = o->ac_off.data(), v.ac = o->ac.data(), v.gt = o->gt.data();
		v.block_off = o->block_off.data(), v.seq_off = o->seq_off.data(), v.at_off = o->at_off.data(), v.seq = o->seq.data();
		v.at = o->at.data(), v.contig_len = o->contig_len.data();
		CallsOwner *raw = o.release();
		return &raw->view;
	});
}

extern "C" void povu_hip_calls_free(povu_hip_calls *c)
{
	delete reinterpret_cast<CallsOwner *>(c);
}
