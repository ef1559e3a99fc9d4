// nest_kernels.hip -- the nested calls of povu_hip_call with POVU_HIP_T_NESTED (include/povu_hip.h).
//
// The definition is this project's own ("Nested calls"; restated in tests/nested_ref.py).  Nesting is the
// nesting of traversals along a path, not PVST parentage: traversal t encloses t' of another called site when t' lies within
// t on the same path and is shorter.  Two steps of povu_hip_call:
//   classes  (between callability and the slot table)
//     index     the traversals of the called sites, compacted and radix-sorted by their global path position (which names
//               the path too); an entry holds its first and last position, its site and its traversal;
//     cover     per exact allele of a called site of two alleles or more, from its first traversal t: position k of t is
//               covered when the running maximum of the last positions of the enclosed entries that start before k exceeds
//               k.  The entries that start inside t are one stretch of the index.  Tier 1: a lane per allele of up to 64
//               steps walks steps and entries in one merge.  Tier 2: a wave per longer allele, 64 positions a round -- the
//               round's entries drop their ends into the slot of their start (LDS), a wave prefix maximum over the slots
//               and the carry of the rounds before give every lane its maximum.  The mask is kept a byte a step, S -> Z;
//     skeleton  the 64-bit hash (sum of mix(rank, step) over the uncovered steps, S -> Z) and the length of what is left;
//     classes   the exact alleles grouped by (site, length, hash) and compared skeleton by skeleton (exact_groups.hpp, the
//               machinery of the traversals' alleles); a class is numbered by the scan of the "lowest allele of its group"
//               flags, so classes come in the order of their lowest allele.
//   records  (once the flubble records are known, before they are sorted and before any block is formed)
//     parent    a wave per record walks the entries that start inside its traversal and offers itself, as (length, record),
//               to every enclosed entry that is a record too (atomic minimum: the shortest encloser, then the lowest site);
//     level     a lane per record climbs its chain of parents: the top's PVST height - 1 plus the links climbed;
//     profile   big from the written lengths, reach by climbing while the level is above max_level, the kept records
//               compacted -- what is dropped here is never spelled;
//     span      with POVU_HIP_T_SPANNING ("Spanning alleles") a wave per record: the rows of its ancestors' sites in the (site,
//               slot) table, 64 ancestors a round in the lanes' registers, then the slots 64 a round -- a lane whose slot is
//               empty at the record's site looks for an ancestor row where it is not; a ballot per slot round is the word of
//               the record's spanned entries.
// Work: an entry is visited once per called traversal that encloses (or overlaps) it -- path steps times nesting depth, the
// bound of the scans themselves.
#include "nest_kernels.hpp"

#include "exact_groups.hpp"

namespace povu_hip
{

static constexpr uint32_t N1_STEPS = 64; // steps of the longest allele tier 1 covers

// ---- index
__global__ void k_ns_called_flag(uint32_t R, const uint32_t *__restrict__ rq, const uint8_t *__restrict__ called, uint8_t *__restrict__ flag)
{
	for (uint32_t t = blockIdx.x * Q_TPB + threadIdx.x; t < R; t += gridDim.x * Q_TPB)
		flag[t] = called[rq[t]];
}
__global__ void k_ns_pos_key(uint32_t ni, int which, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ rpos, uint32_t *__restrict__ key)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < ni; k += gridDim.x * Q_TPB) {
		const uint64_t p = trav_first_pos(rpos, perm[k]);
		key[k] = which ? (uint32_t)(p >> 32) : (uint32_t)p;
	}
}
__global__ void k_ns_index(uint32_t ni, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ rpos, const uint32_t *__restrict__ rlen,
			   const uint32_t *__restrict__ rq, uint64_t *__restrict__ ipos, uint64_t *__restrict__ iend, uint32_t *__restrict__ iq,
			   uint32_t *__restrict__ it)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < ni; k += gridDim.x * Q_TPB) {
		const uint32_t t = perm[k];
		const TravSpan sp = trav_span(rpos, rlen, t);
		ipos[k] = sp.first_pos();
		iend[k] = sp.last_pos();
		iq[k] = rq[t];
		it[k] = t;
	}
}

// the index of the flagged traversals: compacted, radix-sorted by global position
void nest_index(povu_hip_ctx *ctx, const TravDevice &d, const uint8_t *flag, NestIndex &ix, const NestIndexWs &w)
{
	hipStream_t s = ctx->stream;
	const uint32_t R = d.R;
	ix.ni = 0;
	if (R) {
		compact_flagged_u8(flag, R, w.ilist, w.count, w.tmp, w.tmp_bytes, s);
		ix.ni = read_back(w.count, s);
	}
	const uint32_t ni = ix.ni;
	if (!ni)
		return;
	LsdSort sort{w.ilist, w.pb, w.key, w.kout, ni, w.tmp, w.tmp_bytes, s};
	auto write_key = [&](int which, const uint32_t *perm, uint32_t *k) {
		KLAUNCH(k_ns_pos_key, dim3(stride_blocks(ni)), dim3(Q_TPB), 0, s, ni, which, perm, d.rpos, k);
	};
	sort.pass(0, (unsigned)std::min<uint64_t>(32, bits_for(ctx->n_path_steps)), write_key);
	if (ctx->n_path_steps >= (1ull << 32))
		sort.pass(1, 32, write_key);
	KLAUNCH(k_ns_index, dim3(stride_blocks(ni)), dim3(Q_TPB), 0, s, ni, sort.cur, d.rpos, d.rlen, d.rq, ix.ipos, ix.iend, ix.iq, ix.it);
}

// ---- cover and skeleton
// site of every exact allele; candidates: the alleles of called sites of two alleles or more
__global__ void k_ns_allele_site(uint32_t n_al, const uint32_t *__restrict__ afirst, const uint32_t *__restrict__ rq,
				 const uint32_t *__restrict__ aoff, const uint8_t *__restrict__ called, uint32_t *__restrict__ aq,
				 uint8_t *__restrict__ cand)
{
	for (uint32_t a = blockIdx.x * Q_TPB + threadIdx.x; a < n_al; a += gridDim.x * Q_TPB) {
		const uint32_t q = rq[afirst[a]];
		aq[a] = q;
		cand[a] = called[q] && aoff[q + 1] - aoff[q] >= 2;
	}
}

struct CoverArgs {
	const uint32_t *steps;
	const uint64_t *rpos;
	const uint32_t *rlen, *rq, *afirst, *soff;
	const uint8_t *cand;
	const uint64_t *ipos, *iend;
	const uint32_t *iq;
	uint32_t ni;
	uint8_t *cov;	// [allele steps] 1: covered, S -> Z
	uint32_t *slen; // skeleton length
	uint64_t *shash;
	uint32_t mask_hi, mask_lo;
};
__device__ __forceinline__ uint64_t kept_bits(const CoverArgs &A, uint64_t h) { return h & (((uint64_t)A.mask_hi << 32) | A.mask_lo); }
// entry e is enclosed by the traversal of site q over [.., end] of len steps (it starts at or after the traversal's start)
__device__ __forceinline__ bool enclosed(const CoverArgs &A, uint32_t e, uint32_t q, uint64_t end, uint32_t len)
{
	const uint64_t ie = A.iend[e];
	return A.iq[e] != q && ie <= end && ie - A.ipos[e] < (uint64_t)len - 1;
}

// tier 1: a lane per allele; longer alleles (all candidates with force2) are handed over.  An allele that is no candidate
// gets a skeleton of its own (length 0, hash = its number): it stays a class of its own.
__global__ __launch_bounds__(Q_TPB) void k_ns_cover_t1(uint32_t n_al, CoverArgs A, uint32_t force2, uint8_t *__restrict__ hand)
{
	const uint32_t a = blockIdx.x * Q_TPB + threadIdx.x;
	if (a >= n_al)
		return;
	hand[a] = 0;
	if (!A.cand[a]) {
		A.slen[a] = 0;
		A.shash[a] = kept_bits(A, a);
		return;
	}
	const uint32_t t = A.afirst[a];
	const TravSpan sp = trav_span(A.rpos, A.rlen, t);
	if (force2 || sp.len > N1_STEPS) {
		hand[a] = 1;
		return;
	}
	const uint64_t pos = sp.first_pos(), end = sp.last_pos();
	const uint32_t q = A.rq[t], base = A.soff[a];
	uint32_t e = lower_bound(A.ipos, 0u, A.ni, pos), m = 0;
	uint64_t top = 0; // the running maximum of the enclosed entries' last positions (every one is at least 1)
	for (uint64_t k = pos; k <= end; k++) {
		for (; e < A.ni && A.ipos[e] < k; e++)
			if (enclosed(A, e, q, end, sp.len))
				top = max(top, A.iend[e]);
		const bool c = top > k;
		A.cov[base + (uint32_t)(sp.rev ? end - k : k - pos)] = c;
		m += !c;
	}
	uint64_t h = 0;
	uint32_t j = 0;
	for (uint32_t i = 0; i < sp.len; i++)
		if (!A.cov[base + i]) // (this lane's own stores)
			h += step_hash(j++, sp.step(A.steps, i));
	A.slen[a] = m;
	A.shash[a] = kept_bits(A, h);
}

// tier 2: a wave (a workgroup of 64 lanes: its barriers are the wave's own) per allele of `list`, 64 positions a round
__global__ __launch_bounds__(64) void k_ns_cover_t2(const uint32_t *__restrict__ list, uint32_t n2, CoverArgs A)
{
	__shared__ uint32_t slot[64];
	const uint32_t lane = threadIdx.x;
	for (uint32_t w = blockIdx.x; w < n2; w += gridDim.x) {
		const uint32_t a = list[w], t = A.afirst[a], q = A.rq[t], base = A.soff[a];
		const TravSpan sp = trav_span(A.rpos, A.rlen, t);
		const uint64_t pos = sp.first_pos(), end = sp.last_pos();
		uint32_t e = lower_bound(A.ipos, 0u, A.ni, pos), carry = 0; // ends relative to pos: at least 1
		for (uint32_t cb = 0; cb < sp.len; cb += 64) {
			// the entries that start at the round's positions: their ends into the slot of their start
			const uint32_t e_hi = lower_bound(A.ipos, 0u, A.ni, pos + cb + 64);
			slot[lane] = 0;
			__syncthreads();
			for (uint32_t x = e + lane; x < e_hi; x += 64)
				if (enclosed(A, x, q, end, sp.len) && A.ipos[x] - pos - cb < 64)
					atomicMax(&slot[(uint32_t)(A.ipos[x] - pos) - cb], (uint32_t)(A.iend[x] - pos));
			__syncthreads();
			const uint32_t incl = wave_inclusive_max(slot[lane]);
			uint32_t before = __shfl_up(incl, 1, 64); // the entries that start before this lane's position
			if (lane == 0)
				before = 0;
			const uint32_t k = cb + lane;
			if (k < sp.len)
				A.cov[base + (sp.rev ? sp.len - 1 - k : k)] = max(carry, before) > k;
			carry = max(carry, __shfl(incl, 63, 64));
			e = e_hi;
			__syncthreads();
		}
	}
}
__global__ __launch_bounds__(64) void k_ns_skel_t2(const uint32_t *__restrict__ list, uint32_t n2, CoverArgs A)
{
	const uint32_t lane = threadIdx.x;
	const unsigned long long below = (1ull << lane) - 1ull;
	for (uint32_t w = blockIdx.x; w < n2; w += gridDim.x) {
		const uint32_t a = list[w], base = A.soff[a];
		const TravSpan sp = trav_span(A.rpos, A.rlen, A.afirst[a]);
		uint32_t m = 0;
		uint64_t h = 0;
		for (uint32_t cb = 0; cb < sp.len; cb += 64) {
			const uint32_t i = cb + lane;
			const bool open = i < sp.len && !A.cov[base + i];
			const unsigned long long mask = __ballot(open);
			if (open)
				h += step_hash(m + (uint32_t)__popcll(mask & below), sp.step(A.steps, i));
			m += (uint32_t)__popcll(mask);
		}
		h = wave_sum(h);
		if (lane == 0) {
			A.slen[a] = m;
			A.shash[a] = kept_bits(A, h);
		}
	}
}

// exact alleles a and b (of one site) have the same skeleton
struct SameSkeleton {
	const uint32_t *steps;
	const uint64_t *rpos;
	const uint32_t *rlen, *afirst, *soff;
	const uint8_t *cand, *cov;
	__device__ __forceinline__ bool operator()(uint32_t a, uint32_t b) const
	{
		if (!cand[a])
			return false; // (two alleles of a site that is no candidate: classes of their own)
		const TravSpan sa = trav_span(rpos, rlen, afirst[a]), sb = trav_span(rpos, rlen, afirst[b]);
		const uint32_t la = sa.len, lb = sb.len, ba = soff[a], bb = soff[b];
		for (uint32_t i = 0, j = 0;; i++, j++) {
			while (i < la && cov[ba + i])
				i++;
			while (j < lb && cov[bb + j])
				j++;
			if (i == la || j == lb)
				return i == la && j == lb;
			if (sa.step(steps, i) != sb.step(steps, j))
				return false;
		}
	}
};

// ---- classes
// class of every allele (global numbering) and, from the group's first allele, the class's representative
__global__ void k_ns_class_of(uint32_t n_al, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ rep, const uint32_t *__restrict__ cidx,
			      const uint32_t *__restrict__ afirst, uint32_t *__restrict__ cglob, uint32_t *__restrict__ crep,
			      uint32_t *__restrict__ cfirst)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < n_al; k += gridDim.x * Q_TPB) {
		const uint32_t a = perm[k], c = cidx[perm[rep[k]]];
		cglob[a] = c;
		if (rep[k] == k) {
			crep[c] = a;
			cfirst[c] = afirst[a];
		}
	}
}
__global__ void k_ns_class_off(uint32_t n, const uint32_t *__restrict__ aoff, const uint32_t *__restrict__ cidx, uint32_t *__restrict__ coff)
{
	for (uint32_t q = blockIdx.x * Q_TPB + threadIdx.x; q <= n; q += gridDim.x * Q_TPB)
		coff[q] = cidx[aoff[q]];
}
__global__ void k_ns_trav_class(uint32_t R, const uint32_t *__restrict__ rq, const uint32_t *__restrict__ oa, const uint32_t *__restrict__ aoff,
				const uint32_t *__restrict__ cglob, const uint32_t *__restrict__ coff, uint32_t *__restrict__ oc)
{
	for (uint32_t t = blockIdx.x * Q_TPB + threadIdx.x; t < R; t += gridDim.x * Q_TPB) {
		const uint32_t q = rq[t];
		oc[t] = cglob[aoff[q] + oa[t]] - coff[q];
	}
}

NestClasses nest_classes(povu_hip_ctx *ctx, const TravDevice &d, const uint8_t *called, uint32_t max_steps, bool force_tier2)
{
	hipStream_t s = ctx->stream;
	const uint32_t n = d.q.n, R = d.R, n_al = d.n_al, hbits = hash_bits_hook();
	const size_t R1 = (size_t)R + 1, A1 = (size_t)n_al + 1, n1 = (size_t)n + 1;
	NestClasses c;
	NestIndex &ix = c.ix;
	uint8_t *flag, *cov, *cand, *hand, *rbad;
	uint32_t *ilist, *pb, *key, *kout, *words, *slen, *aq, *list2, *ga, *gb, *gkey, *gkout, *mark, *hmax, *head, *rep, *blist, *firstf, *cidx, *cglob;
	uint64_t *shash;
	unsigned long long *tot;
	void *tmp;
	const size_t tmp_bytes = prim_tmp_bytes(std::max({R1, A1, n1}), true) + 256;
	carve(ctx->ns_idx, [&](Spans &take) { take(R1, ix.ipos, ix.iend, ix.iq, ix.it); });
	carve(ctx->ns_cls, [&](Spans &take) {
		take(n1, c.coff);
		take(A1, c.crep, c.cfirst);
		take(R1, c.oc);
	});
	carve(ctx->ns_ws, [&](Spans &take) {
		take(R1, flag, ilist, pb, key, kout);
		take(d.n_steps + 1, cov);
		take(A1, shash, slen, aq, list2, ga, gb, gkey, gkout, mark, hmax, head, rep, blist, firstf, cidx, cglob, cand, hand, rbad);
		take(8, words);
		take(2, tot);
		take(tmp_bytes, tmp);
	});
	HIP_CHECK(hipMemsetAsync(words, 0, 32, s));
	// ---- index
	if (R)
		KLAUNCH(k_ns_called_flag, dim3(stride_blocks(R)), dim3(Q_TPB), 0, s, R, d.rq, called, flag);
	nest_index(ctx, d, flag, ix, NestIndexWs{ilist, pb, key, kout, words, tmp, tmp_bytes});
	const uint32_t ni = ix.ni;
	if (!n_al) {
		HIP_CHECK(hipMemsetAsync(c.coff, 0, n1 * 4, s));
		return c;
	}
	// ---- cover, skeleton
	KLAUNCH(k_ns_allele_site, dim3(stride_blocks(n_al)), dim3(Q_TPB), 0, s, n_al, d.afirst, d.rq, d.aoff, called, aq, cand);
	HIP_CHECK(hipMemsetAsync(cov, 0, d.n_steps + 1, s));
	const CoverArgs CA{ctx->path_steps, d.rpos, d.rlen, d.rq, d.afirst, d.soff, cand, ix.ipos, ix.iend, ix.iq, ni,
			   cov, slen, shash, hash_mask_hi(hbits), hash_mask_lo(hbits)};
	KLAUNCH(k_ns_cover_t1, dim3(lane_blocks(n_al)), dim3(Q_TPB), 0, s, n_al, CA, force_tier2 ? 1u : 0u, hand);
	compact_flagged_u8(hand, n_al, list2, words + 1, tmp, tmp_bytes, s);
	c.n_tier2 = read_back(words + 1, s);
	if (c.n_tier2) {
		const unsigned wg = (unsigned)std::min<uint32_t>(c.n_tier2, 1u << 16);
		KLAUNCH(k_ns_cover_t2, dim3(wg), dim3(64), 0, s, list2, c.n_tier2, CA);
		KLAUNCH(k_ns_skel_t2, dim3(wg), dim3(64), 0, s, list2, c.n_tier2, CA);
	}
	// ---- classes
	GroupWs gw{ga, gb, gkey, gkout, mark, hmax, head, rep, blist, rbad, tmp, tmp_bytes};
	const uint32_t *sp = group_exact(n_al, aq, slen, shash, hbits, bits_for(max_steps), bits_for(n), SameSkeleton{ctx->path_steps, d.rpos, d.rlen, d.afirst, d.soff, cand, cov},
					 gw, words + 2, tot, &c.n_splits, s);
	number_groups(n_al, sp, rep, firstf, cidx, nullptr, tmp, tmp_bytes, s);
	c.n_cl = read_back(cidx + n_al, s);
	KLAUNCH(k_ns_class_of, dim3(stride_blocks(n_al)), dim3(Q_TPB), 0, s, n_al, sp, rep, cidx, d.afirst, cglob, c.crep, c.cfirst);
	KLAUNCH(k_ns_class_off, dim3(stride_blocks(n1)), dim3(Q_TPB), 0, s, n, d.aoff, cidx, c.coff);
	if (R)
		KLAUNCH(k_ns_trav_class, dim3(stride_blocks(R)), dim3(Q_TPB), 0, s, R, d.rq, d.oa, d.aoff, cglob, c.coff, c.oc);
	return c;
}

// ---- records: parent, level, profile
__global__ void k_ns_rec_of(uint32_t nfl, const uint32_t *__restrict__ rlist, uint32_t *__restrict__ rec_of)
{
	for (uint32_t j = blockIdx.x * Q_TPB + threadIdx.x; j < nfl; j += gridDim.x * Q_TPB)
		rec_of[rlist[j]] = j;
}
// a wave per record: the record offers itself to every record it encloses (par: the minimum of (steps - 1) << 32 | record)
__global__ __launch_bounds__(Q_TPB) void k_ns_parent(uint32_t nfl, const uint32_t *__restrict__ rlist, const uint32_t *__restrict__ rq,
						     const uint64_t *__restrict__ rpos, const uint32_t *__restrict__ rlen, NestIndex ix,
						     const uint32_t *__restrict__ rec_of, unsigned long long *__restrict__ par)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	for (uint32_t j = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); j < nfl; j += waves) {
		const uint32_t t = rlist[j], q = rq[t];
		const TravSpan sp = trav_span(rpos, rlen, t);
		const uint64_t pos = sp.first_pos(), end = sp.last_pos();
		const uint32_t lo = lower_bound(ix.ipos, 0u, ix.ni, pos), hi = lower_bound(ix.ipos, 0u, ix.ni, end + 1);
		for (uint32_t x = lo + lane; x < hi; x += 64) {
			const uint64_t ie = ix.iend[x];
			if (ix.iq[x] == q || ie > end || ie - ix.ipos[x] >= (uint64_t)sp.len - 1)
				continue;
			const uint32_t jj = rec_of[ix.it[x]];
			if (jj != NO_QUERY)
				atomicMin(par + jj, ((unsigned long long)(sp.len - 1) << 32) | j);
		}
	}
}
// a lane per record climbs its chain: level, the parent's site; cnt[0] += the records with a parent
__global__ __launch_bounds__(Q_TPB) void k_ns_level(uint32_t nfl, const uint32_t *__restrict__ rlist, const uint32_t *__restrict__ rq,
						    const uint32_t *__restrict__ height, const unsigned long long *__restrict__ par,
						    uint32_t *__restrict__ level, uint32_t *__restrict__ parent_q, unsigned long long *__restrict__ cnt)
{
	for (uint32_t j0 = blockIdx.x * Q_TPB; j0 < nfl; j0 += gridDim.x * Q_TPB) {
		const uint32_t j = j0 + threadIdx.x;
		uint32_t has = 0;
		if (j < nfl) {
			uint32_t cur = j, up = 0;
			for (uint32_t k = 0; k < nfl && par[cur] != ~0ull; k++, up++)
				cur = (uint32_t)par[cur];
			level[j] = height[rq[rlist[cur]]] - 1 + up;
			has = par[j] != ~0ull;
			parent_q[j] = has ? rq[rlist[(uint32_t)par[j]]] : NO_QUERY;
		}
		has = wave_sum(has);
		if ((threadIdx.x & 63u) == 0 && has)
			atomicAdd(cnt, (unsigned long long)has);
	}
}
// the profile's choice: keep[j], rescued[j]; cnt[1] += popped, cnt[2] += rescued
__global__ __launch_bounds__(Q_TPB) void k_ns_profile(uint32_t nfl, uint32_t profile, uint32_t max_level, uint64_t max_ref, uint64_t max_al,
						      const uint64_t *__restrict__ ref_len, const uint64_t *__restrict__ max_len,
						      const unsigned long long *__restrict__ par, const uint32_t *__restrict__ level,
						      uint8_t *__restrict__ keep, uint8_t *__restrict__ rescued, unsigned long long *__restrict__ cnt)
{
	auto big = [&](uint32_t r) { return (max_ref && ref_len[r] > max_ref) || (max_al && max_len[r] > max_al); };
	for (uint32_t j0 = blockIdx.x * Q_TPB; j0 < nfl; j0 += gridDim.x * Q_TPB) {
		const uint32_t j = j0 + threadIdx.x;
		uint32_t popped = 0, saved = 0;
		if (j < nfl) {
			bool k = false, r = false;
			if (profile == POVU_HIP_PROFILE_TOP_LEVEL_ONLY) {
				k = level[j] == 0;
			} else {
				// reach: the level is within max_level, or the parent is big and reached itself
				bool reach = true;
				uint32_t cur = j;
				for (uint32_t it = 0; it < nfl && (int32_t)level[cur] > (int32_t)max_level; it++) {
					if (par[cur] == ~0ull || !big((uint32_t)par[cur])) {
						reach = false;
						break;
					}
					cur = (uint32_t)par[cur];
				}
				const bool b = big(j);
				k = reach && !b;
				r = k && (int32_t)level[j] > (int32_t)max_level;
				popped = reach && b;
				saved = r;
			}
			keep[j] = k;
			rescued[j] = r;
		}
		popped = wave_sum(popped);
		saved = wave_sum(saved);
		if ((threadIdx.x & 63u) == 0) {
			if (popped)
				atomicAdd(cnt + 1, (unsigned long long)popped);
			if (saved)
				atomicAdd(cnt + 2, (unsigned long long)saved);
		}
	}
}

// the spanned entries: a wave per record j.  The chain of parents is walked by the whole wave (every lane reads the same
// par[]), lane k keeps the table row of ancestor k of the round; a lane climbs nothing on its own.  The first round (the 64
// nearest ancestors) is walked once and stays in the registers over all slot rounds; a chain longer than that is walked on
// from ancestor 64 only while some lane of the slot round still looks.  bits[j * W + w]: the ballot of slot round w; star[j];
// cnt[3] += records with a spanned entry, cnt[4] += spanned entries, both of the records that are written (keep, pass).  The
// grid is capped (SPAN_BLOCKS): a wave strides over its records and adds what it counted once, so the two counters see
// thousands of atomics on one address, not two a record
static constexpr unsigned SPAN_BLOCKS = 4096; // (the device's wave slots at Q_TPB lanes a workgroup, twice over)
__global__ __launch_bounds__(Q_TPB) void k_ns_span(uint32_t nfl, const uint32_t *__restrict__ rlist, const uint32_t *__restrict__ rq,
						   const uint32_t *__restrict__ op, const uint32_t *__restrict__ qstatus,
						   const unsigned long long *__restrict__ par, NestSpan A, uint32_t W, const uint8_t *__restrict__ keep,
						   unsigned long long *__restrict__ bits, uint8_t *__restrict__ star, unsigned long long *__restrict__ cnt)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64), S = A.S;
	unsigned long long n_records = 0, n_entries = 0; // of the wave's records that are written: one atomic each at its end
	for (uint32_t j = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); j < nfl; j += waves) {
		const uint32_t t = rlist[j], q = rq[t], own = A.slot_of_path[op[t]];
		const uint64_t base = (uint64_t)A.qidx[q] * S;
		const uint8_t status = qstatus[q] ? 1 : 0; // (any bit: the search was cut short)
		uint32_t row0 = 0, n0 = 0, cur = j;
		for (; n0 < SPAN_ROUND && par[cur] != ~0ull; n0++) {
			cur = (uint32_t)par[cur];
			if (lane == n0)
				row0 = A.qidx[rq[rlist[cur]]];
		}
		const uint32_t cur64 = cur;
		uint32_t n_star = 0;
		for (uint32_t w = 0; w < W; w++) {
			const uint32_t sl = w * 64 + lane;
			const bool need = n0 && sl < S && span_candidate(span_slot_empty(A.smin[base + sl]), status, sl == own);
			bool hit = false;
			uint32_t row = row0, n = n0, at = cur64;
			for (;;) {
				for (uint32_t k = 0; k < n && __ballot(need && !hit); k++) {
					const uint32_t r = __shfl(row, (int)k, 64);
					if (need && !hit)
						hit = !span_slot_empty(A.smin[(uint64_t)r * S + sl]);
				}
				if (n < SPAN_ROUND || !__ballot(need && !hit) || par[at] == ~0ull)
					break;
				for (n = 0; n < SPAN_ROUND && par[at] != ~0ull; n++) {
					at = (uint32_t)par[at];
					if (lane == n)
						row = A.qidx[rq[rlist[at]]];
				}
			}
			const unsigned long long mask = __ballot(hit);
			if (lane == 0)
				bits[(uint64_t)j * W + w] = mask;
			n_star += (uint32_t)__popcll(mask);
		}
		if (lane == 0) {
			star[j] = n_star != 0;
			if (n_star && (!keep || keep[j]) && (!A.pass || A.pass[q])) {
				n_records++;
				n_entries += n_star;
			}
		}
	}
	if (lane == 0 && n_records) {
		atomicAdd(cnt + 3, n_records);
		atomicAdd(cnt + 4, n_entries);
	}
}

NestRecs nest_records(povu_hip_ctx *ctx, const CallView &v, const NestIndex &ix, const povu_hip_call_profile_opts &limits, const NestSpan &span)
{
	hipStream_t s = ctx->stream;
	const uint32_t nfl = v.nfl;
	const TravView &d = v.trav;
	const size_t F1 = (size_t)nfl + 1, R1 = (size_t)d.R + 1;
	NestRecs o;
	unsigned long long *par, *cnt;
	uint32_t *rec_of, *words;
	uint8_t *keep;
	void *tmp;
	const size_t tmp_bytes = prim_tmp_bytes(F1, false) + 256;
	constexpr size_t N_CNT = 6; // enclosed, popped, rescued, records with a `*`, spanned entries; one spare
	const uint32_t W = span.on ? (span.S + 63) / 64 : 0;
	carve(ctx->ns_rec, [&](Spans &take) {
		take(F1, par, o.level, o.parent_q, o.kept, keep, o.rescued);
		take(R1, rec_of);
		take(N_CNT, cnt);
		take(2, words);
		take(tmp_bytes, tmp);
		if (span.on) { // (without the option the arena is laid out as before)
			take((size_t)nfl * W + 1, o.span_bits);
			take(F1, o.star);
		}
	});
	o.span_words = W;
	o.n_kept = nfl;
	HIP_CHECK(hipMemsetAsync(o.rescued, 0, F1, s));
	if (!nfl)
		return o;
	HIP_CHECK(hipMemsetAsync(par, 0xFF, F1 * 8, s));
	HIP_CHECK(hipMemsetAsync(rec_of, 0xFF, R1 * 4, s));
	HIP_CHECK(hipMemsetAsync(cnt, 0, N_CNT * 8, s));
	KLAUNCH(k_ns_rec_of, dim3(stride_blocks(nfl)), dim3(Q_TPB), 0, s, nfl, v.rlist, rec_of);
	KLAUNCH(k_ns_parent, dim3(wave_blocks(nfl)), dim3(Q_TPB), 0, s, nfl, v.rlist, d.rq, d.rpos, d.rlen, ix, rec_of, par);
	KLAUNCH(k_ns_level, dim3(stride_blocks(nfl)), dim3(Q_TPB), 0, s, nfl, v.rlist, d.rq, v.height, par, o.level, o.parent_q, cnt);
	const bool filter = limits.profile != POVU_HIP_PROFILE_RAW_GRAPH;
	if (filter) {
		KLAUNCH(k_ns_profile, dim3(stride_blocks(nfl)), dim3(Q_TPB), 0, s, nfl, limits.profile, limits.max_level, limits.max_ref_length,
			limits.max_allele_length, v.ref_len, v.max_len, par, o.level, keep, o.rescued, cnt);
		compact_flagged_u8(keep, nfl, o.kept, words, tmp, tmp_bytes, s);
		HIP_CHECK(copy_async(&o.n_kept, words, 4, hipMemcpyDeviceToHost, s));
	} else {
		launch_iota(nfl, o.kept, s);
	}
	if (span.on) // (after the profile: the counters are those of the kept records)
		KLAUNCH(k_ns_span, dim3(std::min(wave_blocks(nfl), SPAN_BLOCKS)), dim3(Q_TPB), 0, s, nfl, v.rlist, d.rq, d.op, d.qstatus, par, span, W, filter ? keep : nullptr,
			o.span_bits, o.star, cnt);
	unsigned long long h[N_CNT] = {};
	HIP_CHECK(copy_async(h, cnt, N_CNT * 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	o.n_enclosed = h[0], o.n_popped = h[1], o.n_rescued = h[2], o.n_star_records = h[3], o.n_star_entries = h[4];
	return o;
}

} // namespace povu_hip
