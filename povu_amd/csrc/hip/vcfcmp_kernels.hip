// vcfcmp_kernels.hip -- povu_hip_vcf_compare (include/povu_hip.h): how do the calls of one parsed VCF differ from another's?
//
// The definition is INTEGRATION.md "VCF comparison" (restated in tests/vcfcmp_ref.py; the rules that are plain arithmetic are
// vcfcmp_rules.hpp).  It reads no graph, no paths and no sequences.  Both documents are uploaded as one (vcf_pair.hpp: the
// host builder, the view, the items).
//   keys     the skip rule, the two trims and the hash of the trimmed key: the two tiers of vcf_pair.hpp over KeyPolicy, which
//            trims to vm_trim_limit, hashes REF' and ALT' and writes a key or a skipped item;
//   groups   exact_groups.hpp over (CHROM id, |REF'| + |ALT'|, hash), the comparison the rules' key equality; the groups of the
//            keyed items numbered in first-item order (number_groups), the member list the items stably sorted by that number;
//   classes  a lane per group: members of either side (A's items come first in a group's stretch), the class, the first item;
//   doses    a wave per group, lanes across the common samples in batches of 64: the members in rounds of 64 (a lane finds the
//            tasks of its member's ALT by two bisections), the tasks of a member in rounds of 64, a lane counting those of its
//            column; per-sample counts stay in the lane over all groups of the wave and are added once per wave and batch.
// Every shuffle and ballot runs with all 64 lanes (trip counts around them are wave-uniform); every store is inside the range
// the host carved: items below nI, groups below nG <= nI, samples below nC.
#include "exact_groups.hpp"
#include "vcf_pair.hpp"

namespace povu_hip
{

namespace
{

enum { CN_SHARED = 0, CN_ONLY_A, CN_ONLY_B, CN_SKIPPED_A, CN_SKIPPED_B, CN_WORDS = 8 };

// what the keys kernels write per item
struct VmKeys {
	uint8_t *state, *keep; // (keep: 1 for a keyed item, which the group numbering counts)
	uint64_t *pos;
	uint32_t *suffix, *prefix;
	uint32_t *rq, *rlen; // the grouping's query (CHROM id; n_chroms for a skipped item) and length
	uint64_t *rhash;
	uint64_t mask; // the bits of the hash that are kept (POVU_HIP_TRAV_HASH_BITS)
	uint32_t n_chroms;
};

__device__ __forceinline__ void write_skipped(const VmKeys &O, uint32_t i)
{
	O.state[i] = POVU_HIP_M_SKIPPED, O.keep[i] = 0;
	O.pos[i] = 0, O.suffix[i] = 0, O.prefix[i] = 0;
	O.rq[i] = O.n_chroms, O.rlen[i] = 0, O.rhash[i] = vm_mix64(i) & O.mask; // (equal to no item: SameKey)
}
__device__ __forceinline__ void write_key(const VmKeys &O, const PairView &A, uint32_t i, const PairView::Texts &T, uint64_t s, uint64_t p,
					  uint64_t ref_hash, uint64_t alt_hash)
{
	const uint32_t r = A.record_of(i);
	const uint64_t pos = A.pos[r] + p, nr = T.nr - s - p, na = T.na - s - p;
	O.state[i] = POVU_HIP_M_KEYED, O.keep[i] = 1;
	O.pos[i] = pos, O.suffix[i] = (uint32_t)s, O.prefix[i] = (uint32_t)p;
	O.rq[i] = A.chrom[r], O.rlen[i] = (uint32_t)(nr + na), O.rhash[i] = vm_key_hash(pos, nr, na, ref_hash, alt_hash) & O.mask;
}

// the keys as a policy of the two tiers (vcf_pair.hpp): no item is settled before its texts are looked at
struct KeyPolicy {
	VmKeys O;
	static constexpr bool HASH_REF = true;
	static __device__ __forceinline__ uint64_t trim_limit(uint64_t nr, uint64_t na) { return vm_trim_limit(nr, na); }
	__device__ __forceinline__ bool refused(const PairView &, uint32_t) const { return false; }
	__device__ __forceinline__ void on_refused(uint32_t) const {}
	__device__ __forceinline__ void on_skipped(uint32_t i) const { write_skipped(O, i); }
	__device__ __forceinline__ void on_trimmed(const PairView &A, uint32_t i, const PairView::Texts &T, uint64_t s, uint64_t p, uint64_t ref_hash,
					      uint64_t alt_hash) const
	{
		write_key(O, A, i, T, s, p, ref_hash, alt_hash);
	}
};

// items a and b of one CHROM have the same key
struct SameKey {
	PairView A;
	const uint8_t *state;
	const uint64_t *pos;
	const uint32_t *suffix, *prefix;
	__device__ __forceinline__ bool operator()(uint32_t a, uint32_t b) const
	{
		if (state[a] != POVU_HIP_M_KEYED || state[b] != POVU_HIP_M_KEYED)
			return false;
		const PairView::Texts Ta = A.texts(a), Tb = A.texts(b);
		const uint64_t pa = prefix[a], pb = prefix[b], ca = pa + suffix[a], cb = pb + suffix[b];
		return vm_same_key(pos[a], Ta.ref + pa, Ta.nr - ca, Ta.alt + pa, Ta.na - ca, pos[b], Tb.ref + pb, Tb.nr - cb, Tb.alt + pb, Tb.na - cb);
	}
};

// (the skipped items sort behind every group)
__global__ void k_vm_group_key(uint32_t n, uint32_t nG, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ gid, uint32_t *__restrict__ key)
{
	for (uint32_t x = blockIdx.x * Q_TPB + threadIdx.x; x < n; x += gridDim.x * Q_TPB)
		key[x] = min(gid[perm[x]], nG);
}
// the member list (the items sorted by group) and where every group begins in it; goff[nG]: behind the last group's members
__global__ void k_vm_members(uint32_t n, uint32_t nG, const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ gid,
			     uint32_t *__restrict__ member, uint32_t *__restrict__ goff)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x <= n; x += (uint64_t)gridDim.x * Q_TPB) {
		const uint32_t before = x ? min(gid[sorted[x - 1]], nG) : NO_QUERY;
		if (x == n) {
			if (before != nG)
				goff[nG] = n;
			continue;
		}
		const uint32_t i = sorted[x], g = min(gid[i], nG);
		member[x] = i;
		if (g != before)
			goff[g] = (uint32_t)x; // (g <= nG: inside the nG + 1 offsets)
	}
}

// ---- classes: a lane per group (the loop is by waves: every lane of a wave takes part in the counts)
__global__ __launch_bounds__(Q_TPB) void k_vm_classes(uint32_t nG, uint32_t nIa, const uint32_t *__restrict__ goff, const uint32_t *__restrict__ member,
						      uint8_t *__restrict__ g_class, uint32_t *__restrict__ g_na, uint32_t *__restrict__ g_nb,
						      uint32_t *__restrict__ g_first, unsigned long long *__restrict__ cnt)
{
	const uint32_t lane = threadIdx.x & 63u;
	unsigned long long mine[3] = {0, 0, 0};
	for (uint64_t b = ((uint64_t)blockIdx.x * Q_TPB + threadIdx.x) & ~63ull; b < nG; b += (uint64_t)gridDim.x * Q_TPB) {
		const uint64_t g = b + lane;
		uint32_t cls = 3; // (no group)
		if (g < nG) {
			const uint32_t m0 = goff[g], m1 = goff[g + 1];
			const uint32_t lo = lower_bound(member, m0, m1, nIa); // the first member that is an item of B: the members ascend
			cls = vm_group_class(lo - m0, m1 - lo);
			g_class[g] = (uint8_t)cls, g_na[g] = lo - m0, g_nb[g] = m1 - lo, g_first[g] = member[m0];
		}
#pragma unroll
		for (uint32_t c = 0; c < 3; c++)
			mine[c] += __popcll(__ballot(cls == c));
	}
#pragma unroll
	for (uint32_t c = 0; c < 3; c++)
		if (lane == 0 && mine[c])
			atomicAdd(cnt + CN_SHARED + c, mine[c]);
}
__global__ __launch_bounds__(Q_TPB) void k_vm_count_skipped(uint32_t nI, uint32_t nIa, const uint8_t *__restrict__ state, unsigned long long *__restrict__ cnt)
{
	const uint32_t lane = threadIdx.x & 63u;
	unsigned long long na = 0, nb = 0;
	for (uint64_t b = ((uint64_t)blockIdx.x * Q_TPB + threadIdx.x) & ~63ull; b < nI; b += (uint64_t)gridDim.x * Q_TPB) {
		const uint64_t i = b + lane;
		const bool skipped = i < nI && state[i] != POVU_HIP_M_KEYED;
		na += __popcll(__ballot(skipped && i < nIa));
		nb += __popcll(__ballot(skipped && i >= nIa));
	}
	if (lane == 0 && na)
		atomicAdd(cnt + CN_SKIPPED_A, na);
	if (lane == 0 && nb)
		atomicAdd(cnt + CN_SKIPPED_B, nb);
}

// ---- doses: a wave per group
struct VmDoses {
	uint32_t nG, nC;
	const uint32_t *goff, *member;
	const uint32_t *tkoff;		// [records + 1] tasks of a record, ascending by allele
	const uint32_t *t_al, *t_col;	// [tasks] the column within the task's document
	const uint32_t *col_a, *col_b;	// [nC] the columns of a common sample
	unsigned long long *tp, *fp, *fn, *gteq; // [nC]
};
__global__ __launch_bounds__(Q_TPB) void k_vm_doses(PairView A, VmDoses D)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64), wave = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6);
	for (uint32_t c0 = 0; c0 < D.nC; c0 += 64) {
		const uint32_t c = c0 + lane; // (nC + 64 < 2^32: a column is below the 2^32 - 64 tasks' bound of its document)
		const uint32_t col_a = c < D.nC ? D.col_a[c] : NO_QUERY, col_b = c < D.nC ? D.col_b[c] : NO_QUERY;
		unsigned long long tp = 0, fp = 0, fn = 0, gteq = 0; // of the lane's sample over the wave's groups
		for (uint32_t g = wave; g < D.nG; g += waves) {
			const uint32_t m0 = D.goff[g], m1 = D.goff[g + 1];
			uint32_t dose_a = 0, dose_b = 0;
			for (uint32_t mb = m0; mb < m1; mb += 64) { // the members, 64 a round: a lane finds the tasks of one
				uint32_t t0 = 0, t1 = 0, side = 0;
				if (mb + lane < m1) {
					const uint32_t i = D.member[mb + lane], r = A.record_of(i), k = A.it_k[i];
					side = i >= A.nIa;
					t0 = lower_bound(D.t_al, D.tkoff[r], D.tkoff[r + 1], k); // the first task whose allele is k or more
					t1 = lower_bound(D.t_al, t0, D.tkoff[r + 1], k + 1);
				}
				const uint32_t n_members = min(64u, m1 - mb);
				for (uint32_t j = 0; j < n_members; j++) {
					const uint32_t u0 = __shfl(t0, j, 64), u1 = __shfl(t1, j, 64), sd = __shfl(side, j, 64);
					const uint32_t my_col = sd ? col_b : col_a;
					uint32_t d = 0;
					for (uint32_t tb = u0; tb < u1; tb += 64) { // its tasks, 64 a round
						const uint32_t col = tb + lane < u1 ? D.t_col[tb + lane] : NO_QUERY;
						const uint32_t n_tasks = min(64u, u1 - tb);
						for (uint32_t x = 0; x < n_tasks; x++)
							d += __shfl(col, x, 64) == my_col; // (a task's column is no NO_QUERY)
					}
					dose_a += sd ? 0u : d, dose_b += sd ? d : 0u;
				}
			}
			const int cell = vm_cell(dose_a, dose_b);
			tp += cell == VM_CELL_TP, fp += cell == VM_CELL_FP, fn += cell == VM_CELL_FN, gteq += vm_gteq(dose_a, dose_b);
		}
		if (c < D.nC) {
			if (tp)
				atomicAdd(D.tp + c, tp);
			if (fp)
				atomicAdd(D.fp + c, fp);
			if (fn)
				atomicAdd(D.fn + c, fn);
			if (gteq)
				atomicAdd(D.gteq + c, gteq);
		}
	}
}

struct CmpOwner {
	povu_hip_vcf_cmp view{}; // first member: the owner is recovered from it in povu_hip_vcf_cmp_free
	PinnedVec<uint8_t> block; // every array of the view that came from the device, in one page-locked block (HostSpans)
	std::vector<uint32_t> col_a, col_b;
};

} // namespace

static povu_hip_vcf_cmp *vcf_compare(povu_hip_ctx *ctx, const povu_hip_vcf_doc *da, const povu_hip_vcf_doc *db, uint32_t flags, CallTimer &timer)
{
	PairWant want{};
	want.tkoff = want.t_al = want.t_col = true;
	PairUpload U = pair_build(ctx, da, db, "the VCF comparison needs ", want);
	const bool force = flags & POVU_HIP_V_FORCE_TIER2;
	const uint32_t nRa = U.nRa, nR = U.nR, nAl = U.nAl, nT = U.nT, nI = U.nI, nIa = U.nIa, nC = U.nC, n_chroms = U.n_chroms, hbits = hash_bits_hook();
	const size_t i1 = (size_t)nI + 1;
	auto o = std::make_unique<CmpOwner>();

	HIP_CHECK(hipSetDevice(ctx->device));
	ctx->wait_tail();
	hipStream_t s = U.s = ctx->stream;
	// ---- the layout: what is uploaded and worked on (vc_ws), the results (vc_hit)
	uint32_t *aoff, *tkoff, *ioff, *chrom, *t_al, *t_col, *col_a, *col_b, *it_rec, *it_k, *suffix, *prefix, *rq, *rlen, *t2, *firstf, *gidx, *gid, *member,
		*goff, *words, *g_na, *g_nb, *g_first;
	uint64_t *toff, *pos, *kpos, *rhash;
	uint8_t *state, *keep, *g_class;
	char *text;
	unsigned long long *cnt, *splits, *tp, *fp, *fn, *gteq;
	GroupWs gw;
	gw.tmp_bytes = prim_tmp_bytes(i1 + 1, true) + 256;
	timer.start(s);
	carve(ctx->vc_ws, [&](Spans &take) {
		take((size_t)nR + 1, aoff, tkoff, ioff, chrom, pos);
		take((size_t)nAl + 1, toff);
		take(U.n_text + 1, text);
		take((size_t)nT + 1, t_al, t_col);
		take((size_t)nC + 1, col_a, col_b);
		take(i1, rq, rlen, t2, firstf, gw.pa, gw.pb, gw.key, gw.kout, gw.mark, gw.hmax, gw.head, gw.rep, gw.blist, member);
		take(i1 + 1, gidx, goff);
		take(i1, rhash);
		take(i1, gw.rbad, keep);
		take(8, words);
		take(CN_WORDS, cnt);
		take(1, splits);
		take(gw.tmp_bytes, gw.tmp);
	});
	carve(ctx->vc_hit, [&](Spans &take) {
		take(i1, it_rec, it_k, suffix, prefix, gid, g_na, g_nb, g_first);
		take(i1, kpos);
		take(i1, state, g_class);
		take((size_t)nC + 1, tp, fp, fn, gteq);
	});
	U.up(aoff, U.aoff), U.up(tkoff, U.tkoff), U.up(ioff, U.ioff), U.up(chrom, U.chrom), U.up(pos, U.pos), U.up(toff, U.toff);
	U.up_text(text);
	U.up(t_al, U.t_al), U.up(t_col, U.t_col), U.up(col_a, U.col_a), U.up(col_b, U.col_b);
	HIP_CHECK(hipMemsetAsync(words, 0, 32, s));
	HIP_CHECK(hipMemsetAsync(cnt, 0, CN_WORDS * 8, s));
	for (unsigned long long *p : {tp, fp, fn, gteq})
		HIP_CHECK(hipMemsetAsync(p, 0, ((size_t)nC + 1) * 8, s));

	// ---- items, keys
	const PairView A{nR, nRa, nI, nIa, aoff, ioff, toff, text, pos, chrom, it_rec, it_k};
	const KeyPolicy K{{state, keep, kpos, suffix, prefix, rq, rlen, rhash, ((uint64_t)hash_mask_hi(hbits) << 32) | hash_mask_lo(hbits), n_chroms}};
	uint32_t n_t2 = 0, nG = 0;
	uint64_t n_splits = 0;
	if (nI) {
		n_t2 = launch_tiers(A, K, force, t2, words + 1, s);
		// ---- groups: the trimmed texts of a key have at most 2 * longest bytes, a CHROM id is at most n_chroms (a skipped item's)
		const uint32_t *sp = group_exact(nI, rq, rlen, rhash, hbits, bits_for(2 * U.longest), bits_for(n_chroms), SameKey{A, state, kpos, suffix, prefix},
						 gw, words + 2, splits, &n_splits, s);
		number_groups(nI, sp, gw.rep, firstf, gidx, keep, gw.tmp, gw.tmp_bytes, s);
		nG = read_back(gidx + nI, s); // (waits for the stream: n_splits has arrived)
		KLAUNCH(k_eg_group_of, dim3(stride_blocks(nI)), dim3(Q_TPB), 0, s, nI, sp, gw.rep, gidx, keep, gid);
		// ---- members: the items stably sorted by group, so those of a group stay in item order, A's first
		launch_iota(nI, gw.pa, s);
		LsdSort sort{gw.pa, gw.pb, gw.key, gw.kout, nI, gw.tmp, gw.tmp_bytes, s};
		sort.pass(0, bits_for(nG), [&](int, const uint32_t *cur, uint32_t *k) { KLAUNCH(k_vm_group_key, dim3(stride_blocks(nI)), dim3(Q_TPB), 0, s, nI, nG, cur, gid, k); });
		KLAUNCH(k_vm_members, dim3(stride_blocks(i1)), dim3(Q_TPB), 0, s, nI, nG, sort.cur, gid, member, goff);
		KLAUNCH(k_vm_count_skipped, dim3(std::min(stride_blocks(nI), COUNT_BLOCKS)), dim3(Q_TPB), 0, s, nI, nIa, state, cnt);
	}
	// ---- classes, doses
	if (nG) {
		KLAUNCH(k_vm_classes, dim3(std::min(stride_blocks(nG), COUNT_BLOCKS)), dim3(Q_TPB), 0, s, nG, nIa, goff, member, g_class, g_na, g_nb, g_first, cnt);
		if (nC) {
			const VmDoses D{nG, nC, goff, member, tkoff, t_al, t_col, col_a, col_b, tp, fp, fn, gteq};
			KLAUNCH(k_vm_doses, dim3(std::min(wave_blocks(nG), COUNT_BLOCKS)), dim3(Q_TPB), 0, s, A, D);
		}
	}

	// ---- to the host
	uint64_t h_cnt[CN_WORDS] = {0};
	povu_hip_vcf_cmp &v = o->view;
	static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are read as uint64_t");
	const size_t g1 = (size_t)nG + 1, c1 = (size_t)nC + 1;
	hand_off_block(o->block, ctx, [&](HostSpans &take) {
		const uint32_t *h_rec = take(it_rec, nI, i1), *h_k = take(it_k, nI, i1);
		const uint8_t *h_state = take(state, nI, i1);
		const uint64_t *h_pos = take(kpos, nI, i1);
		const uint32_t *h_suffix = take(suffix, nI, i1), *h_prefix = take(prefix, nI, i1), *h_gid = take(gid, nI, i1);
		v.group_class = take(g_class, nG, g1), v.group_n_a = take(g_na, nG, g1), v.group_n_b = take(g_nb, nG, g1), v.group_first = take(g_first, nG, g1);
		v.sample_tp = reinterpret_cast<const uint64_t *>(take(tp, nC, c1)), v.sample_fp = reinterpret_cast<const uint64_t *>(take(fp, nC, c1));
		v.sample_fn = reinterpret_cast<const uint64_t *>(take(fn, nC, c1)), v.sample_gteq = reinterpret_cast<const uint64_t *>(take(gteq, nC, c1));
		v.item_record_a = h_rec, v.item_record_b = h_rec + nIa, v.item_alt_a = h_k, v.item_alt_b = h_k + nIa;
		v.item_state_a = h_state, v.item_state_b = h_state + nIa, v.item_pos_a = h_pos, v.item_pos_b = h_pos + nIa;
		v.item_suffix_a = h_suffix, v.item_suffix_b = h_suffix + nIa, v.item_prefix_a = h_prefix, v.item_prefix_b = h_prefix + nIa;
		v.item_group_a = h_gid, v.item_group_b = h_gid + nIa;
	});
	HIP_CHECK(copy_async(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, s));
	v.device_ms = timer.stop(s);
	o->col_a = std::move(U.col_a), o->col_b = std::move(U.col_b);
	v.n_items_a = nIa, v.n_items_b = nI - nIa, v.n_groups = nG, v.n_common_samples = nC;
	v.sample_col_a = o->col_a.data(), v.sample_col_b = o->col_b.data();
	v.n_shared = h_cnt[CN_SHARED], v.n_only_a = h_cnt[CN_ONLY_A], v.n_only_b = h_cnt[CN_ONLY_B];
	v.n_skipped_a = h_cnt[CN_SKIPPED_A], v.n_skipped_b = h_cnt[CN_SKIPPED_B];
	v.n_samples_only_a = da->n_samples - nC, v.n_samples_only_b = db->n_samples - nC;
	v.n_tier2 = n_t2, v.n_splits = n_splits;
	return &o.release()->view;
}

} // namespace povu_hip

// ---- C ABI

extern "C" povu_hip_vcf_cmp *povu_hip_vcf_compare(povu_hip_ctx *ctx, const povu_hip_vcf_doc *doc_a, const povu_hip_vcf_doc *doc_b,
						  const povu_hip_vcf_opts *opts, char *err, size_t errlen)
{
	CallTimer timer;
	return guarded_call(ctx, err, errlen, (povu_hip_vcf_cmp *)nullptr, [&] { return vcf_compare(ctx, doc_a, doc_b, opts ? opts->flags : 0u, timer); });
}
extern "C" void povu_hip_vcf_cmp_free(povu_hip_vcf_cmp *c)
{
	delete reinterpret_cast<CmpOwner *>(c);
}
