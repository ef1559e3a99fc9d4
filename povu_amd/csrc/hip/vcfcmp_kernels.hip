// vcfcmp_kernels.hip -- povu_hip_vcf_compare (include/povu_hip.h): how do the calls of one parsed VCF differ from another's?
//
// The definition is INTEGRATION.md "VCF comparison" (restated in tests/vcfcmp_ref.py; the rules that are plain arithmetic are
// vcfcmp_rules.hpp).  It reads no graph, no paths and no sequences.  Both documents are uploaded as one: A's records, alleles,
// texts and tasks, then B's, the CHROM strings interned over both.
//   items    one per (record, ALT): the host sums the ALT counts to offsets, a lane per item finds its record in them;
//   keys     the skip rule, the two trims and the hash of the trimmed key.  A lane per item while the shorter text has at most
//            TIER1_BYTES bytes, else a wave per item: 64 bytes a ballot backwards, then forwards, the hash a sum of per-lane
//            partial polynomials (the same value whichever kernel computes it);
//   groups   exact_groups.hpp over (CHROM id, |REF'| + |ALT'|, hash), the comparison the rules' key equality; the groups
//            numbered by a scan over their first items, the member list the items stably sorted by that number;
//   classes  a lane per group: members of either side (A's items come first in a group's stretch), the class, the first item;
//   doses    a wave per group, lanes across the common samples in batches of 64: the members in rounds of 64 (a lane finds the
//            tasks of its member's ALT by two bisections), the tasks of a member in rounds of 64, a lane counting those of its
//            column; per-sample counts stay in the lane over all groups of the wave and are added once per wave and batch.
// Every shuffle and ballot runs with all 64 lanes (trip counts around them are wave-uniform); every store is inside the range
// the host carved: items below nI, groups below nG <= nI, samples below nC.
#include "call_common.hpp"
#include "exact_groups.hpp"
#include "vcfcmp_rules.hpp"

#include <string>
#include <unordered_map>

namespace povu_hip
{

namespace
{

constexpr uint32_t TIER1_BYTES = 32;
constexpr unsigned COUNT_BLOCKS = 2048; // (the device's wave slots at 256 lanes a workgroup: what the counting kernels stride over)
enum { CN_SHARED = 0, CN_ONLY_A, CN_ONLY_B, CN_SKIPPED_A, CN_SKIPPED_B, CN_WORDS = 8 };

// both documents as one, and the items
struct VmView {
	uint32_t nI, nIa, nRa;	 // items, those of A, records of A
	const uint32_t *aoff;	 // [records + 1] alleles of a record
	const uint64_t *toff;	 // [alleles + 1]
	const char *text;
	const uint64_t *pos;	 // [records]
	const uint32_t *chrom;	 // [records] CHROM id over both documents
	uint32_t *it_rec, *it_k; // [nI] the record within its document, the ALT
	struct Texts {
		const char *ref, *alt;
		uint64_t nr, na;
	};
	__device__ __forceinline__ uint32_t record_of(uint32_t i) const { return it_rec[i] + (i >= nIa ? nRa : 0u); }
	__device__ __forceinline__ Texts texts(uint32_t i) const
	{
		const uint32_t ar = aoff[record_of(i)], aa = ar + it_k[i];
		return {text + toff[ar], text + toff[aa], toff[ar + 1] - toff[ar], toff[aa + 1] - toff[aa]};
	}
};
// what the keys kernels write per item
struct VmKeys {
	uint8_t *state;
	uint64_t *pos;
	uint32_t *suffix, *prefix;
	uint32_t *rq, *rlen; // the grouping's query (CHROM id; n_chroms for a skipped item) and length
	uint64_t *rhash;
	uint64_t mask; // the bits of the hash that are kept (POVU_HIP_TRAV_HASH_BITS)
	uint32_t n_chroms;
};

__global__ void k_vm_items(VmView A, uint32_t nR, const uint32_t *__restrict__ ioff)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < A.nI; i += gridDim.x * Q_TPB) {
		uint32_t lo = 0, hi = nR; // the last record whose items begin at or before i (ioff[0] = 0, nI > 0 hence nR > 0)
		while (hi - lo > 1) {
			const uint32_t mid = (lo + hi) >> 1;
			if (ioff[mid] <= i)
				lo = mid;
			else
				hi = mid;
		}
		A.it_rec[i] = lo - (lo >= A.nRa ? A.nRa : 0u);
		A.it_k[i] = i - ioff[lo] + 1;
	}
}

__device__ __forceinline__ void write_skipped(const VmKeys &O, uint32_t i)
{
	O.state[i] = POVU_HIP_M_SKIPPED;
	O.pos[i] = 0, O.suffix[i] = 0, O.prefix[i] = 0;
	O.rq[i] = O.n_chroms, O.rlen[i] = 0, O.rhash[i] = vm_mix64(i) & O.mask; // (equal to no item: SameKey)
}
__device__ __forceinline__ void write_key(const VmKeys &O, const VmView &A, uint32_t i, const VmView::Texts &T, uint64_t s, uint64_t p,
					  uint64_t ref_hash, uint64_t alt_hash)
{
	const uint32_t r = A.record_of(i);
	const uint64_t pos = A.pos[r] + p, nr = T.nr - s - p, na = T.na - s - p;
	O.state[i] = POVU_HIP_M_KEYED;
	O.pos[i] = pos, O.suffix[i] = (uint32_t)s, O.prefix[i] = (uint32_t)p;
	O.rq[i] = A.chrom[r], O.rlen[i] = (uint32_t)(nr + na), O.rhash[i] = vm_key_hash(pos, nr, na, ref_hash, alt_hash) & O.mask;
}

// tier 1: a lane per item; the items whose shorter text is long (or every item, with force) go to `t2`
__global__ void k_vm_keys(VmView A, VmKeys O, uint32_t force, uint32_t *__restrict__ t2, uint32_t *__restrict__ n_t2)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < A.nI; i += gridDim.x * Q_TPB) {
		const VmView::Texts T = A.texts(i);
		if (force || min(T.nr, T.na) > TIER1_BYTES) {
			t2[atomicAdd(n_t2, 1u)] = i; // (at most nI of them)
			continue;
		}
		if (vm_skipped(T.ref, T.nr, T.alt, T.na)) {
			write_skipped(O, i);
			continue;
		}
		const uint64_t s = vm_suffix(T.ref, T.nr, T.alt, T.na), p = vm_prefix(T.ref, T.nr, T.alt, T.na, s);
		write_key(O, A, i, T, s, p, vm_text_hash(T.ref + p, T.nr - s - p), vm_text_hash(T.alt + p, T.na - s - p));
	}
}

// the polynomial hash of t[0, n), lanes across the bytes
__device__ __forceinline__ uint64_t wave_text_hash(const char *__restrict__ t, uint64_t n, uint32_t lane)
{
	uint64_t h = 0, power = vm_pow(lane);
	const uint64_t stride = vm_pow(64);
	for (uint64_t x = lane; x < n; x += 64, power *= stride)
		h += vm_term(t[x], power);
	return wave_sum(h);
}
// tier 2: a wave per item of `t2`
__global__ __launch_bounds__(Q_TPB) void k_vm_keys_wave(const uint32_t *__restrict__ t2, uint32_t n2, VmView A, VmKeys O)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	for (uint32_t x = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); x < n2; x += waves) {
		const uint32_t i = t2[x];
		const VmView::Texts T = A.texts(i);
		bool skip = vm_skip_head(T.ref, T.nr, T.alt, T.na);
		for (uint64_t c0 = 0; !skip && c0 < T.na; c0 += 64)
			skip = __ballot(c0 + lane < T.na && vm_skip_byte(T.alt[c0 + lane])) != 0;
		if (skip) {
			if (lane == 0)
				write_skipped(O, i);
			continue;
		}
		uint64_t limit = vm_trim_limit(T.nr, T.na), s = limit;
		for (uint64_t c0 = 0; c0 < limit; c0 += 64) {
			const unsigned long long m = __ballot(c0 + lane < limit && vm_suffix_differs(T.ref, T.nr, T.alt, T.na, c0 + lane));
			if (m) {
				s = c0 + (uint64_t)(__ffsll((long long)m) - 1);
				break;
			}
		}
		limit = vm_trim_limit(T.nr - s, T.na - s);
		uint64_t p = limit;
		for (uint64_t c0 = 0; c0 < limit; c0 += 64) {
			const unsigned long long m = __ballot(c0 + lane < limit && vm_prefix_differs(T.ref, T.alt, c0 + lane));
			if (m) {
				p = c0 + (uint64_t)(__ffsll((long long)m) - 1);
				break;
			}
		}
		const uint64_t hr = wave_text_hash(T.ref + p, T.nr - s - p, lane), ha = wave_text_hash(T.alt + p, T.na - s - p, lane);
		if (lane == 0)
			write_key(O, A, i, T, s, p, hr, ha);
	}
}

// items a and b of one CHROM have the same key
struct SameKey {
	VmView A;
	const uint8_t *state;
	const uint64_t *pos;
	const uint32_t *suffix, *prefix;
	__device__ __forceinline__ bool operator()(uint32_t a, uint32_t b) const
	{
		if (state[a] != POVU_HIP_M_KEYED || state[b] != POVU_HIP_M_KEYED)
			return false;
		const VmView::Texts Ta = A.texts(a), Tb = A.texts(b);
		const uint64_t pa = prefix[a], pb = prefix[b], ca = pa + suffix[a], cb = pb + suffix[b];
		return vm_same_key(pos[a], Ta.ref + pa, Ta.nr - ca, Ta.alt + pa, Ta.na - ca, pos[b], Tb.ref + pb, Tb.nr - cb, Tb.alt + pb, Tb.na - cb);
	}
};

// a skipped item is the first of no group
__global__ void k_vm_keyed_firsts(uint32_t n, const uint8_t *__restrict__ state, uint32_t *__restrict__ firstf)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < n; i += gridDim.x * Q_TPB)
		if (state[i] != POVU_HIP_M_KEYED)
			firstf[i] = 0;
}
// group number of every item, from its group's first member
__global__ void k_vm_group_of(uint32_t n, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ rep, const uint32_t *__restrict__ gidx,
			      const uint8_t *__restrict__ state, uint32_t *__restrict__ gid)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < n; k += gridDim.x * Q_TPB) {
		const uint32_t r = rep[k], i = perm[k];
		gid[i] = state[i] != POVU_HIP_M_KEYED ? NO_QUERY : gidx[perm[r < n ? r : k]];
	}
}
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
			uint32_t lo = m0, hi = m1; // the first member that is an item of B: the members ascend
			while (lo < hi) {
				const uint32_t mid = lo + ((hi - lo) >> 1);
				if (member[mid] < nIa)
					lo = mid + 1;
				else
					hi = mid;
			}
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
// the first task of [lo, hi) whose allele is k or more
__device__ __forceinline__ uint32_t first_task_of(const uint32_t *__restrict__ t_al, uint32_t lo, uint32_t hi, uint32_t k)
{
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (t_al[mid] < k)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}
__global__ __launch_bounds__(Q_TPB) void k_vm_doses(VmView A, VmDoses D)
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
					t0 = first_task_of(D.t_al, D.tkoff[r], D.tkoff[r + 1], k);
					t1 = first_task_of(D.t_al, t0, D.tkoff[r + 1], k + 1);
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
	PinnedVec<uint32_t> it_rec, it_k, suffix, prefix, gid, g_na, g_nb, g_first;
	PinnedVec<uint8_t> state, g_class;
	PinnedVec<uint64_t> pos;
	PinnedVec<unsigned long long> tp, fp, fn, gteq;
	std::vector<uint32_t> col_a, col_b;
};

// what the kernels index by must lie within what they index (all true of povu_hip_vcf_parse)
void check_cmp_doc(const povu_hip_vcf_doc *d, const char *which)
{
	auto ascends = [](const uint64_t *off, uint64_t n, uint64_t total) {
		if (!off || off[0] != 0 || off[n] != total)
			return false;
		for (uint64_t k = 0; k < n; k++)
			if (off[k] > off[k + 1])
				return false;
		return true;
	};
	bool ok = ascends(d->allele_off, d->n_records, d->n_alleles) && ascends(d->task_off, d->n_records, d->n_tasks) &&
		  ascends(d->text_off, d->n_alleles, d->n_text_bytes) && (!d->n_records || (d->rec_chrom && d->chrom && d->rec_pos)) &&
		  (!d->n_alleles || d->allele_walk) && (!d->n_text_bytes || d->text) && (!d->n_samples || d->sample) &&
		  (!d->n_tasks || (d->task_record && d->task_allele && d->task_col));
	for (uint64_t c = 0; ok && c < d->n_samples; c++)
		ok = d->sample[c] != nullptr;
	for (uint64_t r = 0; ok && r < d->n_records; r++) {
		ok = d->rec_chrom[r] < d->n_chroms && d->chrom[d->rec_chrom[r]];
		for (uint64_t t = d->task_off[r]; ok && t < d->task_off[r + 1]; t++)
			ok = d->task_record[t] == r && d->task_col[t] < d->n_samples && (t == d->task_off[r] || d->task_allele[t - 1] <= d->task_allele[t]);
	}
	if (!ok)
		throw HipError(std::string("the offsets, tasks and CHROM ids of document ") + which + " do not belong together");
}
// the ALTs of record r: its alleles with a text, REF first, but REF
uint64_t alts_of(const povu_hip_vcf_doc *d, uint64_t r)
{
	uint64_t n = 0;
	for (uint64_t a = d->allele_off[r]; a < d->allele_off[r + 1] && (d->allele_walk[a] & 2u); a++)
		n++;
	return n ? n - 1 : 0;
}

} // namespace

static povu_hip_vcf_cmp *vcf_compare(povu_hip_ctx *ctx, const povu_hip_vcf_doc *da, const povu_hip_vcf_doc *db, uint32_t flags, CallTimer &timer)
{
	if (!ctx || !da || !db)
		throw HipError("null context or document");
	const bool force = flags & POVU_HIP_V_FORCE_TIER2;
	const povu_hip_vcf_doc *docs[2] = {da, db};
	const char *who = "the VCF comparison needs ";
	for (const povu_hip_vcf_doc *d : docs) { // (a side first: the sums below do not wrap)
		refuse_2_32(d->n_records + 64, who, "records of a document");
		refuse_2_32(d->n_alleles + 64, who, "alleles of a document");
		refuse_2_32(d->n_tasks + 64, who, "tasks of a document");
		refuse_2_32(d->n_text_bytes + 64, who, "text bytes of a document");
		refuse_2_32(d->n_samples + 64, who, "sample columns of a document");
	}
	refuse_2_32(da->n_records + db->n_records + 64, who, "records");
	refuse_2_32(da->n_alleles + db->n_alleles + 64, who, "alleles");
	refuse_2_32(da->n_tasks + db->n_tasks + 64, who, "tasks");
	refuse_2_32(da->n_text_bytes + db->n_text_bytes + 64, who, "text bytes");
	check_cmp_doc(da, "A");
	check_cmp_doc(db, "B");
	const uint32_t nRa = (uint32_t)da->n_records, nR = nRa + (uint32_t)db->n_records, nAl = (uint32_t)(da->n_alleles + db->n_alleles);
	const uint32_t nT = (uint32_t)(da->n_tasks + db->n_tasks), hbits = hash_bits_hook();
	const uint64_t n_text = da->n_text_bytes + db->n_text_bytes;

	// ---- both documents as one; the items' offsets; the CHROM ids; the common samples
	std::vector<uint32_t> h_aoff((size_t)nR + 1), h_tkoff((size_t)nR + 1), h_ioff((size_t)nR + 1), h_chrom(nR), h_tal(nT), h_tcol(nT);
	std::vector<uint64_t> h_toff((size_t)nAl + 1), h_pos(nR);
	std::unordered_map<std::string, uint32_t> chrom_of;
	uint64_t n_items = 0, n_items_a = 0, longest = 0;
	{
		uint64_t r0 = 0, a0 = 0, t0 = 0, x0 = 0;
		for (int side = 0; side < 2; side++) { // (by side, not by pointer: a document may be compared with itself)
			const povu_hip_vcf_doc *d = docs[side];
			std::vector<uint32_t> id(d->n_chroms);
			for (uint64_t k = 0; k < d->n_chroms; k++)
				id[k] = d->chrom[k] ? chrom_of.emplace(d->chrom[k], (uint32_t)chrom_of.size()).first->second : 0u;
			for (uint64_t r = 0; r < d->n_records; r++) {
				h_aoff[r0 + r] = (uint32_t)(a0 + d->allele_off[r]);
				h_tkoff[r0 + r] = (uint32_t)(t0 + d->task_off[r]);
				h_ioff[r0 + r] = (uint32_t)std::min<uint64_t>(n_items, 0xFFFFFFFFull);
				h_pos[r0 + r] = d->rec_pos[r];
				h_chrom[r0 + r] = id[d->rec_chrom[r]];
				const uint64_t alts = alts_of(d, r), ar = d->allele_off[r];
				n_items += alts;
				for (uint64_t k = 0; k <= alts && ar + k < d->allele_off[r + 1]; k++)
					longest = std::max(longest, d->text_off[ar + k + 1] - d->text_off[ar + k]);
			}
			for (uint64_t a = 0; a < d->n_alleles; a++)
				h_toff[a0 + a] = x0 + d->text_off[a];
			for (uint64_t t = 0; t < d->n_tasks; t++)
				h_tal[t0 + t] = d->task_allele[t], h_tcol[t0 + t] = d->task_col[t];
			r0 += d->n_records, a0 += d->n_alleles, t0 += d->n_tasks, x0 += d->n_text_bytes;
			if (side == 0)
				n_items_a = n_items;
		}
		h_aoff[nR] = nAl, h_tkoff[nR] = nT, h_toff[nAl] = n_text;
	}
	refuse_2_32(n_items + 64, who, "(record, ALT) items");
	h_ioff[nR] = (uint32_t)n_items;
	const uint32_t nI = (uint32_t)n_items, nIa = (uint32_t)n_items_a, n_chroms = (uint32_t)chrom_of.size();
	auto o = std::make_unique<CmpOwner>();
	{
		std::unordered_map<std::string, uint32_t> col_of_b; // (of several columns of one name the first counts)
		for (uint64_t c = 0; c < db->n_samples; c++)
			col_of_b.emplace(db->sample[c], (uint32_t)c);
		for (uint64_t c = 0; c < da->n_samples; c++) {
			const auto at = col_of_b.find(da->sample[c]);
			if (at == col_of_b.end())
				continue;
			o->col_a.push_back((uint32_t)c), o->col_b.push_back(at->second);
			col_of_b.erase(at);
		}
	}
	const uint32_t nC = (uint32_t)o->col_a.size();
	const size_t i1 = (size_t)nI + 1;

	HIP_CHECK(hipSetDevice(ctx->device));
	ctx->wait_tail();
	hipStream_t s = ctx->stream;
	// ---- the layout: what is uploaded and worked on (vc_ws), the results (vc_hit)
	uint32_t *aoff, *tkoff, *ioff, *chrom, *t_al, *t_col, *col_a, *col_b, *it_rec, *it_k, *suffix, *prefix, *rq, *rlen, *t2, *firstf, *gidx, *gid, *member,
		*goff, *words, *g_na, *g_nb, *g_first;
	uint64_t *toff, *pos, *kpos, *rhash;
	uint8_t *state, *g_class;
	char *text;
	unsigned long long *cnt, *splits, *tp, *fp, *fn, *gteq;
	GroupWs gw;
	gw.tmp_bytes = prim_tmp_bytes(i1 + 1, true) + 256;
	timer.start(s);
	carve(ctx->vc_ws, [&](Spans &take) {
		take((size_t)nR + 1, aoff, tkoff, ioff, chrom, pos);
		take((size_t)nAl + 1, toff);
		take(n_text + 1, text);
		take((size_t)nT + 1, t_al, t_col);
		take((size_t)nC + 1, col_a, col_b);
		take(i1, rq, rlen, t2, firstf, gw.pa, gw.pb, gw.key, gw.kout, gw.mark, gw.hmax, gw.head, gw.rep, gw.blist, member);
		take(i1 + 1, gidx, goff);
		take(i1, rhash);
		take(i1, gw.rbad);
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
	auto up = [&](void *dst, const void *src, size_t bytes) {
		if (bytes)
			HIP_CHECK(copy_async(dst, src, bytes, hipMemcpyHostToDevice, s));
	};
	up(aoff, h_aoff.data(), ((size_t)nR + 1) * 4);
	up(tkoff, h_tkoff.data(), ((size_t)nR + 1) * 4);
	up(ioff, h_ioff.data(), ((size_t)nR + 1) * 4);
	up(chrom, h_chrom.data(), (size_t)nR * 4);
	up(pos, h_pos.data(), (size_t)nR * 8);
	up(toff, h_toff.data(), ((size_t)nAl + 1) * 8);
	up(text, da->text, da->n_text_bytes);
	up(text + da->n_text_bytes, db->text, db->n_text_bytes);
	up(t_al, h_tal.data(), (size_t)nT * 4);
	up(t_col, h_tcol.data(), (size_t)nT * 4);
	up(col_a, o->col_a.data(), (size_t)nC * 4);
	up(col_b, o->col_b.data(), (size_t)nC * 4);
	HIP_CHECK(hipMemsetAsync(words, 0, 32, s));
	HIP_CHECK(hipMemsetAsync(cnt, 0, CN_WORDS * 8, s));
	for (unsigned long long *p : {tp, fp, fn, gteq})
		HIP_CHECK(hipMemsetAsync(p, 0, ((size_t)nC + 1) * 8, s));

	// ---- items, keys
	const VmView A{nI, nIa, nRa, aoff, toff, text, pos, chrom, it_rec, it_k};
	const VmKeys K{state, kpos, suffix, prefix, rq, rlen, rhash, ((uint64_t)hash_mask_hi(hbits) << 32) | hash_mask_lo(hbits), n_chroms};
	uint32_t n_t2 = 0, nG = 0;
	uint64_t n_splits = 0;
	if (nI) {
		KLAUNCH(k_vm_items, dim3(stride_blocks(nI)), dim3(Q_TPB), 0, s, A, nR, ioff);
		KLAUNCH(k_vm_keys, dim3(stride_blocks(nI)), dim3(Q_TPB), 0, s, A, K, force ? 1u : 0u, t2, words + 1);
		n_t2 = read_back(words + 1, s);
		if (n_t2)
			KLAUNCH(k_vm_keys_wave, dim3(wave_blocks(n_t2)), dim3(Q_TPB), 0, s, t2, n_t2, A, K);
		// ---- groups: the trimmed texts of a key have at most 2 * longest bytes, a CHROM id is at most n_chroms (a skipped item's)
		const uint32_t *sp = group_exact(nI, rq, rlen, rhash, hbits, bits_for(2 * longest), bits_for(n_chroms), SameKey{A, state, kpos, suffix, prefix}, gw,
						 words + 2, splits, &n_splits, s);
		HIP_CHECK(hipMemsetAsync(firstf, 0, i1 * 4, s));
		KLAUNCH(k_eg_first, dim3(stride_blocks(nI)), dim3(Q_TPB), 0, s, nI, sp, gw.rep, firstf);
		KLAUNCH(k_vm_keyed_firsts, dim3(stride_blocks(nI)), dim3(Q_TPB), 0, s, nI, state, firstf);
		scan_exclusive_u32(firstf, gidx, i1, gw.tmp, gw.tmp_bytes, s);
		nG = read_back(gidx + nI, s); // (waits for the stream: n_splits has arrived)
		KLAUNCH(k_vm_group_of, dim3(stride_blocks(nI)), dim3(Q_TPB), 0, s, nI, sp, gw.rep, gidx, state, gid);
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
	hand_off(o->it_rec, i1, it_rec, nI, ctx);
	hand_off(o->it_k, i1, it_k, nI, ctx);
	hand_off(o->state, i1, state, nI, ctx);
	hand_off(o->pos, i1, kpos, nI, ctx);
	hand_off(o->suffix, i1, suffix, nI, ctx);
	hand_off(o->prefix, i1, prefix, nI, ctx);
	hand_off(o->gid, i1, gid, nI, ctx);
	hand_off(o->g_class, (size_t)nG + 1, g_class, nG, ctx);
	hand_off(o->g_na, (size_t)nG + 1, g_na, nG, ctx);
	hand_off(o->g_nb, (size_t)nG + 1, g_nb, nG, ctx);
	hand_off(o->g_first, (size_t)nG + 1, g_first, nG, ctx);
	hand_off(o->tp, (size_t)nC + 1, tp, nC, ctx);
	hand_off(o->fp, (size_t)nC + 1, fp, nC, ctx);
	hand_off(o->fn, (size_t)nC + 1, fn, nC, ctx);
	hand_off(o->gteq, (size_t)nC + 1, gteq, nC, ctx);
	HIP_CHECK(copy_async(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, s));
	povu_hip_vcf_cmp &v = o->view;
	v.device_ms = timer.stop(s);
	v.n_items_a = nIa, v.n_items_b = nI - nIa, v.n_groups = nG, v.n_common_samples = nC;
	v.item_record_a = o->it_rec.data(), v.item_record_b = o->it_rec.data() + nIa;
	v.item_alt_a = o->it_k.data(), v.item_alt_b = o->it_k.data() + nIa;
	v.item_state_a = o->state.data(), v.item_state_b = o->state.data() + nIa;
	v.item_pos_a = o->pos.data(), v.item_pos_b = o->pos.data() + nIa;
	v.item_suffix_a = o->suffix.data(), v.item_suffix_b = o->suffix.data() + nIa;
	v.item_prefix_a = o->prefix.data(), v.item_prefix_b = o->prefix.data() + nIa;
	v.item_group_a = o->gid.data(), v.item_group_b = o->gid.data() + nIa;
	v.group_class = o->g_class.data(), v.group_n_a = o->g_na.data(), v.group_n_b = o->g_nb.data(), v.group_first = o->g_first.data();
	v.sample_col_a = o->col_a.data(), v.sample_col_b = o->col_b.data();
	static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are read as uint64_t");
	v.sample_tp = reinterpret_cast<const uint64_t *>(o->tp.data()), v.sample_fp = reinterpret_cast<const uint64_t *>(o->fp.data());
	v.sample_fn = reinterpret_cast<const uint64_t *>(o->fn.data()), v.sample_gteq = reinterpret_cast<const uint64_t *>(o->gteq.data());
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
