// vcf_pair.hpp -- two parsed VCFs as one: what the VCF comparison (vcfcmp_kernels.hip) and the haplotype comparison
// (vcfhap_kernels.hip) do alike before they differ.
//   host     pair_build (vcf_pair.hip): the refusals, both documents laid end to end -- A's records, alleles, texts and tasks,
//            then B's, the CHROM strings interned over both --, the items' offsets, the common samples; PairUpload carries the
//            host arrays to the device, HostSpans brings a result's arrays back in one page-locked block;
//   items    PairView, the device's view of the pair; k_pair_items: a lane per (record, ALT) finds its record in the offsets;
//   tiers    tier_items<P>: a lane per item while the shorter text has at most TIER1_BYTES bytes; tier_items_wave<P>: a wave
//            per item beyond that, through the wave loops of vcfcmp_rules.hpp (64 bytes a ballot backwards, then forwards,
//            the hash a sum of per-lane partial polynomials: the same value whichever kernel computes it).  The policy P says
//            what the caller makes of an item: a key, or an edit.
// Every ballot and shuffle of the wave tier runs with all 64 lanes: LaneWave's calls are made by every lane of the wave, with
// wave-uniform trip counts around them (vcfcmp_rules.hpp, "a wave at a time").
#pragma once
#include "query_common.hpp"
#include "vcfcmp_rules.hpp"

#include <string>
#include <vector>

namespace povu_hip
{

constexpr uint32_t TIER1_BYTES = 32;
constexpr unsigned COUNT_BLOCKS = 2048; // (the device's wave slots at 256 lanes a workgroup: what the counting kernels stride over)

// both documents as one, and the items
struct PairView {
	uint32_t nR, nRa, nI, nIa; // records, those of A, items, those of A
	const uint32_t *aoff;	   // [nR + 1] alleles of a record
	const uint32_t *ioff;	   // [nR + 1] items of a record
	const uint64_t *toff;	   // [alleles + 1]
	const char *text;
	const uint64_t *pos;	 // [nR]
	const uint32_t *chrom;	 // [nR] CHROM id over both documents
	uint32_t *it_rec, *it_k; // [nI] the record within its document, the ALT
	struct Texts {
		const char *ref, *alt;
		uint64_t nr, na;
	};
	__device__ __forceinline__ uint32_t record_of(uint32_t i) const { return it_rec[i] + (i >= nIa ? nRa : 0u); }
	__device__ __forceinline__ uint64_t ref_len(uint32_t r) const
	{
		const uint32_t ar = aoff[r];
		return aoff[r + 1] > ar ? toff[ar + 1] - toff[ar] : 0;
	}
	__device__ __forceinline__ Texts texts(uint32_t i) const
	{
		const uint32_t ar = aoff[record_of(i)], aa = ar + it_k[i];
		return {text + toff[ar], text + toff[aa], toff[ar + 1] - toff[ar], toff[aa + 1] - toff[aa]};
	}
};

[[maybe_unused]] static __global__ void k_pair_items(PairView A)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < A.nI; i += gridDim.x * Q_TPB) {
		const uint32_t lo = span_of(A.ioff, A.nR, i); // the last record whose items begin at or before i (ioff[0] = 0, nI > 0 hence nR > 0)
		A.it_rec[i] = lo - (lo >= A.nRa ? A.nRa : 0u);
		A.it_k[i] = i - A.ioff[lo] + 1;
	}
}

// the wave of the calling lane, for the wave loops of vcfcmp_rules.hpp: every lane of the wave makes the call
struct LaneWave {
	uint32_t lane;
	template <class F>
	__device__ __forceinline__ uint64_t ballot(F &&f) const { return __ballot(f(lane)); }
	template <class F>
	__device__ __forceinline__ uint64_t sum(F &&f) const { return wave_sum(f(lane)); }
};

// The two tiers over a policy P, which holds the caller's output arrays and says
//   P::HASH_REF                            whether the trimmed REF is hashed beside the trimmed ALT;
//   P::trim_limit(nr, na)                  how many bytes a trim may take of texts of these lengths;
//   refused(A, i), on_refused(i)           an item settled before its texts are looked at, and its writer;
//   on_skipped(i)                          the writer of an item under the skip rule;
//   on_trimmed(A, i, T, s, p, ref_hash, alt_hash)  the writer of a trimmed item (ref_hash 0 without HASH_REF).
// tier 1: a lane per item; the items whose shorter text is long (or every item, with force) go to `t2`
template <class P>
__global__ void tier_items(PairView A, P O, uint32_t force, uint32_t *__restrict__ t2, uint32_t *__restrict__ n_t2)
{
	for (uint32_t i = blockIdx.x * Q_TPB + threadIdx.x; i < A.nI; i += gridDim.x * Q_TPB) {
		const PairView::Texts T = A.texts(i);
		if (force || min(T.nr, T.na) > TIER1_BYTES) {
			t2[atomicAdd(n_t2, 1u)] = i; // (at most nI of them)
			continue;
		}
		if (O.refused(A, i)) {
			O.on_refused(i);
			continue;
		}
		if (vm_skipped(T.ref, T.nr, T.alt, T.na)) {
			O.on_skipped(i);
			continue;
		}
		const uint64_t s = vm_suffix_upto(T.ref, T.nr, T.alt, T.na, P::trim_limit(T.nr, T.na));
		const uint64_t p = vm_prefix_upto(T.ref, T.alt, P::trim_limit(T.nr - s, T.na - s));
		O.on_trimmed(A, i, T, s, p, P::HASH_REF ? vm_text_hash(T.ref + p, T.nr - s - p) : 0, vm_text_hash(T.alt + p, T.na - s - p));
	}
}
// tier 2: a wave per item of `t2`
template <class P>
__global__ __launch_bounds__(Q_TPB) void tier_items_wave(const uint32_t *__restrict__ t2, uint32_t n2, PairView A, P O)
{
	const LaneWave w{threadIdx.x & 63u};
	const uint32_t waves = gridDim.x * (Q_TPB / 64);
	const auto limit = [](uint64_t nr, uint64_t na) { return P::trim_limit(nr, na); };
	for (uint32_t x = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); x < n2; x += waves) {
		const uint32_t i = t2[x];
		const PairView::Texts T = A.texts(i);
		if (O.refused(A, i)) {
			if (w.lane == 0)
				O.on_refused(i);
			continue;
		}
		if (wave_skipped(T.ref, T.nr, T.alt, T.na, w)) {
			if (w.lane == 0)
				O.on_skipped(i);
			continue;
		}
		const uint64_t s = wave_suffix(T.ref, T.nr, T.alt, T.na, limit, w), p = wave_prefix(T.ref, T.nr, T.alt, T.na, s, limit, w);
		const uint64_t hr = P::HASH_REF ? wave_text_hash(T.ref + p, T.nr - s - p, w) : 0, ha = wave_text_hash(T.alt + p, T.na - s - p, w);
		if (w.lane == 0)
			O.on_trimmed(A, i, T, s, p, hr, ha);
	}
}
// both tiers over the nI > 0 items; gives the number of items the wave tier took.  t2: [nI]; n_t2: a cleared word
template <class P>
uint32_t launch_tiers(const PairView &A, const P &O, bool force, uint32_t *t2, uint32_t *n_t2, hipStream_t s)
{
	KLAUNCH(k_pair_items, dim3(stride_blocks(A.nI)), dim3(Q_TPB), 0, s, A);
	KLAUNCH(tier_items<P>, dim3(stride_blocks(A.nI)), dim3(Q_TPB), 0, s, A, O, force ? 1u : 0u, t2, n_t2);
	const uint32_t n2 = read_back(n_t2, s);
	if (n2)
		KLAUNCH(tier_items_wave<P>, dim3(wave_blocks(n2)), dim3(Q_TPB), 0, s, t2, n2, A, O);
	return n2;
}

// ---- the host's half (vcf_pair.hip)

// which task arrays and sample tables a caller uploads: pair_build fills no other (the task words of a large pair are
// gigabytes, and the host's copy of them is most of a call's wall time)
struct PairWant {
	bool tkoff; // the tasks of a record, which the caller bisects by allele: the documents' tasks must ascend by allele
	bool t_rec, t_al, t_col;
	bool t_ph;   // (task_phase must be present)
	bool colmap; // per column of A, then of B: its common sample, or NO_QUERY
};
// The host arrays of a pair, and their way to the device
struct PairUpload {
	const povu_hip_vcf_doc *da = nullptr, *db = nullptr;
	uint32_t nRa = 0, nR = 0, nAl = 0, nT = 0, nI = 0, nIa = 0, n_chroms = 0, nC = 0, n_cols_a = 0, n_cols = 0, max_phase = 0;
	uint64_t n_text = 0, longest = 0; // text bytes; the longest text of a REF or a counted ALT
	std::vector<uint32_t> aoff, ioff, chrom;       // [nR + 1], [nR + 1], [nR]
	std::vector<uint64_t> toff, pos;	       // [nAl + 1], [nR]
	std::vector<uint32_t> tkoff;		       // [nR + 1]
	std::vector<uint32_t> t_rec, t_al, t_col, t_ph; // [nT] the record over both documents; allele, column and phase as the document has them
	std::vector<uint32_t> col_a, col_b, colmap;    // [nC] the columns of a common sample; [n_cols + 1]
	std::vector<std::string> chrom_name;	       // [n_chroms]
	hipStream_t s = nullptr;		       // (set by the caller before the first `up`)
	void up(void *dst, const void *src, size_t bytes) const
	{
		if (bytes)
			HIP_CHECK(copy_async(dst, src, bytes, hipMemcpyHostToDevice, s));
	}
	template <class T>
	void up(T *dst, const std::vector<T> &v) const { up(dst, v.data(), v.size() * sizeof(T)); }
	// A's text, then B's
	void up_text(char *dst) const { up(dst, da->text, da->n_text_bytes), up(dst + da->n_text_bytes, db->text, db->n_text_bytes); }
};
// What both calls do before their first launch: null context or documents and counts that do not fit 32 bits are refused in
// the caller's words (`who`: "the ... needs "), both documents verified (check_pair_doc) and laid end to end, the items
// counted, the samples matched by name.  pos_limit > 0: a POS of that or more is refused
PairUpload pair_build(const povu_hip_ctx *ctx, const povu_hip_vcf_doc *da, const povu_hip_vcf_doc *db, const char *who, const PairWant &want,
		      uint64_t pos_limit = 0);

// The arrays of a result in one page-locked block: `take(dev, n, size)` gives room for `size` elements and copies the first n
// from the device.  Declared once as a list and run twice, as Spans: to measure (no base), then to place and copy.  One
// block, because the context's pool keeps a bounded number of blocks whatever their size: thirty arrays a call would push
// each other out of it and be page-locked again on the next call
struct HostSpans {
	uint8_t *base = nullptr; // null: measure only
	hipStream_t s = nullptr;
	size_t bytes = 0;
	template <typename T>
	T *operator()(const T *dev, size_t n, size_t size)
	{
		const size_t at = bytes;
		bytes += (size * sizeof(T) + 63) & ~size_t(63);
		if (!base)
			return nullptr;
		T *h = reinterpret_cast<T *>(base + at);
		if (n)
			HIP_CHECK(copy_async(h, dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
		return h;
	}
};
// `results` run twice over `block`, sized between the runs from the context's pool
template <class List>
void hand_off_block(PinnedVec<uint8_t> &block, povu_hip_ctx *ctx, List &&results)
{
	HostSpans measure;
	results(measure);
	block.resize(measure.bytes, ctx->pool);
	HostSpans filled{block.data(), ctx->stream};
	results(filled);
}

} // namespace povu_hip
