// vcfcmp_rules.hpp -- the rules of the VCF comparison (INTEGRATION.md "VCF comparison"; restated in tests/vcfcmp_ref.py) that
// are plain arithmetic: which (record, ALT) is skipped, the case fold, how many bytes the two trims take at either end of REF
// and ALT, when two trimmed keys are equal, the hash of a key and the class of a (group, sample) cell from its two doses.
// Free of HIP, the wave's loops included ("a wave at a time" below): the tier kernels of vcf_pair.hpp run them per lane and
// per wave for the VCF comparison and for the haplotype comparison; host/vcfcheck.cpp writes the texts with them;
// host/vcfcmp_check.cpp and host/vcfhap_check.cpp run the same text on the CPU under the sanitizers, over an emulated wave.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define VCFCMP_FN __host__ __device__ inline
#else
#define VCFCMP_FN inline
#endif

namespace povu_hip
{

// ---- the skip rule.  The head of it reads at most one byte of either text; a `[` or `]` anywhere in ALT skips too
VCFCMP_FN bool vm_skip_head(const char *ref, uint64_t nr, const char *alt, uint64_t na)
{
	if (nr == 0 || (nr == 1 && ref[0] == '.'))
		return true;
	return na && (alt[0] == '<' || (na == 1 && alt[0] == '*'));
}
VCFCMP_FN bool vm_skip_byte(char c) { return c == '[' || c == ']'; }
VCFCMP_FN bool vm_skipped(const char *ref, uint64_t nr, const char *alt, uint64_t na)
{
	bool skip = vm_skip_head(ref, nr, alt, na);
	for (uint64_t i = 0; !skip && i < na; i++)
		skip = vm_skip_byte(alt[i]);
	return skip;
}

// ---- the key.  Letters are folded to upper case
VCFCMP_FN uint8_t vm_fold(char c) { return (uint8_t)(c >= 'a' && c <= 'z' ? c - 'a' + 'A' : c); }

// The trims, suffix first: at most `limit` bytes go, so that both texts keep a byte; byte i counted from the end (suffix) or
// from the front (prefix, of the texts the suffix trim left) goes while it is the same in both
VCFCMP_FN uint64_t vm_trim_limit(uint64_t nr, uint64_t na) { return (nr < na ? nr : na) ? (nr < na ? nr : na) - 1 : 0; }
VCFCMP_FN bool vm_suffix_differs(const char *ref, uint64_t nr, const char *alt, uint64_t na, uint64_t i)
{
	return vm_fold(ref[nr - 1 - i]) != vm_fold(alt[na - 1 - i]);
}
VCFCMP_FN bool vm_prefix_differs(const char *ref, const char *alt, uint64_t i) { return vm_fold(ref[i]) != vm_fold(alt[i]); }
// (under any limit: the haplotype comparison's lets a text become empty)
VCFCMP_FN uint64_t vm_suffix_upto(const char *ref, uint64_t nr, const char *alt, uint64_t na, uint64_t limit)
{
	uint64_t s = 0;
	while (s < limit && !vm_suffix_differs(ref, nr, alt, na, s))
		s++;
	return s;
}
VCFCMP_FN uint64_t vm_prefix_upto(const char *ref, const char *alt, uint64_t limit)
{
	uint64_t p = 0;
	while (p < limit && !vm_prefix_differs(ref, alt, p))
		p++;
	return p;
}
VCFCMP_FN uint64_t vm_suffix(const char *ref, uint64_t nr, const char *alt, uint64_t na)
{
	return vm_suffix_upto(ref, nr, alt, na, vm_trim_limit(nr, na));
}
// (nr, na: the lengths before the suffix trim took s bytes)
VCFCMP_FN uint64_t vm_prefix(const char *ref, uint64_t nr, const char *alt, uint64_t na, uint64_t s)
{
	return vm_prefix_upto(ref, alt, vm_trim_limit(nr - s, na - s));
}

// two trimmed keys of one CHROM are equal: POS', both lengths, the folded bytes
VCFCMP_FN bool vm_same_key(uint64_t pos_a, const char *ref_a, uint64_t nr_a, const char *alt_a, uint64_t na_a, uint64_t pos_b, const char *ref_b,
			   uint64_t nr_b, const char *alt_b, uint64_t na_b)
{
	if (pos_a != pos_b || nr_a != nr_b || na_a != na_b)
		return false;
	for (uint64_t i = 0; i < nr_a; i++)
		if (vm_fold(ref_a[i]) != vm_fold(ref_b[i]))
			return false;
	for (uint64_t i = 0; i < na_a; i++)
		if (vm_fold(alt_a[i]) != vm_fold(alt_b[i]))
			return false;
	return true;
}

// ---- the hash of a key, a function of the key alone.  A text hashes to the polynomial sum of (byte + 1) * VM_BASE^i over its
// folded bytes, modulo 2^64: a sum, so lanes may take the terms in any split and add
static constexpr uint64_t VM_BASE = 0x9E3779B97F4A7C15ull; // (odd)
VCFCMP_FN uint64_t vm_pow(uint64_t e)
{
	uint64_t r = 1, b = VM_BASE;
	for (; e; e >>= 1, b *= b)
		if (e & 1)
			r *= b;
	return r;
}
VCFCMP_FN uint64_t vm_term(char c, uint64_t power) { return ((uint64_t)vm_fold(c) + 1) * power; }
VCFCMP_FN uint64_t vm_text_hash(const char *t, uint64_t n)
{
	uint64_t h = 0, p = 1;
	for (uint64_t i = 0; i < n; i++, p *= VM_BASE)
		h += vm_term(t[i], p);
	return h;
}
VCFCMP_FN uint64_t vm_mix64(uint64_t x) // splitmix64's finaliser (mix64 of exact_groups.hpp)
{
	x ^= x >> 30;
	x *= 0xbf58476d1ce4e5b9ull;
	x ^= x >> 27;
	x *= 0x94d049bb133111ebull;
	x ^= x >> 31;
	return x;
}
// POS', both trimmed lengths and both text hashes
VCFCMP_FN uint64_t vm_key_hash(uint64_t pos, uint64_t nr, uint64_t na, uint64_t ref_hash, uint64_t alt_hash)
{
	uint64_t h = vm_mix64(pos ^ 0x243F6A8885A308D3ull);
	h = vm_mix64(h ^ (nr << 32) ^ na);
	h = vm_mix64(h ^ ref_hash);
	return vm_mix64(h + alt_hash);
}

// ---- a wave at a time: the skip rule's scan, both trims and the text hash with 64 lanes across the bytes.  `w` is the wave:
// w.ballot(f) gives the 64-bit mask of the lanes l for which f(l) holds, w.sum(f) the sum of f(l) over the lanes.  On the
// device w holds the calling lane and every lane of the wave makes the same calls (LaneWave of vcf_pair.hpp: __ballot and
// wave_sum); the check programs loop l over 0 .. 63 (host/wave_emu.hpp).  The bounds (`limit`, `n`) belong to the item and
// the item to the wave, so the trip counts are wave-uniform and every ballot and shuffle runs with all 64 lanes.
// The first index below `limit` at which pred holds, else `limit`: 64 a chunk, to the first ballot that is not empty
template <class W, class Pred>
VCFCMP_FN uint64_t wave_first(uint64_t limit, const W &w, Pred &&pred)
{
	for (uint64_t c0 = 0; c0 < limit; c0 += 64) {
		const uint64_t m = w.ballot([&](uint32_t l) { return c0 + l < limit && pred(c0 + l); });
		if (m)
			return c0 + (uint64_t)__builtin_ctzll(m);
	}
	return limit;
}
template <class W>
VCFCMP_FN bool wave_skipped(const char *ref, uint64_t nr, const char *alt, uint64_t na, const W &w)
{
	return vm_skip_head(ref, nr, alt, na) || wave_first(na, w, [&](uint64_t i) { return vm_skip_byte(alt[i]); }) != na;
}
// (limit_of: vm_trim_limit, or the haplotype comparison's vh_trim_limit)
template <class W, class Limit>
VCFCMP_FN uint64_t wave_suffix(const char *ref, uint64_t nr, const char *alt, uint64_t na, Limit &&limit_of, const W &w)
{
	return wave_first(limit_of(nr, na), w, [&](uint64_t i) { return vm_suffix_differs(ref, nr, alt, na, i); });
}
template <class W, class Limit>
VCFCMP_FN uint64_t wave_prefix(const char *ref, uint64_t nr, const char *alt, uint64_t na, uint64_t s, Limit &&limit_of, const W &w)
{
	return wave_first(limit_of(nr - s, na - s), w, [&](uint64_t i) { return vm_prefix_differs(ref, alt, i); });
}
// vm_text_hash of t[0, n): lane l sums the terms l, l + 64, ...
template <class W>
VCFCMP_FN uint64_t wave_text_hash(const char *t, uint64_t n, const W &w)
{
	const uint64_t stride = vm_pow(64);
	return w.sum([&](uint32_t l) {
		uint64_t h = 0, power = vm_pow(l);
		for (uint64_t x = l; x < n; x += 64, power *= stride)
			h += vm_term(t[x], power);
		return h;
	});
}

// ---- the class of a (group, common sample) cell from the doses of both sides
enum { VM_CELL_NONE = 0, VM_CELL_TP = 1, VM_CELL_FP = 2, VM_CELL_FN = 3 };
VCFCMP_FN int vm_cell(uint32_t dose_a, uint32_t dose_b)
{
	return dose_a ? (dose_b ? VM_CELL_TP : VM_CELL_FP) : (dose_b ? VM_CELL_FN : VM_CELL_NONE);
}
VCFCMP_FN bool vm_gteq(uint32_t dose_a, uint32_t dose_b) { return dose_a && dose_a == dose_b; }

// the class of a group from its member counts (POVU_HIP_M_SHARED, _ONLY_A, _ONLY_B of include/povu_hip.h)
VCFCMP_FN uint8_t vm_group_class(uint32_t n_a, uint32_t n_b) { return n_a && n_b ? 0 : n_a ? 1 : 2; }

} // namespace povu_hip
