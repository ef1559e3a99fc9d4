// vcfcheck_rules.hpp -- the rules of the VCF checks (INTEGRATION.md "VCF checks"; restated in tests/vcfcheck_ref.py) that are
// plain arithmetic: how an AT walk is read, which step of a walk a search begins at and compares in either direction, and
// when a walk occurs at a position of one path -- entirely inside it.  Free of HIP: vcfcheck_kernels.hip runs them per lane,
// host/vcfcheck.cpp reads the walks with them, host/vcfcheck_check.cpp runs both on the CPU under the sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define VCFCHECK_FN __host__ __device__ inline
#else
#define VCFCHECK_FN inline
#endif

namespace povu_hip
{

// ---- the walk tokenizer.  A walk is `[<>]id` repeated, id a decimal number below 2^32 - 1
enum { VC_TOKEN_END = 0, VC_TOKEN_STEP = 1, VC_TOKEN_BAD = -1 };
// the step at s[*i] (VC_TOKEN_STEP: *id and *rev set, *i behind it), the end of the text, or a byte that begins no step
VCFCHECK_FN int vc_next_step(const char *s, size_t n, size_t *i, uint32_t *id, uint8_t *rev)
{
	if (*i >= n)
		return VC_TOKEN_END;
	const char c = s[*i];
	if (c != '>' && c != '<')
		return VC_TOKEN_BAD;
	size_t k = *i + 1;
	uint64_t v = 0;
	while (k < n && s[k] >= '0' && s[k] <= '9') {
		v = v * 10 + (uint64_t)(s[k] - '0');
		if (v >= 0xFFFFFFFFull)
			return VC_TOKEN_BAD;
		k++;
	}
	if (k == *i + 1)
		return VC_TOKEN_BAD; // no digit
	*id = (uint32_t)v;
	*rev = c == '<';
	*i = k;
	return VC_TOKEN_STEP;
}

// ---- the occurrence rule.  A walk w of m path words (vertex << 1 | '<') is searched forward as it stands and reverse as
// flip(w[m - 1]) .. flip(w[0]): step k of what is compared, and the step whose occurrences are the candidates
VCFCHECK_FN uint32_t vc_pattern_step(const uint32_t *w, uint32_t m, bool rev, uint32_t k) { return rev ? w[m - 1 - k] ^ 1u : w[k]; }
VCFCHECK_FN uint32_t vc_anchor(const uint32_t *w, uint32_t m, bool rev) { return vc_pattern_step(w, m, rev, 0); }
// m steps from global position g stay inside the path that ends in front of position path_end (g lies in that path)
VCFCHECK_FN bool vc_fits(uint64_t g, uint32_t m, uint64_t path_end) { return (uint64_t)m <= path_end - g; }
// steps [k0, k1) of the pattern stand at g + k0 .. of `steps` (the caller has checked vc_fits)
VCFCHECK_FN bool vc_equal_steps(const uint32_t *steps, uint64_t g, const uint32_t *w, uint32_t m, bool rev, uint32_t k0, uint32_t k1)
{
	for (uint32_t k = k0; k < k1; k++)
		if (steps[g + k] != vc_pattern_step(w, m, rev, k))
			return false;
	return true;
}
// the walk occurs at g, entirely inside its path
VCFCHECK_FN bool vc_occurs_at(const uint32_t *steps, uint64_t g, uint64_t path_end, const uint32_t *w, uint32_t m, bool rev)
{
	return vc_fits(g, m, path_end) && vc_equal_steps(steps, g, w, m, rev, 0, m);
}

// ---- the spanning allele `*` (VCF 4.2; INTEGRATION.md "Spanning alleles").  An allele spelled `*` is absent because of an
// overlapping event: it has no walk of its own, its AT entry is the one character `*` (read as a walk without steps, no bad
// step), and a genotype entry that names it is not searched and is never a failure
VCFCHECK_FN bool vc_star_text(const char *s, size_t n) { return n == 1 && s[0] == '*'; }
// the state of an allele (VC_AS_*; 0: its walk is searched).  `*` comes first: such an allele is not NO_AT for the walk it lacks
enum { VC_AS_NO_AT = 1, VC_AS_BAD_STEP = 2, VC_AS_STAR = 4 };
VCFCHECK_FN uint8_t vc_allele_state(bool has_text, const char *text, size_t n_text, bool has_walk, size_t n_steps, bool unknown_step)
{
	if (has_text && vc_star_text(text, n_text))
		return VC_AS_STAR;
	if (!has_walk || !n_steps)
		return VC_AS_NO_AT;
	return unknown_step ? VC_AS_BAD_STEP : 0;
}

// ---- the status of a task from what was found for its allele in its slot (POVU_HIP_V_* of include/povu_hip.h)
VCFCHECK_FN uint8_t vc_status(bool no_at, bool bad_step, bool no_slot, bool fwd, bool rev, bool forward_only)
{
	if (no_at)
		return 3; // POVU_HIP_V_NO_AT
	if (bad_step)
		return 4; // POVU_HIP_V_BAD_STEP
	if (no_slot)
		return 5; // POVU_HIP_V_NO_SLOT
	if (fwd)
		return 0; // POVU_HIP_V_FOUND_FWD
	if (rev && !forward_only)
		return 1; // POVU_HIP_V_FOUND_REV
	return 2;	  // POVU_HIP_V_ABSENT
}
// ... from the state of its allele (`has`: the record has the allele at all).  A task of a `*` allele reads found_fwd: there
// is nothing to find, and no other status is no failure
VCFCHECK_FN uint8_t vc_task_status(bool has, uint8_t astate, bool no_slot, bool fwd, bool rev, bool forward_only)
{
	if (has && (astate & VC_AS_STAR))
		return 0; // POVU_HIP_V_FOUND_FWD
	return vc_status(!has || (astate & VC_AS_NO_AT), has && (astate & VC_AS_BAD_STEP), no_slot, fwd, rev, forward_only);
}

} // namespace povu_hip
