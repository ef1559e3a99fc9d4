// offref_rules.hpp -- the rules of the off-reference calls (INTEGRATION.md "Off-reference calls"; restated in
// tests/offref_ref.py) that are plain arithmetic: which site is a candidate, which child keeps its parent from being called
// off-reference, when one traversal encloses another on a path, and the key by which the tightest host wins.  Free of HIP:
// offref_kernels.hip runs them per lane, host/offref_check.cpp on the CPU under the sanitizers.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define OFFREF_FN __host__ __device__ inline
#else
#define OFFREF_FN inline
#endif

namespace povu_hip
{

// the families of the subflubble vertices
OFFREF_FN bool offref_is_subflubble(uint8_t f) { return f == 'T' || f == 'O' || f == 'C' || f == 'M' || f == 'S'; }
// a site (never the root: the root is no site) is a candidate when no subflubble vertex lies on its way to the root, itself
// included, the reference paths do not call it, and some path traverses it
OFFREF_FN bool offref_candidate(bool under_subflubble, bool callable, uint32_t n_traversals)
{
	return !under_subflubble && !callable && n_traversals > 0;
}
// the innermost rule: a child that is callable or a candidate takes "called off-reference" from its parent
OFFREF_FN bool offref_clears_parent(bool callable, bool candidate) { return callable || candidate; }

// the steps [f, l] of a path lie within [hf, hl], which is longer
OFFREF_FN bool offref_encloses(uint64_t hf, uint64_t hl, uint64_t f, uint64_t l) { return hf <= f && l <= hl && l - f < hl - hf; }
// the offer of a host traversal of `steps` steps of site q: the smallest key wins (fewest steps, then the lowest site)
OFFREF_FN uint64_t offref_host_key(uint32_t steps, uint32_t q) { return ((uint64_t)(steps - 1) << 32) | q; }
static constexpr uint64_t OFFREF_NO_HOST = ~0ull;
OFFREF_FN uint32_t offref_host_site(uint64_t key) { return (uint32_t)key; }

} // namespace povu_hip
