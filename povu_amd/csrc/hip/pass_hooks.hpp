// pass_hooks.hpp -- the environment hooks of a decompose pass (A/B switches and tuning knobs of the tree and class stages):
// the one place that names them and reads the environment for them.  plan_pass reads them once per pass into
// PassPlan::hooks, so a test may switch them between the passes of one process and a reader of the plan sees which form
// ran.  Plain C++ (no HIP): the sanitizer check of the host code compiles it.  Every value is parsed with atoi.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace povu_hip
{

// bits of the class sort's payload that carry the list size in a black-only pass, at most (LszField, par_kernels.hpp)
static constexpr unsigned LSZ_FIELD_CAP = 8;
// sides a lane of the small class walk walks before it hands its class to the wave walk (tree_kernels.hip, class_walks)
static constexpr uint32_t CLASS_BUDGET = 256;

struct PassHooks {
	int wide_counts = 0;		     // POVU_HIP_WIDE_COUNTS: bracket counts as words -- 1 = all three, 2 = srccnt and incnt, 3 = incnt only
	int word_prefix = 0;		     // POVU_HIP_WORD_PREFIX: prefix sums as words, not count records -- 1 = both, 2 = psin, 3 = the range starts
	unsigned lsz_field = LSZ_FIELD_CAP; // POVU_HIP_LSZ_FIELD: lowers the cap of the payload's size field, 0 = the bare stack index
	uint32_t walk_route = 0;	     // POVU_HIP_WALK_ROUTE: the route both forms of the wave walk are given (k_class_walk_wave)
	unsigned dfs_blocks = 49152;	     // POVU_HIP_DFS_BLOCKS: workgroups of the small class walk at most, at least 1 (the default: measured, see class_walks)
	uint32_t class_budget = CLASS_BUDGET; // POVU_HIP_CLASS_BUDGET: that budget, at least 16
	bool rank_stats = false;	     // POVU_HIP_RANK_STATS (set at all): both rankings leave the statistics of their records
	// POVU_HIP_RANK_BITS: bucket bits of both rankings, 2..6.  3 = one element in 8 is a splitter (1 in 16 measured 0.2 ms slower
	// on 2.4e8 slots once the other kernels had changed; POVU_HIP_F_SPARSE_SPLITTERS still forces it)
	unsigned rank_bits = 3;
};

inline PassHooks read_pass_hooks()
{
	PassHooks h;
	if (const char *ev = getenv("POVU_HIP_WIDE_COUNTS"))
		h.wide_counts = atoi(ev);
	if (const char *ev = getenv("POVU_HIP_WORD_PREFIX"))
		h.word_prefix = atoi(ev);
	if (const char *ev = getenv("POVU_HIP_LSZ_FIELD"))
		h.lsz_field = (unsigned)std::min(std::max(atoi(ev), 0), (int)LSZ_FIELD_CAP);
	if (const char *ev = getenv("POVU_HIP_WALK_ROUTE"))
		h.walk_route = (uint32_t)atoi(ev);
	if (const char *ev = getenv("POVU_HIP_DFS_BLOCKS"))
		h.dfs_blocks = std::max(1u, (unsigned)atoi(ev)); // (the cap at the number of blocks there are: where the launch is sized)
	if (const char *ev = getenv("POVU_HIP_CLASS_BUDGET"))
		h.class_budget = (uint32_t)std::max(16, atoi(ev));
	h.rank_stats = getenv("POVU_HIP_RANK_STATS") != nullptr;
	if (const char *ev = getenv("POVU_HIP_RANK_BITS"))
		h.rank_bits = (unsigned)std::min(6, std::max(2, atoi(ev)));
	return h;
}

} // namespace povu_hip
