// call_modes.hpp -- the modes of a variant call and which of them combine (INTEGRATION.md "Variant calls" and the sections of
// the modes), free of HIP: the profile names, the seven modes with the names the library's messages and the command line give
// them, the refusals as a list of rules with both texts each produces, and the one function that finds the first rule a
// request meets.  Included by call_kernels.hip (check_call_inputs), by host/call.cpp (parse_call_args), by host/vcf.cpp (the
// profile names) and by host/modes_check.cpp, which walks every request through it under the sanitizers.  A new mode is a line
// of MODE and its lines of RULES (each with the stage its refusal is thrown at) and CLI_ORDER.
#pragma once
#include "../../../include/povu_hip.h"

#include <cstdint>
#include <string>

namespace modes
{

// by POVU_HIP_PROFILE_*
static constexpr uint32_t N_PROFILES = POVU_HIP_PROFILE_DECOMPOSED + 1;
static const char *const PROFILE_NAME[N_PROFILES] = {"raw-graph", "top-level-only", "popped", "left-normalized", "decomposed"};

enum Mode : uint32_t { INVERSIONS, NESTED, MERGE, OFFREF, UNTANGLE, REGIONS, CLUSTER, N_MODES };
struct ModeNames {
	uint32_t t_flag; // its POVU_HIP_T_* bit; 0: given beside the flags (regions with n > 0, a cluster threshold above 0)
	const char *lib, *cli;
};
static const ModeNames MODE[N_MODES] = {
	{POVU_HIP_T_INVERSIONS, "POVU_HIP_T_INVERSIONS", "--inversions"},
	{POVU_HIP_T_NESTED, "POVU_HIP_T_NESTED", "--nested"},
	{POVU_HIP_T_MERGE, "POVU_HIP_T_MERGE", "--merge-primitives"},
	{POVU_HIP_T_OFFREF, "POVU_HIP_T_OFFREF", "--off-reference"},
	{POVU_HIP_T_UNTANGLE, "POVU_HIP_T_UNTANGLE", "--untangle"},
	{0, "povu_hip_call_restricted", "--region"},
	{0, "povu_hip_call_clustered", "--cluster"},
};
// the modes of a request as a set: bit m for Mode m
inline uint32_t set_of(uint32_t t_flags, bool regions, bool cluster)
{
	uint32_t set = (regions ? 1u << REGIONS : 0u) | (cluster ? 1u << CLUSTER : 0u);
	for (uint32_t m = 0; m < N_MODES; m++)
		if (t_flags & MODE[m].t_flag)
			set |= 1u << m;
	return set;
}

// what `who` is refused with
enum With : uint32_t {
	OTHER,		   // the mode `other`
	NOT_RAW,	   // a profile other than raw-graph
	NOT_DECOMPOSED,	   // a profile other than decomposed (`who` needs that one)
	NESTED_OR_IMPLIED, // NESTED, or a profile that implies it (top-level-only, popped)
};
// where check_call_inputs throws a rule's refusal among its other checks
enum Stage : uint32_t {
	AT_FLAGS,   // behind the unknown profile, in front of the limits of the decomposed profile
	AT_CLUSTER, // behind the checks of the cluster threshold and the cluster flags
	AT_END,	    // behind every other check of the inputs
};
// {profile} in a text stands for the name of the request's profile
struct Rule {
	Mode who;
	With with;
	Mode other; // (with OTHER)
	Stage stage;
	const char *lib, *cli;
};
#define POVU_CLUSTERED "a clustered call (povu_hip_call_clustered) is refused "
// in the order the library checks them
static const Rule RULES[] = {
	{OFFREF, OTHER, NESTED, AT_FLAGS, "POVU_HIP_T_OFFREF (off-reference calls) is refused together with POVU_HIP_T_NESTED",
	 "Flag '--off-reference' cannot be combined with --nested"},
	{OFFREF, OTHER, MERGE, AT_FLAGS, "POVU_HIP_T_OFFREF (off-reference calls) is refused together with POVU_HIP_T_MERGE",
	 "Flag '--off-reference' cannot be combined with --merge-primitives"},
	{OFFREF, NOT_RAW, OFFREF, AT_FLAGS, "POVU_HIP_T_OFFREF (off-reference calls) is refused with profile {profile}: only raw-graph",
	 "Flag '--off-reference' is called under --profile raw-graph alone"},
	{UNTANGLE, OTHER, NESTED, AT_FLAGS, "POVU_HIP_T_UNTANGLE (untangled calls) is refused together with POVU_HIP_T_NESTED",
	 "Flag '--untangle' cannot be combined with --nested"},
	{UNTANGLE, OTHER, MERGE, AT_FLAGS, "POVU_HIP_T_UNTANGLE (untangled calls) is refused together with POVU_HIP_T_MERGE",
	 "Flag '--untangle' cannot be combined with --merge-primitives"},
	{UNTANGLE, OTHER, OFFREF, AT_FLAGS, "POVU_HIP_T_UNTANGLE (untangled calls) is refused together with POVU_HIP_T_OFFREF",
	 "Flag '--untangle' cannot be combined with --off-reference"},
	{UNTANGLE, NOT_RAW, UNTANGLE, AT_FLAGS, "POVU_HIP_T_UNTANGLE (untangled calls) is refused with profile {profile}: only raw-graph",
	 "Flag '--untangle' is called under --profile raw-graph alone"},
	{MERGE, NOT_DECOMPOSED, MERGE, AT_FLAGS, "POVU_HIP_T_MERGE merges the rows of the decomposed profile: refused with profile {profile}",
	 "Flag '--merge-primitives' merges the rows of --profile decomposed and needs that profile"},
	// (clusters stand where a nested call's classes stand, and no rewriting profile reads them)
	{CLUSTER, NESTED_OR_IMPLIED, CLUSTER, AT_CLUSTER, POVU_CLUSTERED "together with POVU_HIP_T_NESTED and the profiles that imply it",
	 "Flag '--cluster' cannot be combined with --nested"},
	{CLUSTER, NOT_RAW, CLUSTER, AT_CLUSTER, POVU_CLUSTERED "with profile {profile}", "Flag '--cluster' is called under --profile raw-graph alone, not {profile}"},
	{CLUSTER, OTHER, MERGE, AT_CLUSTER, POVU_CLUSTERED "together with POVU_HIP_T_MERGE", "Flag '--cluster' cannot be combined with --merge-primitives"},
	{CLUSTER, OTHER, OFFREF, AT_CLUSTER, POVU_CLUSTERED "together with POVU_HIP_T_OFFREF", "Flag '--cluster' cannot be combined with --off-reference"},
	{CLUSTER, OTHER, UNTANGLE, AT_CLUSTER, POVU_CLUSTERED "together with POVU_HIP_T_UNTANGLE", "Flag '--cluster' cannot be combined with --untangle"},
	{REGIONS, OTHER, OFFREF, AT_END,
	 "regions (povu_hip_call_restricted) are refused together with POVU_HIP_T_OFFREF: an off-reference site has no locus on a region's path",
	 "Flag '--region' cannot be combined with --off-reference"},
};
#undef POVU_CLUSTERED
static constexpr uint32_t N_RULES = sizeof RULES / sizeof RULES[0];
// the order the command line checks them in: --cluster (its profile before --nested), --merge-primitives, --off-reference,
// --region, --untangle
static const uint8_t CLI_ORDER[N_RULES] = {9, 8, 10, 11, 12, 7, 0, 1, 2, 13, 3, 4, 5, 6};

enum Side : uint32_t { LIBRARY, COMMAND_LINE };

inline bool applies(const Rule &r, uint32_t set, uint32_t profile)
{
	if (!(set >> r.who & 1u))
		return false;
	switch (r.with) {
	case OTHER:
		return set >> r.other & 1u;
	case NOT_RAW:
		return profile != POVU_HIP_PROFILE_RAW_GRAPH;
	case NOT_DECOMPOSED:
		return profile != POVU_HIP_PROFILE_DECOMPOSED;
	default:
		return (set >> NESTED & 1u) || profile == POVU_HIP_PROFILE_TOP_LEVEL_ONLY || profile == POVU_HIP_PROFILE_POPPED;
	}
}
// the first rule, in the order of `side`, that refuses the modes `set` (set_of) under `profile` (a known one); NULL: none does
inline const Rule *refused(Side side, uint32_t set, uint32_t profile)
{
	for (uint32_t k = 0; k < N_RULES; k++) {
		const Rule &r = RULES[side == LIBRARY ? k : CLI_ORDER[k]];
		if (applies(r, set, profile))
			return &r;
	}
	return nullptr;
}
// the text of the refusal
inline std::string message(const Rule &r, Side side, uint32_t profile)
{
	std::string m = side == LIBRARY ? r.lib : r.cli;
	const size_t at = m.find("{profile}");
	if (at != std::string::npos)
		m.replace(at, 9, PROFILE_NAME[profile]);
	return m;
}

} // namespace modes
