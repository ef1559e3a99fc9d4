// modes_check.cpp -- the modes of a call (hip/call_modes.hpp) on the CPU, built with -fsanitize=address,undefined (make modes_check;
// run by tests/test_call_modes.py): all 2^7 * 5 requests through the table against the exclusions restated here, every exclusion
// found from either mode of its pair, no message without a rule, and the two texts of every rule against literal strings of
// their own here, which pin the wording.  With `--table` it prints the first refusal of both sides for every request;
// tests/test_call_modes.py compares that with the recorded answers of tests/golden/call_modes.json.
#include "../hip/call_modes.hpp"
#include "../hip/span_rules.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace md = modes;

#define CHECK(cond)                                                                         \
	do {                                                                                \
		if (!(cond)) {                                                              \
			fprintf(stderr, "modes_check: %s failed (line %d)\n", #cond, __LINE__); \
			abort();                                                            \
		}                                                                           \
	} while (0)

static const char *const NAME[] = {"raw-graph", "top-level-only", "popped", "left-normalized", "decomposed"};

// the texts as they were written, by rule in the library's order; a text in two halves has the profile's name between them
struct Pinned {
	const char *lib, *lib_tail, *cli, *cli_tail;
};
static const Pinned PINNED[] = {
	{"POVU_HIP_T_OFFREF (off-reference calls) is refused together with POVU_HIP_T_NESTED", nullptr, "Flag '--off-reference' cannot be combined with --nested",
	 nullptr},
	{"POVU_HIP_T_OFFREF (off-reference calls) is refused together with POVU_HIP_T_MERGE", nullptr,
	 "Flag '--off-reference' cannot be combined with --merge-primitives", nullptr},
	{"POVU_HIP_T_OFFREF (off-reference calls) is refused with profile ", ": only raw-graph", "Flag '--off-reference' is called under --profile raw-graph alone",
	 nullptr},
	{"POVU_HIP_T_UNTANGLE (untangled calls) is refused together with POVU_HIP_T_NESTED", nullptr, "Flag '--untangle' cannot be combined with --nested", nullptr},
	{"POVU_HIP_T_UNTANGLE (untangled calls) is refused together with POVU_HIP_T_MERGE", nullptr, "Flag '--untangle' cannot be combined with --merge-primitives",
	 nullptr},
	{"POVU_HIP_T_UNTANGLE (untangled calls) is refused together with POVU_HIP_T_OFFREF", nullptr, "Flag '--untangle' cannot be combined with --off-reference",
	 nullptr},
	{"POVU_HIP_T_UNTANGLE (untangled calls) is refused with profile ", ": only raw-graph", "Flag '--untangle' is called under --profile raw-graph alone", nullptr},
	{"POVU_HIP_T_MERGE merges the rows of the decomposed profile: refused with profile ", "",
	 "Flag '--merge-primitives' merges the rows of --profile decomposed and needs that profile", nullptr},
	{"a clustered call (povu_hip_call_clustered) is refused together with POVU_HIP_T_NESTED and the profiles that imply it", nullptr,
	 "Flag '--cluster' cannot be combined with --nested", nullptr},
	{"a clustered call (povu_hip_call_clustered) is refused with profile ", "", "Flag '--cluster' is called under --profile raw-graph alone, not ", ""},
	{"a clustered call (povu_hip_call_clustered) is refused together with POVU_HIP_T_MERGE", nullptr, "Flag '--cluster' cannot be combined with --merge-primitives",
	 nullptr},
	{"a clustered call (povu_hip_call_clustered) is refused together with POVU_HIP_T_OFFREF", nullptr, "Flag '--cluster' cannot be combined with --off-reference",
	 nullptr},
	{"a clustered call (povu_hip_call_clustered) is refused together with POVU_HIP_T_UNTANGLE", nullptr, "Flag '--cluster' cannot be combined with --untangle",
	 nullptr},
	{"regions (povu_hip_call_restricted) are refused together with POVU_HIP_T_OFFREF: an off-reference site has no locus on a region's path", nullptr,
	 "Flag '--region' cannot be combined with --off-reference", nullptr},
};

// the exclusions restated (include/povu_hip.h says them in prose): the pairs of modes, and what a mode asks of the profile
static const md::Mode PAIR[][2] = {{md::OFFREF, md::NESTED},   {md::OFFREF, md::MERGE},	  {md::UNTANGLE, md::NESTED}, {md::UNTANGLE, md::MERGE},
				   {md::UNTANGLE, md::OFFREF}, {md::CLUSTER, md::NESTED}, {md::CLUSTER, md::MERGE},   {md::CLUSTER, md::OFFREF},
				   {md::CLUSTER, md::UNTANGLE}, {md::REGIONS, md::OFFREF}};
static bool has(uint32_t set, md::Mode m) { return set >> m & 1u; }
static bool excluded(uint32_t set, uint32_t profile)
{
	for (auto &p : PAIR)
		if (has(set, p[0]) && has(set, p[1]))
			return true;
	if ((has(set, md::OFFREF) || has(set, md::UNTANGLE) || has(set, md::CLUSTER)) && profile != POVU_HIP_PROFILE_RAW_GRAPH)
		return true;
	return has(set, md::MERGE) && profile != POVU_HIP_PROFILE_DECOMPOSED;
}

static std::string pinned(const char *head, const char *tail, uint32_t profile) { return tail ? std::string(head) + NAME[profile] + tail : head; }

int main(int argc, char **argv)
{
	CHECK(md::N_MODES == 7 && md::N_PROFILES == 5 && md::N_RULES == sizeof PINNED / sizeof PINNED[0]);
	for (uint32_t p = 0; p < md::N_PROFILES; p++)
		CHECK(!strcmp(md::PROFILE_NAME[p], NAME[p]));
	// the command line's order is the same rules in another order
	uint32_t seen = 0;
	for (uint32_t k = 0; k < md::N_RULES; k++) {
		CHECK(md::CLI_ORDER[k] < md::N_RULES && !(seen >> md::CLI_ORDER[k] & 1u));
		seen |= 1u << md::CLI_ORDER[k];
	}
	// a refusal is thrown at its rule's stage among the library's other checks: the first rule is the first thrown only if the
	// stages do not go back along the library's order
	for (uint32_t k = 1; k < md::N_RULES; k++)
		CHECK(md::RULES[k - 1].stage <= md::RULES[k].stage);
	// the modes: the flags are distinct bits and set_of reads them back
	for (uint32_t m = 0; m < md::N_MODES; m++) {
		const uint32_t f = md::MODE[m].t_flag;
		CHECK((f == 0) == (m == md::REGIONS || m == md::CLUSTER) && !(f & (f - 1)));
		CHECK(md::set_of(f, m == md::REGIONS, m == md::CLUSTER) == 1u << m);
	}
	CHECK(md::set_of(POVU_HIP_T_FORCE_TIER2, false, false) == 0 && md::set_of(~0u, true, true) == (1u << md::N_MODES) - 1);
	// every rule: both texts are the pinned ones under every profile it can meet, and each names its mode
	for (uint32_t k = 0; k < md::N_RULES; k++) {
		const md::Rule &r = md::RULES[k];
		for (uint32_t p = 0; p < md::N_PROFILES; p++) {
			CHECK(md::message(r, md::LIBRARY, p) == pinned(PINNED[k].lib, PINNED[k].lib_tail, p));
			CHECK(md::message(r, md::COMMAND_LINE, p) == pinned(PINNED[k].cli, PINNED[k].cli_tail, p));
		}
		CHECK(strstr(r.lib, md::MODE[r.who].lib) && strstr(r.cli, md::MODE[r.who].cli));
		if (r.with == md::OTHER)
			CHECK(strstr(r.lib, md::MODE[r.other].lib) && strstr(r.cli, md::MODE[r.other].cli));
	}
	// every request: refused exactly when the restatement excludes it, on both sides alike, by a rule that applies
	const bool table = argc > 1 && !strcmp(argv[1], "--table");
	for (uint32_t p = 0; p < md::N_PROFILES; p++)
		for (uint32_t set = 0; set < 1u << md::N_MODES; set++) {
			const md::Rule *lib = md::refused(md::LIBRARY, set, p), *cli = md::refused(md::COMMAND_LINE, set, p);
			CHECK((lib != nullptr) == excluded(set, p) && (cli != nullptr) == excluded(set, p));
			CHECK(!lib || (md::applies(*lib, set, p) && md::applies(*cli, set, p)));
			if (table)
				printf("%u\t%u\t%s\t%s\n", set, p, lib ? md::message(*lib, md::LIBRARY, p).c_str() : "", cli ? md::message(*cli, md::COMMAND_LINE, p).c_str() : "");
		}
	// every exclusion is found from either mode of its pair: alone under a profile both accept, whichever mode the rule calls
	// `who`, a rule of exactly the two applies, and neither mode alone is refused there
	for (auto &pr : PAIR)
		for (int side = 0; side < 2; side++) {
			const md::Mode a = pr[side], b = pr[1 - side];
			const uint32_t p = a == md::MERGE || b == md::MERGE ? POVU_HIP_PROFILE_DECOMPOSED : POVU_HIP_PROFILE_RAW_GRAPH;
			const uint32_t set = 1u << a | 1u << b;
			uint32_t found = 0;
			for (const md::Rule &r : md::RULES)
				found += md::applies(r, set, p) && (r.with == md::OTHER || r.with == md::NESTED_OR_IMPLIED) &&
					 ((r.who == a && (r.with == md::OTHER ? r.other : md::NESTED) == b) || (r.who == b && (r.with == md::OTHER ? r.other : md::NESTED) == a));
			CHECK(found == 1 && md::refused(md::LIBRARY, set, p) && md::refused(md::COMMAND_LINE, set, p));
			CHECK(a == md::MERGE || b == md::MERGE || (!md::refused(md::LIBRARY, 1u << a, p) && !md::refused(md::COMMAND_LINE, 1u << b, p)));
		}
	// the order where two rules apply, as each side has always answered
	auto says = [](md::Side side, uint32_t set, uint32_t p, const char *text) {
		const md::Rule *r = md::refused(side, set, p);
		return r && md::message(*r, side, p) == text;
	};
	const uint32_t N = 1u << md::NESTED, M = 1u << md::MERGE, O = 1u << md::OFFREF, U = 1u << md::UNTANGLE, R = 1u << md::REGIONS, C = 1u << md::CLUSTER;
	CHECK(says(md::LIBRARY, O | U | N, 0, PINNED[0].lib) && says(md::COMMAND_LINE, O | U | N, 0, PINNED[0].cli));
	CHECK(says(md::LIBRARY, U | O | R, 0, PINNED[5].lib) && says(md::COMMAND_LINE, U | O | R, 0, PINNED[13].cli));
	CHECK(says(md::LIBRARY, C | N, 2, PINNED[8].lib) && says(md::COMMAND_LINE, C | N, 2, "Flag '--cluster' is called under --profile raw-graph alone, not popped"));
	CHECK(says(md::LIBRARY, C, 1, PINNED[8].lib) && says(md::LIBRARY, C, 3, "a clustered call (povu_hip_call_clustered) is refused with profile left-normalized"));
	CHECK(says(md::LIBRARY, C | M, 0, "POVU_HIP_T_MERGE merges the rows of the decomposed profile: refused with profile raw-graph") &&
	      says(md::COMMAND_LINE, C | M, 0, PINNED[10].cli) && says(md::COMMAND_LINE, C | M, 4, "Flag '--cluster' is called under --profile raw-graph alone, not decomposed"));
	CHECK(says(md::LIBRARY, C | O | R, 0, PINNED[11].lib) && says(md::COMMAND_LINE, M | O, 0, PINNED[7].cli) && says(md::LIBRARY, M | O, 0, PINNED[1].lib));
	// the spanning alleles are an option of the nested call and no line of the table (span_rules.hpp): POVU_HIP_T_SPANNING sets
	// no mode, and its own refusals name the flag on both sides, the rewriting profiles in front of "not nested"
	CHECK(md::set_of(POVU_HIP_T_SPANNING, false, false) == 0 && md::set_of(POVU_HIP_T_SPANNING | POVU_HIP_T_NESTED, false, false) == N);
	for (int cli = 0; cli < 2; cli++) {
		const char *flag = cli ? "'--spanning-alleles'" : "POVU_HIP_T_SPANNING";
		for (uint32_t p = 0; p < md::N_PROFILES; p++)
			for (int nested = 0; nested < 2; nested++) {
				const bool implied = nested || p == POVU_HIP_PROFILE_TOP_LEVEL_ONLY || p == POVU_HIP_PROFILE_POPPED;
				const char *why = povu_hip::span_refused(cli != 0, implied, p);
				const bool rewriting = p == POVU_HIP_PROFILE_LEFT_NORMALIZED || p == POVU_HIP_PROFILE_DECOMPOSED;
				CHECK((why != nullptr) == (rewriting || !implied));
				CHECK(!why || strstr(why, flag));
				CHECK(!why || !rewriting || strstr(why, md::PROFILE_NAME[p]));
			}
	}
	if (!table)
		puts("modes_check: ok");
	return 0;
}
