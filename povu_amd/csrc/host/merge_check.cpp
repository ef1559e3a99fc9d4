// merge_check.cpp -- the votes of the merged primitives (hip/prim_merge.hpp) on the CPU, built with -fsanitize=address,undefined
// (make merge_check; run by tests/test_merge_core.py).  The rows of a record lie in arrays of exactly their number, as the
// device's lie in the arena, so that a look outside them is an error here.
//
// stdin: one member and its slots a line,
//   `A B K RULE N_ALTS  { P | W N (POS REF_LEN LEAD)*N }*N_ALTS  N_SLOTS G*N_SLOTS`
// [A, B] the span of the member's group, K its ALT, RULE 0 for a group that keeps the plain projection, then for every ALT of
// the record `P` (kept whole) or `W` and its N primitive rows (LEAD 0 or 1), then the allele every slot carries (65535: '.').
// stdout, per line: the vote of every slot (0 none, 1 reference, 2 this ALT, 3 reference because the slot's ALT lies
// elsewhere), then `|` and the value (0, 1, 255), the conflict flag and the reference-elsewhere flag of those votes taken
// together as one slot's.
#include "../hip/prim_merge.hpp"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace pm = prim_merge;

#define CHECK(cond)                                                                         \
	do {                                                                                \
		if (!(cond)) {                                                              \
			fprintf(stderr, "merge_check: %s failed (line %d)\n", #cond, __LINE__); \
			abort();                                                            \
		}                                                                           \
	} while (0)

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		if (line.empty())
			continue;
		std::istringstream is(line);
		unsigned long long a = 0, b = 0;
		uint32_t k = 0, rule = 0, n_alts = 0, n_slots = 0;
		if (!(is >> a >> b >> k >> rule >> n_alts) || a > b || !k || k > n_alts) {
			fprintf(stderr, "merge_check: bad line: %s\n", line.c_str());
			return 2;
		}
		std::vector<uint64_t> pos;
		std::vector<uint32_t> ref_len;
		std::vector<uint8_t> lead;
		std::vector<pm::OtherAlt> alt(n_alts);
		for (uint32_t x = 0; x < n_alts; x++) {
			std::string what;
			uint32_t n = 0;
			if (!(is >> what) || (what != "P" && what != "W") || (what == "W" && !(is >> n))) {
				fprintf(stderr, "merge_check: bad ALT %u: %s\n", x + 1, line.c_str());
				return 2;
			}
			alt[x] = {what == "W", pos.size(), pos.size() + n};
			for (uint32_t r = 0; r < n; r++) {
				unsigned long long p = 0;
				uint32_t len = 0, ld = 0;
				if (!(is >> p >> len >> ld) || len + ld == 0) {
					fprintf(stderr, "merge_check: bad row: %s\n", line.c_str());
					return 2;
				}
				// what the bisection relies on
				CHECK(r == 0 || (pos.back() <= p && pm::span_end(pos.back(), ref_len.back(), lead.back()) <= pm::span_end(p, len, (uint8_t)ld)));
				pos.push_back(p), ref_len.push_back(len), lead.push_back((uint8_t)ld);
			}
		}
		if (!(is >> n_slots)) {
			fprintf(stderr, "merge_check: no slots: %s\n", line.c_str());
			return 2;
		}
		// (exact sizes: the sanitizer sees a read behind the last row)
		pos.shrink_to_fit(), ref_len.shrink_to_fit(), lead.shrink_to_fit();
		const pm::Rows rows{pos.data(), ref_len.data(), lead.data()};
		pm::Tally tally;
		std::string out;
		for (uint32_t s = 0; s < n_slots; s++) {
			uint32_t g = 0;
			if (!(is >> g)) {
				fprintf(stderr, "merge_check: slot %u is missing: %s\n", s, line.c_str());
				return 2;
			}
			const uint32_t v = pm::vote(g, k, n_alts, rule != 0, rows, a, b, [&](uint32_t other) {
				CHECK(other >= 1 && other <= n_alts && other != k);
				return alt[other - 1];
			});
			pm::cast(tally, v);
			out += std::to_string(v) + " ";
		}
		printf("%s| %u %u %u\n", out.c_str(), (unsigned)pm::slot_value(tally), pm::conflict(tally) ? 1u : 0u, pm::ref_consistent(tally) ? 1u : 0u);
	}
	return 0;
}
