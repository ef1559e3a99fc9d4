// region_check.cpp -- the rules of the region calls (hip/region_rules.hpp) on the CPU, built with -fsanitize=address,undefined
// (make region_check; run by tests/test_region_cli.py): the parser's accepts and refusals, the normalisation and the interval
// search against a brute-force union on random intervals (the lists in arrays of exactly their number, so that a look outside
// them is an error here), and the step predicate at every off-by-one.
#include "../hip/region_rules.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>

namespace rg = region;

#define CHECK(cond)                                                                          \
	do {                                                                                 \
		if (!(cond)) {                                                               \
			fprintf(stderr, "region_check: %s failed (line %d)\n", #cond, __LINE__); \
			abort();                                                             \
		}                                                                            \
	} while (0)

static void accepts(const char *text, const char *name, uint64_t s, uint64_t e)
{
	std::string n;
	uint64_t a = 0, b = 0;
	const std::string err = rg::parse(text, n, a, b);
	if (!err.empty())
		fprintf(stderr, "region_check: %s\n", err.c_str());
	CHECK(err.empty() && n == name && a == s && b == e);
}
static void refuses(const char *text, const char *word)
{
	std::string n;
	uint64_t a = 0, b = 0;
	const std::string err = rg::parse(text, n, a, b);
	CHECK(!err.empty() && err.find(text) != std::string::npos && err.find(word) != std::string::npos);
}

int main()
{
	// ---- the parser
	accepts("chr20:31000000-32000000", "chr20", 31000000, 32000000);
	accepts("HG1#1#chr1:3-4", "HG1#1#chr1", 3, 4);
	accepts("a:b:1-2", "a:b", 1, 2); // the last ':'
	accepts("a-b:0-1", "a-b", 0, 1); // a '-' in the name
	accepts("x:1-999999999999999999", "x", 1, 999999999999999999ull);
	refuses("chr1", "no ':'");
	refuses(":1-2", "empty path name");
	refuses("chr1:12", "no '-'");
	refuses("chr1:1a-5", "start '1a'");
	refuses("chr1:1-5x", "end '5x'");
	refuses("chr1:-5", "start ''");
	refuses("chr1:1-", "end ''");
	refuses("chr1:1-2-3", "end '2-3'"); // the first '-' behind the ':'
	refuses("chr1:1-1000000000000000000", "18 digits");
	refuses("chr1:+1-5", "start '+1'");
	refuses("chr1:5-5", "below the end");
	refuses("chr1:9-3", "below the end");

	// ---- the predicate: a step of `len` bases behind `off` holds [off + 1, off + 1 + max(len, 1))
	for (uint64_t off : {0ull, 1ull, 7ull, 1000ull})
		for (uint64_t len : {0ull, 1ull, 2ull, 5ull}) {
			const uint64_t first = off + 1, last = first + (len ? len : 1);
			CHECK(!rg::step_in_region(off, len, first > 1 ? first - 1 : 0, first)); // e == off + 1: ends in front of it
			CHECK(rg::step_in_region(off, len, first > 1 ? first - 1 : 0, first + 1)); // ... and one behind
			CHECK(!rg::step_in_region(off, len, last, last + 3));		    // s == off + 1 + len: begins behind it
			CHECK(rg::step_in_region(off, len, last - 1, last + 3));	    // ... and one in front
			CHECK(rg::step_in_region(off, len, 0, rg::END_LIMIT - 1));
			if (len > 2)
				CHECK(rg::step_in_region(off, len, first + 1, first + 2)); // strictly inside
		}
	CHECK(rg::step_in_region(4, 0, 5, 6) && !rg::step_in_region(4, 0, 6, 7) && !rg::step_in_region(4, 0, 4, 5)); // no bases: one position

	// ---- normalisation and search against the brute-force union
	std::mt19937_64 rng(12345);
	for (int round = 0; round < 400; round++) {
		const uint32_t n = 1 + (uint32_t)(rng() % 40), n_paths = 1 + (uint32_t)(rng() % 4);
		const uint64_t span = 8 + rng() % 120;
		std::vector<rg::Region> r(n);
		for (auto &x : r) {
			x.path = (uint32_t)(rng() % n_paths);
			x.s = rng() % span;
			x.e = x.s + 1 + rng() % (round % 3 ? 6 : 40);
		}
		const rg::Normalised N = rg::normalise(r);
		CHECK(N.first.size() == N.path.size() + 1 && N.first.back() == N.s.size() && N.s.size() == N.e.size());
		for (size_t k = 0; k < N.path.size(); k++) {
			CHECK(k == 0 || N.path[k - 1] < N.path[k]);
			CHECK(N.first[k] < N.first[k + 1]);
			for (uint32_t i = N.first[k]; i < N.first[k + 1]; i++) {
				CHECK(N.s[i] < N.e[i]);
				CHECK(i == N.first[k] || N.e[i - 1] < N.s[i]); // neither overlapping nor touching
			}
		}
		for (uint32_t p = 0; p < n_paths; p++) {
			const size_t k = std::find(N.path.begin(), N.path.end(), p) - N.path.begin();
			const bool has = std::any_of(r.begin(), r.end(), [&](const rg::Region &x) { return x.path == p; });
			CHECK(has == (k < N.path.size()));
			if (!has)
				continue;
			// this path's list alone, in arrays of exactly its size
			const std::vector<uint64_t> s(N.s.begin() + N.first[k], N.s.begin() + N.first[k + 1]), e(N.e.begin() + N.first[k], N.e.begin() + N.first[k + 1]);
			for (uint64_t off = 0; off < span + 45; off++)
				for (uint64_t len : {0ull, 1ull, 3ull, 50ull}) {
					const bool brute = std::any_of(r.begin(), r.end(), [&](const rg::Region &x) { return x.path == p && rg::step_in_region(off, len, x.s, x.e); });
					CHECK(rg::step_in_any(s.data(), e.data(), 0, (uint32_t)s.size(), off, len) == brute);
				}
		}
	}
	const uint64_t one_s[1] = {5}, one_e[1] = {6};
	CHECK(!rg::step_in_any(one_s, one_e, 0, 0, 4, 1)); // an empty list
	puts("region_check: ok");
	return 0;
}
