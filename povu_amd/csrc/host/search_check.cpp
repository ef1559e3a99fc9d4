// search_check.cpp -- the binary searches of the device code (hip/search_rules.hpp) on the CPU, built with
// -fsanitize=address,undefined (make search_check; run by tests/test_search_rules.py).  The two primitives are held to
// std::partition_point on every 0/1-monotone predicate over short ranges, with both index types; the named forms to
// std::lower_bound / std::upper_bound on arrays with runs of equal keys; the midpoint on ranges that end at the top of the
// index type, where lo + hi wraps; span_of and the keys of the component view (CompSpans, common.hpp, which needs HIP: its
// two one-line keys are restated here) on offset tables with empty spans.
#include "../hip/search_rules.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

using namespace povu_hip;

#define REQUIRE(cond) \
	do { \
		if (!(cond)) { \
			fprintf(stderr, "search_check: %s failed (line %d)\n", #cond, __LINE__); \
			return 1; \
		} \
	} while (0)

// ---- every monotone predicate over [lo, lo + n), n = 0 .. 65: true on the first k indices.  The answer of the standard
// library is taken over the indices themselves; every probe must lie inside the range
template <class I> static int primitives_against_partition_point()
{
	for (I lo : {I(0), I(1), I(1000)})
		for (I n = 0; n <= 65; n++) {
			std::vector<I> idx(n);
			std::iota(idx.begin(), idx.end(), lo);
			const I hi = lo + n;
			for (I k = 0; k <= n; k++) {
				bool inside = true;
				auto holds = [&](I i) {
					inside = inside && i >= lo && i < hi;
					return i < lo + k;
				};
				const I want = lo + I(std::partition_point(idx.begin(), idx.end(), [&](I i) { return i < lo + k; }) - idx.begin());
				REQUIRE(first_not(lo, hi, holds) == want && inside);
				if (n >= 1 && k >= 1) // (upto(lo) holds: the last index of the true prefix)
					REQUIRE(last_upto(lo, hi, holds) == want - 1 && inside);
			}
		}
	return 0;
}

// ---- the named forms on arrays with runs of equal keys, from lo != 0 too: a key below all, above all, equal to each element
// and between the runs
static int named_forms_against_std()
{
	const std::vector<std::vector<uint32_t>> arrays = {{}, {5}, {5, 5, 5}, {2, 2, 4, 4, 4, 6, 8, 8, 10}, {1, 3, 3, 3, 3, 3, 3, 7, 9, 9, 9, 11, 11, 13, 20, 20, 20}};
	for (const auto &a : arrays)
		for (uint32_t lo = 0; lo <= a.size(); lo++)
			for (uint32_t hi = lo; hi <= a.size(); hi++)
				for (uint32_t x = 0; x <= 22; x++) {
					const uint32_t lb = (uint32_t)(std::lower_bound(a.begin() + lo, a.begin() + hi, x) - a.begin());
					const uint32_t ub = (uint32_t)(std::upper_bound(a.begin() + lo, a.begin() + hi, x) - a.begin());
					REQUIRE(lower_bound(a.data(), lo, hi, x) == lb);
					REQUIRE(upper_bound(a.data(), lo, hi, x) == ub);
				}
	// 64-bit keys under 32-bit indices and the reverse, as the kernels have them
	const std::vector<uint64_t> w = {1ull << 33, 1ull << 33, (1ull << 40) + 1, ~0ull};
	for (uint64_t x : std::vector<uint64_t>{0, 1ull << 33, (1ull << 33) + 1, (1ull << 40) + 1, ~0ull}) {
		REQUIRE(lower_bound(w.data(), 0u, 4u, x) == (uint32_t)(std::lower_bound(w.begin(), w.end(), x) - w.begin()));
		REQUIRE(upper_bound(w.data(), uint64_t(1), uint64_t(4), x) == (uint64_t)(std::upper_bound(w.begin() + 1, w.end(), x) - w.begin()));
	}
	return 0;
}

// ---- the midpoint: a range that ends at the top of the index type, a predicate on the index alone.  (lo + hi) >> 1 wraps
// there and probes far below lo
template <class I> static int midpoint_does_not_wrap()
{
	const I top = ~I(0), lo = top - 0xFF, hi = top; // 32 bits: [0xFFFFFF00, 0xFFFFFFFF)
	for (I k = 0; k <= hi - lo; k++) {
		bool inside = true;
		auto holds = [&](I i) {
			if (i < lo || i >= hi) { // (a helper that leaves the range may never come back: stop here, not in a time limit)
				fprintf(stderr, "search_check: a probe outside the range at the top of the index type\n");
				exit(1);
			}
			return i < lo + k;
		};
		const I f = first_not(lo, hi, holds);
		REQUIRE(inside && f == lo + k && f >= lo && f <= hi);
		if (k >= 1) {
			const I l = last_upto(lo, hi, holds);
			REQUIRE(inside && l == lo + k - 1 && l >= lo && l < hi);
		}
	}
	return 0;
}

// ---- offset tables with empty spans (equal neighbouring offsets), several at the front and at the end: the owner of a
// position is the last span that starts at or before it
template <class Key> static uint32_t last_at_or_before(uint32_t n, uint64_t x, Key &&key)
{
	uint32_t at = 0;
	for (uint32_t c = 0; c < n; c++)
		if (key(c) <= x)
			at = c;
	return at;
}
static int owners_in_offset_tables()
{
	const std::vector<std::vector<uint32_t>> tables = {{0}, {0, 0, 0}, {0, 0, 0, 3, 3, 7, 8, 8, 8, 12, 12, 12}, {0, 4, 4, 4, 9, 10, 10}, {0, 1, 2, 3}};
	for (const auto &off : tables) {
		const uint32_t n = (uint32_t)off.size();
		const std::vector<uint64_t> off64(off.begin(), off.end());
		for (uint32_t x = 0; x <= 2 * off.back() + n + 2; x++) {
			REQUIRE(span_of(off.data(), n, x) == last_at_or_before(n, x, [&](uint32_t c) { return off[c]; }));
			REQUIRE(span_of(off64.data(), n, x) == span_of(off.data(), n, x));
			// the component view: a tree vertex is keyed by 2 voff[c] + c, a slot by voff[c] + c
			const uint32_t *voff = off.data();
			REQUIRE(last_upto(0u, n, [=](uint32_t c) { return 2 * voff[c] + c <= x; }) == last_at_or_before(n, x, [&](uint32_t c) { return 2 * off[c] + c; }));
			REQUIRE(last_upto(0u, n, [=](uint32_t c) { return voff[c] + c <= x; }) == last_at_or_before(n, x, [&](uint32_t c) { return off[c] + c; }));
		}
	}
	return 0;
}

int main()
{
	if (primitives_against_partition_point<uint32_t>() || primitives_against_partition_point<uint64_t>())
		return 1;
	if (named_forms_against_std())
		return 1;
	if (midpoint_does_not_wrap<uint32_t>() || midpoint_does_not_wrap<uint64_t>())
		return 1;
	if (owners_in_offset_tables())
		return 1;
	printf("search_check: ok\n");
	return 0;
}
