// region_rules.hpp -- the rules of the region calls (INTEGRATION.md "Region calls"; restated in tests/region_ref.py), everything
// of them that needs no memory space: the reading of `name:start-end`, whether a path step lies in a region, the regions of a
// call grouped by path with their intervals sorted and merged, and the search of a position range in such a merged list.
// Plain C++17: region_kernels.hip runs the search on the device, host/vcf.cpp and the call's host half the rest;
// host/region_check.cpp runs all of it under the sanitizers.
//
// A region (path, s, e) holds the 1-based positions [s, e) of the path.  Step k of the path holds the positions
// [off + 1, off + 1 + max(len, 1)), off the bases in front of it: a segment without bases counts as one position.
#pragma once
#include "prim_align.hpp"
#include "search_rules.hpp"

#include <algorithm>
#include <string>
#include <vector>

namespace region
{

constexpr uint64_t END_LIMIT = 1ull << 63; // e < 2^63
constexpr uint32_t MAX_REGIONS = 65536;
constexpr size_t MAX_DIGITS = 18;

// ---- the step-in-region predicate: the step's positions [first, first + max(len, 1)) meet [s, e)
PRIM_HD bool step_in_region(uint64_t off, uint64_t len, uint64_t s, uint64_t e)
{
	const uint64_t first = off + 1, last = first + (len ? len : 1); // (off + len < 2^63: the bases of a path)
	return first < e && s < last;
}

// ---- the interval search: does a step meet any of iv[lo, hi), sorted by s, disjoint and not touching (normalise)?  The
// one candidate is the last interval that begins in front of the step's end
PRIM_HD bool step_in_any(const uint64_t *iv_s, const uint64_t *iv_e, uint32_t lo, uint32_t hi, uint64_t off, uint64_t len)
{
	const uint64_t last = off + 1 + (len ? len : 1);
	const uint32_t at = povu_hip::lower_bound(iv_s, lo, hi, last); // the first interval with s >= last
	return at > lo && step_in_region(off, len, iv_s[at - 1], iv_e[at - 1]);
}

// ---- the parser: `name:start-end`, split at the last ':' and at the first '-' behind it.  Gives "" or the refusal
inline std::string parse(const std::string &text, std::string &name, uint64_t &s, uint64_t &e)
{
	const std::string what = "region '" + text + "'";
	const size_t colon = text.rfind(':');
	if (colon == std::string::npos)
		return what + " has no ':' (expected <path name>:<start>-<end>)";
	if (colon == 0)
		return what + " has an empty path name";
	const size_t dash = text.find('-', colon + 1);
	if (dash == std::string::npos)
		return what + " has no '-' behind the ':' (expected <path name>:<start>-<end>)";
	const std::string a = text.substr(colon + 1, dash - colon - 1), b = text.substr(dash + 1);
	auto number = [](const std::string &v) { return !v.empty() && v.size() <= MAX_DIGITS && std::all_of(v.begin(), v.end(), [](char c) { return c >= '0' && c <= '9'; }); };
	if (!number(a))
		return what + ": the start '" + a + "' is no number of at most 18 digits";
	if (!number(b))
		return what + ": the end '" + b + "' is no number of at most 18 digits";
	name = text.substr(0, colon);
	s = std::stoull(a), e = std::stoull(b);
	if (s >= e)
		return what + ": the start must be below the end (1-based start, exclusive end)";
	return "";
}

// ---- the regions of a call, normalised: the distinct paths ascending, per path [first[k], first[k + 1]) of the intervals,
// sorted, those that overlap or touch merged
struct Normalised {
	std::vector<uint32_t> path, first;
	std::vector<uint64_t> s, e;
};
struct Region {
	uint32_t path;
	uint64_t s, e;
};
inline Normalised normalise(std::vector<Region> r)
{
	std::sort(r.begin(), r.end(), [](const Region &a, const Region &b) { return a.path != b.path ? a.path < b.path : a.s != b.s ? a.s < b.s : a.e < b.e; });
	Normalised n;
	for (const Region &x : r) {
		if (n.path.empty() || n.path.back() != x.path) {
			n.path.push_back(x.path);
			n.first.push_back((uint32_t)n.s.size());
		} else if (x.s <= n.e.back()) {
			n.e.back() = std::max(n.e.back(), x.e);
			continue;
		}
		n.s.push_back(x.s), n.e.push_back(x.e);
	}
	n.first.push_back((uint32_t)n.s.size());
	return n;
}

} // namespace region
