// span_check.cpp -- the rules of the spanning alleles (hip/span_rules.hpp) on the CPU, built with -fsanitize=address,undefined
// (make span_check; run by tests/test_span_ref.py).  Hand-made chains of records go through span_entry, the walk of the
// definition, and through the rounds of k_ns_span with a loop over the lanes where the device has a wave: the ancestors' rows
// 64 a round, the slots 64 a round, a ballot word per slot round.  Both must agree on every (record, slot); the numbering and
// the counts are checked on the fixture's record by hand.
#include "../hip/span_rules.hpp"

#include <cstdio>
#include <vector>

using namespace povu_hip;

#define REQUIRE(cond) \
	do { \
		if (!(cond)) { \
			fprintf(stderr, "span_check: %s failed (line %d)\n", #cond, __LINE__); \
			return 1; \
		} \
	} while (0)

// records with parents, a site each (record r is of site r), S slots, the (site, slot) table's minima, the sites' status, the
// records' own slots
struct Chains {
	uint32_t S = 0;
	std::vector<uint32_t> parent, own;
	std::vector<uint8_t> status;
	std::vector<uint32_t> smin; // [records * S]
	uint32_t add(uint32_t par, uint32_t own_slot, uint8_t st = 0)
	{
		parent.push_back(par), own.push_back(own_slot), status.push_back(st);
		smin.resize(parent.size() * S, SPAN_SLOT_EMPTY);
		return (uint32_t)parent.size() - 1;
	}
	void cross(uint32_t r, uint32_t sl, uint32_t allele = 0) { smin[(size_t)r * S + sl] = allele; }
	bool empty(uint32_t r, uint32_t sl) const { return span_slot_empty(smin[(size_t)r * S + sl]); }
};

// the definition
static bool by_walk(const Chains &c, uint32_t r, uint32_t sl)
{
	return span_entry(c.empty(r, sl), c.status[r], sl == c.own[r], r, [&](uint32_t x) { return c.parent[x]; }, [&](uint32_t x) { return !c.empty(x, sl); });
}
// the kernel's rounds: bits[w] of record r, one word per 64 slots
static std::vector<uint64_t> by_rounds(const Chains &c, uint32_t r, uint32_t *rounds_walked)
{
	const uint32_t S = c.S, W = (S + 63) / 64;
	std::vector<uint64_t> bits(W, 0);
	uint32_t row[64], n0 = 0, cur = r;
	for (; n0 < SPAN_ROUND && c.parent[cur] != SPAN_NO_RECORD; n0++)
		row[n0] = cur = c.parent[cur];
	const uint32_t cur64 = cur;
	*rounds_walked = n0 ? 1 : 0;
	for (uint32_t w = 0; w < W; w++) {
		bool need[64], hit[64];
		for (uint32_t lane = 0; lane < 64; lane++) {
			const uint32_t sl = w * 64 + lane;
			need[lane] = n0 && sl < S && span_candidate(c.empty(r, sl), c.status[r], sl == c.own[r]);
			hit[lane] = false;
		}
		uint32_t rr[64], n = n0, at = cur64;
		for (uint32_t k = 0; k < n0; k++)
			rr[k] = row[k];
		for (;;) {
			auto open = [&] {
				for (uint32_t lane = 0; lane < 64; lane++)
					if (need[lane] && !hit[lane])
						return true;
				return false;
			};
			for (uint32_t k = 0; k < n && open(); k++)
				for (uint32_t lane = 0; lane < 64; lane++)
					if (need[lane] && !hit[lane])
						hit[lane] = !c.empty(rr[k], w * 64 + lane);
			if (n < SPAN_ROUND || !open() || c.parent[at] == SPAN_NO_RECORD)
				break;
			for (n = 0; n < SPAN_ROUND && c.parent[at] != SPAN_NO_RECORD; n++)
				rr[n] = at = c.parent[at];
			++*rounds_walked;
		}
		for (uint32_t lane = 0; lane < 64; lane++)
			if (hit[lane])
				bits[w] |= 1ull << lane;
	}
	return bits;
}
static int agree(const Chains &c)
{
	for (uint32_t r = 0; r < c.parent.size(); r++) {
		uint32_t rounds = 0;
		const std::vector<uint64_t> bits = by_rounds(c, r, &rounds);
		for (uint32_t sl = 0; sl < c.S; sl++)
			REQUIRE(((bits[sl / 64] >> (sl % 64)) & 1u) == (by_walk(c, r, sl) ? 1u : 0u));
	}
	return 0;
}

static int self_check()
{
	REQUIRE(span_candidate(true, 0, false) && !span_candidate(false, 0, false) && !span_candidate(true, 1, false) && !span_candidate(true, 4, false) &&
		!span_candidate(true, 0, true));
	REQUIRE(span_rounds(0) == 0 && span_rounds(1) == 1 && span_rounds(64) == 1 && span_rounds(65) == 2 && span_rounds(130) == 3);
	REQUIRE(span_star_code(2) == 2 && span_n_alleles(2, true) == 3 && span_n_alleles(2, false) == 2);
	REQUIRE(span_gt_code(SPAN_GT_MISSING, true, 3) == 3 && span_gt_code(SPAN_GT_MISSING, false, 3) == SPAN_GT_MISSING && span_gt_code(1, true, 3) == 1);
	{ // depth 0: a record without a parent has no spanned entry, whatever its slots
		Chains c;
		c.S = 3;
		const uint32_t top = c.add(SPAN_NO_RECORD, 0);
		c.cross(top, 0);
		for (uint32_t sl = 0; sl < 3; sl++)
			REQUIRE(!by_walk(c, top, sl));
		REQUIRE(!agree(c));
	}
	{ // the fixture: slot 0 is the reference (own), slot 1 takes the deletion edge of the parent, slot 2 the child's ALT
		Chains c;
		c.S = 3;
		const uint32_t par = c.add(SPAN_NO_RECORD, 0), kid = c.add(par, 0);
		c.cross(par, 0), c.cross(par, 1, 1), c.cross(par, 2);
		c.cross(kid, 0), c.cross(kid, 2, 1);
		REQUIRE(!by_walk(c, kid, 0) && by_walk(c, kid, 1) && !by_walk(c, kid, 2));
		REQUIRE(!agree(c));
		// its numbering and counts: two classes, `*` is 2; GT 0 2 1, AC=1,1 AN=3 NS=3
		uint32_t gt[3] = {0, SPAN_GT_MISSING, 1}, ac[2] = {0, 0};
		for (uint32_t sl = 0; sl < 3; sl++)
			gt[sl] = span_gt_code(gt[sl], by_walk(c, kid, sl), 2);
		SpanCounts n;
		for (uint32_t sm = 0; sm < 3; sm++)
			span_count_sample(sm, sm + 1, [&](uint32_t sl) { return gt[sl]; }, ac, n);
		REQUIRE(gt[0] == 0 && gt[1] == 2 && gt[2] == 1 && ac[0] == 1 && ac[1] == 1 && n.an == 3 && n.ns == 3);
	}
	{ // the record's own slot is never spanned, although the table calls it empty and its ancestors cross it
		Chains c;
		c.S = 2;
		const uint32_t par = c.add(SPAN_NO_RECORD, 0), kid = c.add(par, 1);
		c.cross(par, 0), c.cross(par, 1);
		REQUIRE(!by_walk(c, kid, 1) && by_walk(c, kid, 0));
		REQUIRE(!agree(c));
	}
	{ // a truncated site: unknown stays missing; a slot with no path at the locus stays missing beside a spanned one
		Chains c;
		c.S = 4;
		const uint32_t par = c.add(SPAN_NO_RECORD, 0), cut = c.add(par, 0, 1), kid = c.add(par, 0);
		c.cross(par, 0), c.cross(par, 1);
		REQUIRE(!by_walk(c, cut, 1) && by_walk(c, kid, 1) && !by_walk(c, kid, 2) && !by_walk(c, kid, 3));
		REQUIRE(!agree(c));
	}
	// chains around and beyond a round of 64: the innermost record's slot is crossed at the outermost ancestor alone, over 130
	// slots (three slot rounds); two samples' slots of a sample counted once in NS
	for (uint32_t depth : {1u, 63u, 64u, 65u, 70u, 129u, 200u}) {
		Chains c;
		c.S = 130;
		uint32_t cur = c.add(SPAN_NO_RECORD, 0);
		c.cross(cur, 0);
		c.cross(cur, 1), c.cross(cur, 64), c.cross(cur, 129);
		for (uint32_t k = 0; k < depth; k++) {
			cur = c.add(cur, 0);
			c.cross(cur, 0);
			if (k == depth / 2)
				c.cross(cur, 77);
		}
		REQUIRE(by_walk(c, cur, 1) && by_walk(c, cur, 64) && by_walk(c, cur, 129) && !by_walk(c, cur, 2) && !by_walk(c, cur, 0));
		REQUIRE(by_walk(c, cur, 77) == (depth / 2 + 1 < depth));
		uint32_t rounds = 0;
		by_rounds(c, cur, &rounds);
		REQUIRE(rounds >= span_rounds(depth));
		REQUIRE(!agree(c));
	}
	{
		uint32_t ac[2] = {0, 0};
		SpanCounts n;
		const uint32_t gt[4] = {2, SPAN_GT_MISSING, SPAN_GT_MISSING, SPAN_GT_MISSING};
		span_count_sample(0, 2, [&](uint32_t sl) { return gt[sl]; }, ac, n);
		span_count_sample(2, 4, [&](uint32_t sl) { return gt[sl]; }, ac, n);
		REQUIRE(ac[0] == 0 && ac[1] == 1 && n.an == 1 && n.ns == 1);
	}
	return 0;
}

int main()
{
	if (self_check())
		return 1;
	printf("span_check: ok\n");
	return 0;
}
