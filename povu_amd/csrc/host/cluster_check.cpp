// cluster_check.cpp -- the rules of the clustered calls (hip/cluster_rules.hpp) on the CPU, built with -fsanitize=address,undefined
// (make cluster_check; run by tests/test_cluster_cli.py): the parser's accepts and refusals, similar / better / sim_ppm against
// __int128 arithmetic on random pairs and at weights whose products pass 2^64 (no graph of that size exists: they are tested
// here only), the weight bound against the true (I, U) of random bags, the ordinal rule against a counted multiset
// intersection, and the leader loop on the worked example and against a brute-force restatement (the bags in vectors of exactly
// their size, so that a look outside them is an error here).
#include "../hip/cluster_rules.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>

namespace cl = cluster;
using u128 = unsigned __int128;

#define CHECK(cond)                                                                           \
	do {                                                                                  \
		if (!(cond)) {                                                                \
			fprintf(stderr, "cluster_check: %s failed (line %d)\n", #cond, __LINE__); \
			abort();                                                              \
		}                                                                             \
	} while (0)

static void accepts(const char *text, uint32_t want)
{
	uint32_t ppm = 0;
	const std::string err = cl::parse(text, &ppm);
	if (!err.empty())
		fprintf(stderr, "cluster_check: %s\n", err.c_str());
	CHECK(err.empty() && ppm == want);
}
static void refuses(const char *text, const char *word)
{
	uint32_t ppm = 77;
	const std::string err = cl::parse(text, &ppm);
	CHECK(!err.empty() && ppm == 77 && err.find(std::string("'") + text + "'") != std::string::npos && err.find(word) != std::string::npos);
}

// the same three rules in the compiler's 128-bit arithmetic, which holds every product of two u64
static bool similar_ref(uint64_t I, uint64_t U, uint32_t T) { return U == 0 || (u128)I * cl::PPM >= (u128)T * U; }
static bool better_ref(uint64_t Ia, uint64_t Ua, uint64_t Ib, uint64_t Ub)
{
	if (!Ua)
		Ia = Ua = 1;
	if (!Ub)
		Ib = Ub = 1;
	return (u128)Ia * Ub > (u128)Ib * Ua;
}
static uint32_t ppm_ref(uint64_t I, uint64_t U) { return U == 0 ? cl::PPM : (uint32_t)((u128)I * cl::PPM / U); }

static cl::Bag make_bag(std::vector<uint32_t> keys, const std::vector<uint64_t> &weight)
{
	std::sort(keys.begin(), keys.end());
	cl::Bag b;
	b.key = keys;
	for (uint32_t k : keys)
		b.w.push_back(weight[k]);
	return b;
}
// I and U by counting
static cl::Frac counted(const cl::Bag &a, const cl::Bag &b, const std::vector<uint64_t> &weight)
{
	std::map<uint32_t, uint32_t> ca, cb;
	for (uint32_t k : a.key)
		ca[k]++;
	for (uint32_t k : b.key)
		cb[k]++;
	uint64_t I = 0;
	for (auto &[k, n] : ca)
		I += (uint64_t)std::min(n, cb.count(k) ? cb[k] : 0u) * weight[k];
	return cl::Frac{I, a.W() + b.W() - I};
}

int main()
{
	// ---- the parser
	accepts("1", 1000000);
	accepts("1.0", 1000000);
	accepts("1.000000", 1000000);
	accepts("0.6", 600000);
	accepts("0.600001", 600001);
	accepts("0.000001", 1);
	accepts(".5", 500000);
	accepts("1.", 1000000);
	accepts("0.95", 950000);
	accepts("000.5", 500000);
	refuses("0", "above 0");
	refuses("0.0", "above 0");
	refuses("0.000000", "above 0");
	refuses("1.0000001", "six decimals");
	refuses("0.1234567", "six decimals");
	refuses("1.000001", "at most 1");
	refuses("1.5", "at most 1");
	refuses("2", "at most 1");
	refuses("10000000", "at most 1");
	refuses("-0.5", "decimal number");
	refuses("+0.5", "decimal number");
	refuses(".", "decimal number");
	refuses("", "decimal number");
	refuses("0.5x", "decimal number");
	refuses("0,5", "decimal number");
	refuses("1e-1", "decimal number");
	refuses("0.5.1", "decimal number");
	refuses(" 0.5", "decimal number");

	// ---- the worked example: I / U = 3 / 5 is exactly 0.6
	CHECK(cl::similar({3, 5}, 600000) && !cl::similar({3, 5}, 600001) && cl::sim_ppm({3, 5}) == 600000);
	CHECK(!cl::similar({0, 4}, 1) && cl::sim_ppm({0, 4}) == 0);
	CHECK(cl::similar({0, 0}, 1000000) && cl::sim_ppm({0, 0}) == 1000000); // bags of empty segments
	CHECK(cl::better({0, 0}, {999999, 1000000}) && !cl::better({5, 5}, {0, 0}) && !cl::better({0, 0}, {5, 5}));
	CHECK(cl::better({2, 3}, {3, 5}) && !cl::better({3, 5}, {2, 3}) && !cl::better({2, 4}, {1, 2})); // a tie is not better

	// ---- against 128-bit arithmetic: small weights, and weights whose products pass 2^64
	std::mt19937_64 rng(20240607);
	for (int round = 0; round < 200000; round++) {
		const int shift = round % 4 == 0 ? 0 : round % 4 == 1 ? 20 : round % 4 == 2 ? 44 : 58;
		auto draw = [&] { return (rng() >> shift) + (round % 7 == 0 ? 0 : 1); };
		uint64_t U = draw(), I = round % 5 == 0 ? U : rng() % (U + 1);
		uint64_t U2 = draw(), I2 = round % 11 == 0 ? U2 : rng() % (U2 + 1);
		if (round % 13 == 0)
			U = I = 0;
		const uint32_t T = round % 3 == 0 ? 1000000 : 1 + (uint32_t)(rng() % 1000000);
		CHECK(cl::similar({I, U}, T) == similar_ref(I, U, T));
		CHECK(cl::better({I, U}, {I2, U2}) == better_ref(I, U, I2, U2));
		CHECK(cl::sim_ppm({I, U}) == ppm_ref(I, U));
		// at the threshold itself and one ppm above it
		const uint32_t s = ppm_ref(I, U);
		CHECK(s == 0 || cl::similar({I, U}, s));
		CHECK(s == 1000000 || !cl::similar({I, U}, s + 1));
	}
	{
		const uint64_t big = ~0ull; // I * 10^6 is far past 2^64
		CHECK(cl::similar({big, big}, 1000000) && cl::sim_ppm({big, big}) == 1000000 && cl::sim_ppm({big - 1, big}) == 999999);
		CHECK(cl::better({big, big}, {big - 1, big}) && !cl::better({big - 1, big}, {big, big}));
		CHECK(cl::similar({big / 2 + 1, big}, 500000) && !cl::similar({big / 2, big}, 500001));
		const cl::U128 p = cl::mul128(big, big);
		CHECK(p.hi == big - 1 && p.lo == 1);
	}

	// ---- bags: the ordinal rule, the bound, the leader loop
	for (int round = 0; round < 3000; round++) {
		const uint32_t n_seg = 1 + (uint32_t)(rng() % 9), n_bag = 1 + (uint32_t)(rng() % 9);
		std::vector<uint64_t> weight(n_seg);
		for (auto &w : weight)
			w = round % 10 == 0 ? 0 : round % 3 == 0 ? rng() % 3 : 1 + rng() % 50;
		std::vector<cl::Bag> bag;
		for (uint32_t b = 0; b < n_bag; b++) {
			std::vector<uint32_t> keys(rng() % 8);
			for (auto &k : keys)
				k = (uint32_t)(rng() % n_seg);
			if (b && rng() % 3 == 0) { // a near copy of an earlier bag
				keys = bag[rng() % b].key;
				if (!keys.empty() && rng() % 2)
					keys[rng() % keys.size()] = (uint32_t)(rng() % n_seg);
			}
			bag.push_back(make_bag(keys, weight));
		}
		const uint32_t T = round % 4 == 0 ? 1000000 : 1 + (uint32_t)(rng() % 1000000);
		for (uint32_t a = 0; a < n_bag; a++)
			for (uint32_t b = 0; b < n_bag; b++) {
				const cl::Frac f = cl::bag_frac(bag[a], bag[b]), g = counted(bag[a], bag[b], weight), h = cl::bag_frac(bag[b], bag[a]);
				CHECK(f.I == g.I && f.U == g.U && h.I == f.I && h.U == f.U);
				const cl::Frac bd = cl::weight_bound(bag[a].W(), bag[b].W());
				CHECK(f.I <= bd.I && f.U >= bd.U && !cl::better(f, bd)); // the bound is never beaten ...
				if (cl::prunable(bag[a].W(), bag[b].W(), T, false, {0, 0}))
					CHECK(!cl::similar(f, T)); // ... so what it skips could not have joined
			}
		// brute force: no pair skipped, first the similar ones, then the best, the lowest cluster on a tie
		std::vector<uint32_t> of, rep;
		uint32_t low = cl::PPM;
		for (uint32_t a = 0; a < n_bag; a++) {
			int at = -1;
			for (uint32_t k = 0; k < rep.size(); k++) {
				const cl::Frac f = counted(bag[a], bag[rep[k]], weight);
				if (!similar_ref(f.I, f.U, T))
					continue;
				const cl::Frac g = at < 0 ? f : counted(bag[a], bag[rep[at]], weight);
				if (at < 0 || better_ref(f.I, f.U, g.I, g.U))
					at = (int)k;
			}
			if (at < 0) {
				of.push_back((uint32_t)rep.size());
				rep.push_back(a);
			} else {
				of.push_back((uint32_t)at);
				const cl::Frac f = counted(bag[a], bag[rep[at]], weight);
				low = std::min(low, ppm_ref(f.I, f.U));
			}
		}
		const cl::Clusters with = cl::leader(bag, T, false), without = cl::leader(bag, T, true);
		CHECK(with.of == of && with.rep == rep && with.minsim == low);
		CHECK(without.of == of && without.rep == rep && without.minsim == low && without.pruned == 0 && without.pairs == with.pairs);
		CHECK(with.pruned <= with.pairs);
	}
	{ // the worked example: bags {1,2,3,4}, {}, {1,2,6,4} of one-base segments
		const std::vector<uint64_t> weight(7, 1);
		const std::vector<cl::Bag> bag{make_bag({1, 2, 3, 4}, weight), make_bag({}, weight), make_bag({1, 2, 6, 4}, weight)};
		const cl::Clusters at = cl::leader(bag, 600000, false), above = cl::leader(bag, 600001, false);
		CHECK((at.of == std::vector<uint32_t>{0, 1, 0}) && (at.rep == std::vector<uint32_t>{0, 1}) && at.minsim == 600000);
		CHECK((above.of == std::vector<uint32_t>{0, 1, 2}) && above.minsim == 1000000);
		CHECK(at.pairs == 3 && at.pruned == 2); // the empty bag against {1,2,3,4}, and {1,2,6,4} against the empty bag: the weights say no
	}
	{ // a segment three times in one bag and twice in the other
		const std::vector<uint64_t> weight{5, 2};
		const cl::Bag a = make_bag({1, 1, 1, 0}, weight), b = make_bag({1, 0, 1}, weight);
		const cl::Frac f = cl::bag_frac(a, b);
		CHECK(f.I == 9 && f.U == 11);
	}
	puts("cluster_check: ok");
	return 0;
}
