// cluster_rules.hpp -- the rules of the clustered calls (INTEGRATION.md "Clustered calls"; restated in tests/cluster_ref.py),
// free of HIP: the parser of the threshold, the similarity of two bags from (I, U) with 128-bit products, the comparison of two
// fractions, sim_ppm, the weight bound that lets a pair be skipped without reading a bag, the intersection of two sorted bags
// and the leader loop over them.  Included by cluster_kernels.hip (the device functions), by host/vcf.cpp (the parser) and by
// host/cluster_check.cpp, which runs all of it under the sanitizers.  There is no floating point in here.
#pragma once
#include "search_rules.hpp"

#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define CL_HD __host__ __device__ __forceinline__
#else
#define CL_HD inline
#endif

namespace cluster
{

static constexpr uint32_t PPM = 1000000u; // the threshold T is F * 10^6, an integer in 1 .. 10^6

// a * b in 128 bits
struct U128 {
	uint64_t hi, lo;
};
CL_HD U128 mul128(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return U128{__umul64hi(a, b), a * b};
#else
	const unsigned __int128 p = (unsigned __int128)a * b;
	return U128{(uint64_t)(p >> 64), (uint64_t)p};
#endif
}
CL_HD bool less128(const U128 &a, const U128 &b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }

// intersection weight I and union weight U of two bags.  U == 0 (bags of empty segments, or no key at all) counts as the
// fraction 1
struct Frac {
	uint64_t I, U;
};
CL_HD Frac canon(Frac f) { return f.U == 0 ? Frac{1, 1} : f; }
// I / U >= T / 10^6
CL_HD bool similar(Frac f, uint32_t T)
{
	f = canon(f);
	return !less128(mul128(f.I, PPM), mul128(f.U, T));
}
// a is strictly the larger fraction
CL_HD bool better(Frac a, Frac b)
{
	a = canon(a), b = canon(b);
	return less128(mul128(b.I, a.U), mul128(a.I, b.U));
}
// floor(I * 10^6 / U), 10^6 when U == 0.  I <= U, so the quotient is the largest q in [0, 10^6] with q * U <= I * 10^6
CL_HD uint32_t sim_ppm(Frac f)
{
	f = canon(f);
	const U128 num = mul128(f.I, PPM);
	uint32_t lo = 0, hi = PPM;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo + 1) / 2;
		if (less128(num, mul128(f.U, mid)))
			hi = mid - 1;
		else
			lo = mid;
	}
	return lo;
}
// the most a pair of bags of weights wa and wr can reach: I <= min, U >= max
CL_HD Frac weight_bound(uint64_t wa, uint64_t wr) { return Frac{wa < wr ? wa : wr, wa < wr ? wr : wa}; }
// the pair need not be read: the bound is not similar, or a best is held and the bound does not beat it (a tie goes to the
// lower cluster, which is the one held)
CL_HD bool prunable(uint64_t wa, uint64_t wr, uint32_t T, bool has_best, Frac best)
{
	const Frac b = weight_bound(wa, wr);
	return !similar(b, T) || (has_best && !better(b, best));
}

// key (s, o) of one bag, o its ordinal among the equal segments of its bag, counts towards I when the other bag holds s more
// than o times
template <class Key>
CL_HD bool key_counts(const Key *other, uint32_t lo, uint32_t hi, Key s, uint32_t o)
{
	return povu_hip::upper_bound(other, lo, hi, s) - povu_hip::lower_bound(other, lo, hi, s) > o;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host only
// F as decimal text with at most six decimals, 0 < F <= 1, to T = F * 10^6 exactly; the refusal, or "" and *ppm
inline std::string parse(const char *text, uint32_t *ppm)
{
	const std::string t = text ? text : "";
	const std::string who = "cluster threshold '" + t + "': ";
	const size_t dot = t.find('.');
	const std::string ip = t.substr(0, dot), fp = dot == std::string::npos ? std::string() : t.substr(dot + 1);
	auto digits = [](const std::string &x) {
		for (char c : x)
			if (c < '0' || c > '9')
				return false;
		return true;
	};
	if (!digits(ip) || !digits(fp) || (ip.empty() && fp.empty()))
		return who + "expected a decimal number such as 0.9";
	if (fp.size() > 6)
		return who + "more than six decimals";
	if (ip.size() > 6)
		return who + "must be above 0 and at most 1";
	uint64_t whole = 0, frac = 0;
	for (char c : ip)
		whole = whole * 10 + (uint64_t)(c - '0');
	for (size_t k = 0; k < 6; k++)
		frac = frac * 10 + (k < fp.size() ? (uint64_t)(fp[k] - '0') : 0);
	const uint64_t T = whole * PPM + frac;
	if (T == 0 || T > PPM)
		return who + "must be above 0 and at most 1";
	*ppm = (uint32_t)T;
	return std::string();
}

// a bag as the kernels keep it: the segments ascending, the weight of every key
struct Bag {
	std::vector<uint32_t> key;
	std::vector<uint64_t> w;
	uint64_t W() const
	{
		uint64_t s = 0;
		for (uint64_t x : w)
			s += x;
		return s;
	}
};
inline Frac bag_frac(const Bag &a, const Bag &r)
{
	uint64_t I = 0;
	for (uint32_t k = 0, o = 0; k < a.key.size(); k++) {
		o = k && a.key[k] == a.key[k - 1] ? o + 1 : 0;
		if (key_counts(r.key.data(), 0u, (uint32_t)r.key.size(), a.key[k], o))
			I += a.w[k];
	}
	return Frac{I, a.W() + r.W() - I};
}
// the leader loop over the sorted bags of one site: the cluster of every allele, the representatives, the lowest sim_ppm of a
// member to its representative, the pairs looked at and the pairs the bound skipped
struct Clusters {
	std::vector<uint32_t> of, rep;
	uint32_t minsim = PPM;
	uint64_t pairs = 0, pruned = 0;
};
inline Clusters leader(const std::vector<Bag> &bag, uint32_t T, bool no_bound)
{
	Clusters c;
	for (uint32_t a = 0; a < bag.size(); a++) {
		bool has = false;
		Frac best{0, 0};
		uint32_t at = 0;
		for (uint32_t k = 0; k < c.rep.size(); k++) {
			c.pairs++;
			if (!no_bound && prunable(bag[a].W(), bag[c.rep[k]].W(), T, has, best)) {
				c.pruned++;
				continue;
			}
			const Frac f = bag_frac(bag[a], bag[c.rep[k]]);
			if (similar(f, T) && (!has || better(f, best)))
				has = true, best = f, at = k;
		}
		if (!has) {
			c.of.push_back((uint32_t)c.rep.size());
			c.rep.push_back(a);
			continue;
		}
		c.of.push_back(at);
		const uint32_t s = sim_ppm(best);
		c.minsim = s < c.minsim ? s : c.minsim;
	}
	return c;
}
#endif

} // namespace cluster
