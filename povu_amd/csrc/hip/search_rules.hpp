// search_rules.hpp -- the binary searches of the device code, written once.  Free of HIP.  Two primitives over an index range
// and a predicate on an index, and on top of them the named forms that have more than one caller:
//   first_not(lo, hi, before)   the first i of [lo, hi) where before(i) fails, hi when there is none; before holds on a prefix
//   last_upto(lo, hi, upto)     the last i of [lo, hi) where upto(i) holds; lo < hi, and upto(lo) is taken for granted
//   lower_bound / upper_bound   first_not over a plain ascending array: the first element >= x / > x
//   span_of                     last_upto over an ascending offset table: the span a position lies in
// (the components of the decompose pass are found through keys made of an offset and the index: CompSpans, common.hpp).
// The midpoint is lo + (hi - lo) / 2, which does not wrap where lo + hi does (lists of 2^31 entries and more, DESIGN.md
// section 3).  The two loops are kept apart on purpose: they probe different indices, and the hot kernels load from them.
// Not here: cluster_rules.hpp sim_ppm bisects a range of VALUES (midpoint rounded up, 128-bit products), no array;
// prim_merge.hpp rows_touch runs a fixed, wave-uniform trip count on purpose.
// host/search_check.cpp holds all of this to the standard library on the CPU under the sanitizers.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SEARCH_FN __host__ __device__ inline
#else
#define SEARCH_FN inline
#endif

namespace povu_hip
{

template <class I, class Before> SEARCH_FN I first_not(I lo, I hi, Before &&before)
{
	while (lo < hi) {
		const I mid = lo + ((hi - lo) >> 1);
		if (before(mid))
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}
template <class I, class Upto> SEARCH_FN I last_upto(I lo, I hi, Upto &&upto)
{
	while (hi - lo > 1) {
		const I mid = lo + ((hi - lo) >> 1);
		if (upto(mid))
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

// (the key takes the array's element type; it is not deduced a second time)
template <class T> struct search_key {
	using type = T;
};
// the first i of [lo, hi) with a[i] >= x / a[i] > x, hi when there is none; a ascending over [lo, hi)
template <class T, class I> SEARCH_FN I lower_bound(const T *a, I lo, I hi, typename search_key<T>::type x)
{
	return first_not(lo, hi, [=](I i) { return a[i] < x; });
}
template <class T, class I> SEARCH_FN I upper_bound(const T *a, I lo, I hi, typename search_key<T>::type x)
{
	return first_not(lo, hi, [=](I i) { return a[i] <= x; });
}
// the span x lies in: the last k of [0, n) with off[k] <= x, off ascending, n > 0 (of equal offsets -- empty spans -- the last)
template <class T, class I> SEARCH_FN I span_of(const T *off, I n, typename search_key<T>::type x)
{
	return last_upto(I(0), n, [=](I k) { return off[k] <= x; });
}

} // namespace povu_hip
