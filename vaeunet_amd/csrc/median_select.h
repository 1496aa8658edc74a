// Median of an odd number of values by forgetful selection: a
// data-oblivious network of compare-exchanges, no branch and no index depends
// on a value.  Hold K0 = (N + 1) / 2 + 1 values; move the smallest to one end
// and the largest to the other; neither can be the median of the N, so forget
// both and take in the next value; repeat until the values are used up and
// three are held: the middle one is the median.  (The minimum of K0 of the N
// values has (N + 1) / 2 values at or above it, so its rank is below
// (N - 1) / 2, the maximum's likewise above: without the two, the median of the
// N - 2 that remain is the same value, and K0 - 1 = (N - 2 + 1) / 2 + 1.)
//
// Every loop is a compile-time recursion, so every array index is a constant
// and the arrays live in registers.  Cost in compare-exchanges (one min + one
// max each): 20 at N = 9, 132 at N = 25, 480 at N = 49.
//
// No HIP dependency: VU_MEDIAN_HD is empty on the host, so a host program can
// include this file (tests/test_median_select.py).  Order: how two values
// compare; the default is the integer min / max of T.  The host test runs
// the network bit-sliced on the 0-1 principle with lo = a & b, hi = a | b.
#pragma once
#if defined(__HIPCC__)
#define VU_MEDIAN_HD __host__ __device__ __forceinline__
#else
#define VU_MEDIAN_HD inline
#endif

template <typename T>
struct MedianOrder {
  static VU_MEDIAN_HD T lo(T a, T b) { return a < b ? a : b; }
  static VU_MEDIAN_HD T hi(T a, T b) { return a < b ? b : a; }
};

namespace median_detail {

// a <- lo, b <- hi
template <typename Ord, typename T>
VU_MEDIAN_HD void cx(T& a, T& b) {
  const T l = Ord::lo(a, b), h = Ord::hi(a, b);
  a = l;
  b = h;
}

// cx(a[I], a[K - 1 - I]) for I in [I, K / 2): the smaller of each pair to the lower half
template <typename Ord, int K, int I, typename T, int M>
VU_MEDIAN_HD void fold(T (&a)[M]) {
  if constexpr (I < K / 2) {
    cx<Ord>(a[I], a[K - 1 - I]);
    fold<Ord, K, I + 1>(a);
  }
}

// the minimum of a[0 .. E) to a[0]
template <typename Ord, int I, int E, typename T, int M>
VU_MEDIAN_HD void min_to_front(T (&a)[M]) {
  if constexpr (I < E) {
    cx<Ord>(a[0], a[I]);
    min_to_front<Ord, I + 1, E>(a);
  }
}

// the maximum of a[I .. L] to a[L]
template <typename Ord, int I, int L, typename T, int M>
VU_MEDIAN_HD void max_to_back(T (&a)[M]) {
  if constexpr (I < L) {
    cx<Ord>(a[I], a[L]);
    max_to_back<Ord, I + 1, L>(a);
  }
}

// the minimum of a[0 .. K) to a[0] and the maximum to a[K - 1]: K / 2 pairs, then the minimum of the lower half and
// the maximum of the upper half; for odd K the unpaired middle element meets both
template <typename Ord, int K, typename T, int M>
VU_MEDIAN_HD void ends(T (&a)[M]) {
  fold<Ord, K, 0>(a);
  min_to_front<Ord, 1, (K + 1) / 2>(a);
  max_to_back<Ord, K / 2, K - 1>(a);
}

// K values held in a[0 .. K); v[N - (K - 3)] is the next one to take in
template <typename Ord, int N, int K, typename T, int M>
VU_MEDIAN_HD T forget(T (&a)[M], const T (&v)[N]) {
  ends<Ord, K>(a);
  if constexpr (K == 3) {
    return a[1];
  } else {
    a[0] = v[N - (K - 3)];   // over the minimum; the maximum a[K - 1] drops out of the held range
    return forget<Ord, N, K - 1>(a, v);
  }
}

template <int I, int E, typename T, int M, int N>
VU_MEDIAN_HD void take(T (&a)[M], const T (&v)[N]) {
  if constexpr (I < E) {
    a[I] = v[I];
    take<I + 1, E>(a, v);
  }
}

}  // namespace median_detail

// the element of rank (N - 1) / 2 of v[0 .. N) in Ord's order, N odd and >= 5
template <int N, typename T, typename Ord = MedianOrder<T>>
VU_MEDIAN_HD T median_select(const T (&v)[N]) {
  static_assert(N % 2 == 1 && N >= 5, "an odd window of at least 5 values");
  constexpr int K0 = (N + 1) / 2 + 1;
  T a[K0];
  median_detail::take<0, K0>(a, v);
  return median_detail::forget<Ord, N, K0>(a, v);
}
