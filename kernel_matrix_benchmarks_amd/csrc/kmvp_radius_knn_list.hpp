// The per-lane candidate list of the radius search (include/kmvp.h kmvp_radius_nearest; pair loop: kmvp_lowd_cutoff_knn.hpp).
//
// kmvp_lowd_knn.hpp's knn_insert orders its list by s alone and gets "ties towards the smaller index" from the walk: the
// brute-force kernels meet the sources in ascending index.  A cell list does not -- records are ordered by row of cells,
// then cell, then the caller's order, so a source with a larger index in an earlier row is met first.  This list is
// therefore ordered by the PAIR (s, j), j the caller's source index:
//   rknn_less     (s, j) < (t, k)  iff  s < t || (s == t && j < k); false both ways for a NaN s
//   rknn_init     a list of capacity KT that keeps the kc <= KT smallest: kc entries at (+inf, -1) behind KT - kc at (-inf, -1)
//   rknn_insert   one candidate into the sorted list: entry t takes the old entry
//                 t - 1 where the candidate is below that one, the candidate where it is below the old entry t only, and
//                 stays otherwise.  A candidate at (+inf, any j >= -1) is below no entry: the caller masks what is outside
//                 the radius to s = +inf and nothing else is needed.  Whatever the order the candidates arrive in, the
//                 list ends as the KT smallest under the order.
//   rknn_insert1  the same for KT = 1: two selects
//   rknn_finish   the end-of-row rule of kmvp_nearest: the K kept entries, or, with exclude_self, the K + 1 kept entries
//                 without the one whose j is the row's own index if it is there and without the last otherwise (exact also
//                 when more than K + 1 sources coincide with the target: the K + 1 entries are then all at distance 0 with
//                 indices below the row's own); an empty entry is (-1, +inf); a NaN row is (-1, NaN) in all K entries.
// Every access is to a compile-time position, so on the device the two arrays stay in registers.
//
// Plain C++ with the device attributes behind a macro: the same text runs in lowd_cutoff_knn_kernel and, compiled with a
// host compiler alone, in tests/test_host_radius_knn_list.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KMVP_HD __host__ __device__
#else
#define KMVP_HD
#endif
#if defined(__clang__)
#define KMVP_UNROLL _Pragma("unroll")
#else
#define KMVP_UNROLL
#endif

namespace kmvp {

template <typename real>
KMVP_HD inline bool rknn_less(real s, int32_t j, real t, int32_t k) {
  return s < t || (s == t && j < k);
}

// A list of capacity KT that keeps kc <= KT entries: they live in positions KT - kc .. KT - 1, behind KT - kc entries at
// (-inf, -1) that no candidate is below (s >= 0) and that therefore never move.  The list's last entry is then the kc-th
// smallest so far whatever kc is: the bound a caller may gate on sits at a fixed position.
template <int KT, typename real>
KMVP_HD inline void rknn_init(real (&sl)[KT], int32_t (&jl)[KT], int kc) {
  KMVP_UNROLL
  for (int t = 0; t < KT; ++t) {
    sl[t] = t < KT - kc ? -(real)__builtin_inf() : (real)__builtin_inf();
    jl[t] = -1;
  }
}

template <int KT, typename real>
KMVP_HD inline void rknn_insert(real (&sl)[KT], int32_t (&jl)[KT], real s, int32_t j) {
  // from the last entry down, so that entry t - 1 is still the old one when entry t is formed, and only two of the
  // comparisons (monotone in t: the list is sorted) are alive at a time
  bool lt = rknn_less<real>(s, j, sl[KT - 1], jl[KT - 1]);
  KMVP_UNROLL
  for (int t = KT - 1; t > 0; --t) {
    const bool lt_prev = rknn_less<real>(s, j, sl[t - 1], jl[t - 1]);
    sl[t] = lt_prev ? sl[t - 1] : (lt ? s : sl[t]);
    jl[t] = lt_prev ? jl[t - 1] : (lt ? j : jl[t]);
    lt = lt_prev;
  }
  sl[0] = lt ? s : sl[0];
  jl[0] = lt ? j : jl[0];
}

template <typename real>
KMVP_HD inline void rknn_insert1(real& s0, int32_t& j0, real s, int32_t j) {
  const bool lt = rknn_less<real>(s, j, s0, j0);
  s0 = lt ? s : s0;
  j0 = lt ? j : j0;
}

// Row `self` of the (N, K) outputs from a list that keeps kc = K + (exclude_self ? 1 : 0) entries (rknn_init).
template <int KT, typename real>
KMVP_HD inline void rknn_finish(const real (&sl)[KT], const int32_t (&jl)[KT], int K, bool exclude_self, int64_t self, bool nan_row,
                                int64_t* idx, double* sqdist) {
  const int kc = K + (exclude_self ? 1 : 0);
  const int off = KT - kc;
  int at = kc;  // the kept entry that is left out: none
  if (exclude_self) {
    at = kc - 1;  // the last of the K + 1
    KMVP_UNROLL
    for (int p = KT - 1; p >= 0; --p)
      if (p >= off && jl[p] >= 0 && (int64_t)jl[p] == self) at = p - off;
  }
  KMVP_UNROLL
  for (int p = 0; p < KT; ++p) {
    const int e = p - off;  // the kept entry at position p
    if (e < 0 || e == at) continue;
    const int o = e > at ? e - 1 : e;
    sqdist[o] = nan_row ? (double)__builtin_nan("") : (double)sl[p];
    idx[o] = nan_row ? (int64_t)-1 : (int64_t)jl[p];
  }
}

}  // namespace kmvp
