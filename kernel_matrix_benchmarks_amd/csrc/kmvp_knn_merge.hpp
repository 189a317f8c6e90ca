// Merge step of the K-nearest-neighbour reduction (include/kmvp.h kmvp_nearest; pair loop: kmvp_lowd_knn.hpp).
//
// lowd_knn_kernel leaves, per (segment, target), a list of KT candidates (s, j) -- squared distance and GLOBAL source
// index, both as float64 -- sorted under the lexicographic order on (s, j) and padded with (+inf, -1).  knn_merge() folds
// S such lists of one target into the K smallest under the same order; the ranks of a communicator are merged by the same
// function with `world` lists in place of segments.  knn_drop_self() is the exclude-self rule.
//
// Plain C++ with the device attributes behind a macro: the same text runs in knn_merge_kernel (kmvp_internal.hpp) and,
// compiled with a host compiler alone, in tests/test_host_knn_merge.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KMVP_HD __host__ __device__
#else
#define KMVP_HD
#endif

namespace kmvp {

constexpr int KNN_MAX_K = 16;  // candidates a list holds at most (K <= 16; K <= 15 with exclude_self: K + 1 are collected)

// (s, j) < (t, k) in the lexicographic order.  NaN compares false both ways; a pad (+inf, -1) is never below a pad.
KMVP_HD inline bool knn_less(double s, double j, double t, double k) { return s < t || (s == t && j < k); }

// The K smallest of S sorted lists of KT candidates each.  Candidate k of list l is
//   s = lists[l * list_stride + k * elem_stride],   j = lists[l * list_stride + (KT + k) * elem_stride]
// (the [list][2 KT][targets] layout of the partial results, `lists` already offset to the target).  The result goes to
// out_s[k * out_stride], out_j[k * out_stride], k < K <= KNN_MAX_K, padded with (+inf, -1).  Candidates with s = +inf are
// pads and never enter.  A NaN distance anywhere marks a NaN target row: the result is then (NaN, -1) in all K entries.
KMVP_HD inline void knn_merge(const double* lists, int64_t list_stride, int64_t elem_stride, int S, int KT, int K,
                              double* out_s, double* out_j, int64_t out_stride) {
  double bs[KNN_MAX_K], bj[KNN_MAX_K];
  const double inf = __builtin_inf();
  for (int k = 0; k < K; ++k) {
    bs[k] = inf;
    bj[k] = -1.0;
  }
  bool nan_row = false;
  for (int l = 0; l < S; ++l) {
    const double* base = lists + (int64_t)l * list_stride;
    for (int k = 0; k < KT; ++k) {
      const double s = base[(int64_t)k * elem_stride];
      const double j = base[(int64_t)(KT + k) * elem_stride];
      if (s != s) nan_row = true;
      // the list is sorted: once a candidate does not enter, no later one of this list does (a pad never does)
      if (!(s < inf) || !knn_less(s, j, bs[K - 1], bj[K - 1])) break;
      int t = K - 1;
      for (; t > 0 && knn_less(s, j, bs[t - 1], bj[t - 1]); --t) {
        bs[t] = bs[t - 1];
        bj[t] = bj[t - 1];
      }
      bs[t] = s;
      bj[t] = j;
    }
  }
  for (int k = 0; k < K; ++k) {
    out_s[(int64_t)k * out_stride] = nan_row ? __builtin_nan("") : bs[k];
    out_j[(int64_t)k * out_stride] = nan_row ? -1.0 : bj[k];
  }
}

// Exclude-self: of K1 = K + 1 sorted candidates (stride `stride`), drop the one with j == self when it is there and the
// last one otherwise; the K survivors stay in place, in order, in entries 0 .. K1 - 2.  Exact also when more than K + 1
// sources coincide with the target: ties go to the smaller index, so the K + 1 candidates are then all at distance 0 with
// indices below `self`, and the first K of them are the answer.
KMVP_HD inline void knn_drop_self(double* s, double* j, int64_t stride, int K1, int64_t self) {
  int at = K1 - 1;
  for (int k = 0; k < K1; ++k)
    if (j[(int64_t)k * stride] == (double)self) {
      at = k;
      break;
    }
  for (int k = at; k + 1 < K1; ++k) {
    s[(int64_t)k * stride] = s[(int64_t)(k + 1) * stride];
    j[(int64_t)k * stride] = j[(int64_t)(k + 1) * stride];
  }
}

}  // namespace kmvp
