// Host-side shim for tests/test_host_radius_knn_list.py: csrc/kmvp_radius_knn_list.hpp (the lexicographic candidate list of
// kmvp_radius_nearest and its end-of-row rule) compiled with the host compiler alone.  One row: n candidates (s, j) in the
// order given, masked at r2 exactly as lowd_cutoff_knn_kernel masks them, through a list of capacity KT that keeps
// K (+ 1 with exclude_self) entries, then rknn_finish into idx[K], sqdist[K].
#include <stdint.h>

#include "kmvp_radius_knn_list.hpp"

namespace {

template <int KT, typename real>
void row(const real* s, const int32_t* j, long n, real r2, int K, int exclude_self, long self, int nan_row, int64_t* idx, double* sqdist) {
  real sl[KT];
  int32_t jl[KT];
  kmvp::rknn_init<KT, real>(sl, jl, K + (exclude_self ? 1 : 0));
  for (long c = 0; c < n; ++c) {
    const real v = s[c] <= r2 ? s[c] : (real)__builtin_inf();
    if (KT == 1) kmvp::rknn_insert1<real>(sl[0], jl[0], v, j[c]);
    else kmvp::rknn_insert<KT, real>(sl, jl, v, j[c]);
  }
  kmvp::rknn_finish<KT, real>(sl, jl, K, exclude_self != 0, (int64_t)self, nan_row != 0, idx, sqdist);
}

template <typename real>
int row_kt(int KT, const real* s, const int32_t* j, long n, real r2, int K, int exclude_self, long self, int nan_row, int64_t* idx,
           double* sqdist) {
  if (K < 1 || K + (exclude_self ? 1 : 0) > KT) return 1;
  switch (KT) {
    case 1: row<1, real>(s, j, n, r2, K, exclude_self, self, nan_row, idx, sqdist); return 0;
    case 4: row<4, real>(s, j, n, r2, K, exclude_self, self, nan_row, idx, sqdist); return 0;
    case 16: row<16, real>(s, j, n, r2, K, exclude_self, self, nan_row, idx, sqdist); return 0;
    default: return 1;
  }
}

}  // namespace

extern "C" {
int hr_row_f32(int KT, const float* s, const int32_t* j, long n, float r2, int K, int exclude_self, long self, int nan_row,
               int64_t* idx, double* sqdist) {
  return row_kt<float>(KT, s, j, n, r2, K, exclude_self, self, nan_row, idx, sqdist);
}
int hr_row_f64(int KT, const double* s, const int32_t* j, long n, double r2, int K, int exclude_self, long self, int nan_row,
               int64_t* idx, double* sqdist) {
  return row_kt<double>(KT, s, j, n, r2, K, exclude_self, self, nan_row, idx, sqdist);
}
}
