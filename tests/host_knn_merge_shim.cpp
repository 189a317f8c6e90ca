// Host-side shim for tests/test_host_knn_merge.py: csrc/kmvp_knn_merge.hpp (the merge of sorted candidate lists and the
// exclude-self drop of the K-nearest-neighbour reduction) compiled with a host compiler alone, behind a C surface.
#include "kmvp_knn_merge.hpp"

extern "C" {

int hk_max_k() { return kmvp::KNN_MAX_K; }

void hk_merge(const double* lists, long list_stride, long elem_stride, int S, int KT, int K, double* out_s, double* out_j,
              long out_stride) {
  kmvp::knn_merge(lists, list_stride, elem_stride, S, KT, K, out_s, out_j, out_stride);
}

void hk_drop_self(double* s, double* j, long stride, int K1, long self) { kmvp::knn_drop_self(s, j, stride, K1, self); }

}
