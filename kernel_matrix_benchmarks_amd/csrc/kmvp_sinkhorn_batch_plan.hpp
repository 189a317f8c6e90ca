// Plan of the batched Sinkhorn solve (kmvp_sinkhorn_batched.hip): the two directions' batch plans and what ties them.
//   direction 1   target image of x with records of y (T1: the new u from v)   = batch_plan_build(B, y_off, x_off)
//   direction 2   target image of y with records of x (T2: the new v from u)   = batch_plan_build(B, x_off, y_off)
// On top of kmvp_batch_plan.hpp, per direction:
//   tile_batch [tiles]   the batch a tile's lanes belong to, -1 for the filler tiles -- BatchTile itself stays as it is
//   tile_begin [B + 1]   batch b owns the tiles [tile_begin[b], tile_begin[b + 1]): contiguous and ascending, the order
//                        in which the solver adds a batch's per-tile error sums
//   other_rec  [n_pad]   for the target in a slot, the record that holds the same point in the OTHER direction's record
//                        array (-1 for a pad slot): where a fresh potential's signal slot is
// Retiring a tile sets its len to 0 and nothing else: rec0 keeps pointing inside the record array, where the pair loop
// still issues its first prefetch.
//
// Plain C++ with nothing of HIP in it, as kmvp_batch_plan.hpp: the same text compiles into kmvp_sinkhorn_batched.hip and,
// with a host compiler alone, into tests/test_host_sinkhorn_batch_plan.py.
#pragma once
#include "kmvp_batch_plan.hpp"

namespace kmvp {

struct SinkhornDirection {
  BatchPlan plan;
  std::vector<int32_t> tile_batch;
  std::vector<int64_t> tile_begin;
  std::vector<int64_t> other_rec;
};

struct SinkhornBatchPlan {
  SinkhornDirection d1, d2;
};

// First batch (>= 0) with points on one side only, -1 if there is none.
inline int sinkhorn_one_sided_batch(int B, const int64_t* y_off, const int64_t* x_off) {
  for (int b = 0; b < B; ++b)
    if ((y_off[b + 1] == y_off[b]) != (x_off[b + 1] == x_off[b])) return b;
  return -1;
}

// One direction: targets at t_off, sources at s_off.  The other direction's records are the targets themselves, padded
// per batch to whole rounds of BATCH_RECORDS in the caller's order.
inline bool sinkhorn_direction_build(int B, const int64_t* s_off, const int64_t* t_off, SinkhornDirection& d) {
  if (!batch_plan_build(B, s_off, t_off, d.plan)) return false;
  d.tile_batch.clear();
  d.tile_begin.assign(1, 0);
  d.other_rec.clear();
  int64_t rec = 0;  // first record of batch b's targets in the other direction's array
  for (int b = 0; b < B; ++b) {
    const int64_t n = t_off[b + 1] - t_off[b];
    for (int64_t t0 = 0; t0 < n; t0 += BATCH_TILE) {
      d.tile_batch.push_back(b);
      for (int64_t l = 0; l < BATCH_TILE; ++l) d.other_rec.push_back(t0 + l < n ? rec + t0 + l : (int64_t)-1);
    }
    d.tile_begin.push_back((int64_t)d.tile_batch.size());
    rec += batch_round_up(n, BATCH_RECORDS);
  }
  while (d.tile_batch.size() < d.plan.tiles.size()) {  // the filler tiles
    d.tile_batch.push_back(-1);
    for (int l = 0; l < BATCH_TILE; ++l) d.other_rec.push_back(-1);
  }
  return true;
}

inline bool sinkhorn_batch_plan_build(int B, const int64_t* y_off, const int64_t* x_off, SinkhornBatchPlan& p) {
  return sinkhorn_direction_build(B, y_off, x_off, p.d1) && sinkhorn_direction_build(B, x_off, y_off, p.d2);
}

}  // namespace kmvp
