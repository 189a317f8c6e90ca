// Layout and launch plan of the batched clouds (include/kmvp.h kmvp_set_batches; kernels: kmvp_lowd_batch.hpp).
//
// B clouds are concatenated in the caller's arrays: batch b owns sources [y_off[b], y_off[b + 1]) and targets
// [x_off[b], x_off[b + 1]).  The kernels work on padded images of both:
//  * targets: every batch is padded to whole wave tiles of BATCH_TILE = 64 slots, so a wave never holds targets of two
//    batches; the padded count is rounded up to whole workgroups (BATCH_WAVES tiles) with filler tiles whose source range
//    is empty and which have no live lane;
//  * sources: every batch is padded to a multiple of BATCH_RECORDS = 8 records (the family's pad records: y = +inf,
//    b = 0), a batch's range starts where the previous one ended, and the record array carries one spare batch of 8
//    records at its very end -- the ping-pong prefetch of the scalar-cache feed reads one batch past the range it consumes.
// One BatchTile per wave tile says which records the wave walks and where its lanes' rows go; tmap / smap are the padded
// -> caller index maps (-1: a pad) of the two gather-pack kernels.
//
// Plain C++ with nothing of HIP in it: the same text compiles into kmvp_batch.hip and, with a host compiler alone, into
// tests/test_host_batch_plan.py.
#pragma once
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KMVP_BATCH_HD __host__ __device__
#else
#define KMVP_BATCH_HD
#endif

namespace kmvp {

constexpr int BATCH_TILE = 64;           // targets per wave tile: one per lane
constexpr int BATCH_WAVES = 4;           // wave tiles per workgroup (WAVES_PER_BLOCK of the pair-loop kernels)
constexpr int64_t BATCH_RECORDS = 8;     // source records per ping-pong round (LOWD_BATCH): ranges are multiples of it
constexpr int64_t BATCH_MAX_RANGE = 0x7fffffff - 7;  // the longest padded range: a multiple of 8 below 2^31

// What one wave reads before its loop.  32 bytes, so that a tile's entry is one aligned scalar load.
struct BatchTile {
  int64_t rec0;  // first record of the tile's source range
  int64_t j0;    // the caller's index of that record's source: position + j0 is the global index of a neighbour
  int64_t i0;    // the caller's index of lane 0's target; lane l < live owns target i0 + l
  int32_t len;   // padded length of the range: a multiple of BATCH_RECORDS, 0 for an empty batch and for filler tiles
  int32_t live;  // lanes that own a target (0 .. BATCH_TILE)
};
static_assert(sizeof(BatchTile) == 32, "one tile entry is 32 bytes");

struct BatchPlan {
  int64_t n_pad = 0;    // target slots: tiles.size() * BATCH_TILE, whole workgroups
  int64_t m_pad = 0;    // records of all ranges
  int64_t m_alloc = 0;  // m_pad + the spare batch: records the array holds
  std::vector<BatchTile> tiles;
  std::vector<int64_t> tmap;  // [n_pad]   target slot -> caller's target index, -1 for a pad
  std::vector<int64_t> smap;  // [m_alloc] record      -> caller's source index, -1 for a pad
};

KMVP_BATCH_HD inline int64_t batch_round_up(int64_t v, int64_t q) { return (v + q - 1) / q * q; }

// Offsets of B batches over `total` points: B + 1 non-decreasing values from 0 to total.  0: fine; 1: does not start at 0;
// 2: not monotone; 3: does not end at total.
inline int batch_offsets_check(int B, const int64_t* off, int64_t total) {
  if (off[0] != 0) return 1;
  for (int b = 0; b < B; ++b)
    if (off[b + 1] < off[b]) return 2;
  if (off[B] != total) return 3;
  return 0;
}

// The plan of B >= 1 batches with checked offsets.  false: a batch's padded source range would reach 2^31 records (the
// pair loop counts positions within a range in 32 bits); the plan is then unusable.
inline bool batch_plan_build(int B, const int64_t* y_off, const int64_t* x_off, BatchPlan& p) {
  p = BatchPlan();
  int64_t rec = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t m = y_off[b + 1] - y_off[b], n = x_off[b + 1] - x_off[b];
    if (m > BATCH_MAX_RANGE) return false;
    const int64_t len = batch_round_up(m, BATCH_RECORDS);
    for (int64_t t0 = 0; t0 < n; t0 += BATCH_TILE) {
      BatchTile t;
      t.rec0 = rec;
      t.j0 = y_off[b];
      t.i0 = x_off[b] + t0;
      t.len = (int32_t)len;
      t.live = (int32_t)(n - t0 < BATCH_TILE ? n - t0 : BATCH_TILE);
      p.tiles.push_back(t);
      for (int l = 0; l < BATCH_TILE; ++l) p.tmap.push_back(l < t.live ? t.i0 + l : (int64_t)-1);
    }
    for (int64_t j = 0; j < len; ++j) p.smap.push_back(j < m ? y_off[b] + j : (int64_t)-1);
    rec += len;
  }
  p.m_pad = rec;
  p.m_alloc = rec + BATCH_RECORDS;
  for (int64_t j = 0; j < BATCH_RECORDS; ++j) p.smap.push_back(-1);  // the spare batch
  while (p.tiles.size() % BATCH_WAVES) {  // filler tiles: an empty range (at record 0, always inside the array), no live lane
    BatchTile t;
    t.rec0 = 0;
    t.j0 = 0;
    t.i0 = 0;
    t.len = 0;
    t.live = 0;
    p.tiles.push_back(t);
    for (int l = 0; l < BATCH_TILE; ++l) p.tmap.push_back(-1);
  }
  p.n_pad = (int64_t)p.tiles.size() * BATCH_TILE;
  return true;
}

}  // namespace kmvp
