// Host-side shim for tests/test_host_sinkhorn_batch_plan.py: csrc/kmvp_sinkhorn_batch_plan.hpp (both directions' plans of
// the batched Sinkhorn solve, the tile-to-batch maps, the tile ranges and the record of every target in the other
// direction) compiled with a host compiler alone, behind a C surface.
#include <stddef.h>

#include "kmvp_sinkhorn_batch_plan.hpp"

extern "C" {

int hs_one_sided(int B, const int64_t* y_off, const int64_t* x_off) { return kmvp::sinkhorn_one_sided_batch(B, y_off, x_off); }

// nullptr: a plan refused the offsets (a range of 2^31 records)
void* hs_build(int B, const int64_t* y_off, const int64_t* x_off) {
  kmvp::SinkhornBatchPlan* p = new kmvp::SinkhornBatchPlan();
  if (!kmvp::sinkhorn_batch_plan_build(B, y_off, x_off, *p)) {
    delete p;
    return nullptr;
  }
  return p;
}

void hs_free(void* h) { delete (kmvp::SinkhornBatchPlan*)h; }

static const kmvp::SinkhornDirection& dir(const void* h, int d) {
  const kmvp::SinkhornBatchPlan& p = *(const kmvp::SinkhornBatchPlan*)h;
  return d == 1 ? p.d1 : p.d2;
}

// out[0 .. 6): n_pad, m_pad, m_alloc, tiles, entries of tile_begin, entries of other_rec
void hs_sizes(const void* h, int d, int64_t* out) {
  const kmvp::SinkhornDirection& s = dir(h, d);
  out[0] = s.plan.n_pad;
  out[1] = s.plan.m_pad;
  out[2] = s.plan.m_alloc;
  out[3] = (int64_t)s.plan.tiles.size();
  out[4] = (int64_t)s.tile_begin.size();
  out[5] = (int64_t)s.other_rec.size();
}

// tiles as rows of six int64: rec0, j0, i0, len, live, batch
void hs_tiles(const void* h, int d, int64_t* out) {
  const kmvp::SinkhornDirection& s = dir(h, d);
  for (size_t t = 0; t < s.plan.tiles.size(); ++t) {
    out[6 * t + 0] = s.plan.tiles[t].rec0;
    out[6 * t + 1] = s.plan.tiles[t].j0;
    out[6 * t + 2] = s.plan.tiles[t].i0;
    out[6 * t + 3] = s.plan.tiles[t].len;
    out[6 * t + 4] = s.plan.tiles[t].live;
    out[6 * t + 5] = t < s.tile_batch.size() ? s.tile_batch[t] : -99;
  }
}

void hs_maps(const void* h, int d, int64_t* tile_begin, int64_t* other_rec, int64_t* tmap, int64_t* smap) {
  const kmvp::SinkhornDirection& s = dir(h, d);
  for (size_t i = 0; i < s.tile_begin.size(); ++i) tile_begin[i] = s.tile_begin[i];
  for (size_t i = 0; i < s.other_rec.size(); ++i) other_rec[i] = s.other_rec[i];
  for (size_t i = 0; i < s.plan.tmap.size(); ++i) tmap[i] = s.plan.tmap[i];
  for (size_t i = 0; i < s.plan.smap.size(); ++i) smap[i] = s.plan.smap[i];
}

}
