// Host-side shim for tests/test_host_batch_plan.py: csrc/kmvp_batch_plan.hpp (the layout and launch plan of the batched
// clouds) compiled with a host compiler alone, behind a C surface.
#include <stddef.h>

#include "kmvp_batch_plan.hpp"

extern "C" {

int hb_tile() { return kmvp::BATCH_TILE; }
int hb_waves() { return kmvp::BATCH_WAVES; }
long hb_records() { return (long)kmvp::BATCH_RECORDS; }
long hb_max_range() { return (long)kmvp::BATCH_MAX_RANGE; }
int hb_tile_bytes() { return (int)sizeof(kmvp::BatchTile); }

int hb_check(int B, const int64_t* off, long total) { return kmvp::batch_offsets_check(B, off, total); }

// nullptr: the plan refused the offsets (a range of 2^31 records)
void* hb_build(int B, const int64_t* y_off, const int64_t* x_off) {
  kmvp::BatchPlan* p = new kmvp::BatchPlan();
  if (!kmvp::batch_plan_build(B, y_off, x_off, *p)) {
    delete p;
    return nullptr;
  }
  return p;
}

void hb_free(void* h) { delete (kmvp::BatchPlan*)h; }

// out[0 .. 5): n_pad, m_pad, m_alloc, tiles, entries of tmap, entries of smap
void hb_sizes(const void* h, int64_t* out) {
  const kmvp::BatchPlan& p = *(const kmvp::BatchPlan*)h;
  out[0] = p.n_pad;
  out[1] = p.m_pad;
  out[2] = p.m_alloc;
  out[3] = (int64_t)p.tiles.size();
  out[4] = (int64_t)p.tmap.size();
  out[5] = (int64_t)p.smap.size();
}

// tiles as rows of five int64: rec0, j0, i0, len, live
void hb_tiles(const void* h, int64_t* out) {
  const kmvp::BatchPlan& p = *(const kmvp::BatchPlan*)h;
  for (size_t t = 0; t < p.tiles.size(); ++t) {
    out[5 * t + 0] = p.tiles[t].rec0;
    out[5 * t + 1] = p.tiles[t].j0;
    out[5 * t + 2] = p.tiles[t].i0;
    out[5 * t + 3] = p.tiles[t].len;
    out[5 * t + 4] = p.tiles[t].live;
  }
}

void hb_maps(const void* h, int64_t* tmap, int64_t* smap) {
  const kmvp::BatchPlan& p = *(const kmvp::BatchPlan*)h;
  for (size_t i = 0; i < p.tmap.size(); ++i) tmap[i] = p.tmap[i];
  for (size_t i = 0; i < p.smap.size(); ++i) smap[i] = p.smap[i];
}

}
