// Host-side shim for tests/test_host_cutoff_plan.py: csrc/kmvp_cutoff_plan.hpp (the cell list and launch plan of the
// cutoff-radius entries) compiled with a host compiler alone, behind a C surface.
#include <stddef.h>

#include "kmvp_cutoff_plan.hpp"

extern "C" {

int hc_tile() { return kmvp::CUTOFF_TILE; }
int hc_waves() { return kmvp::CUTOFF_WAVES; }
long hc_records() { return (long)kmvp::CUTOFF_RECORDS; }
long hc_max_axis() { return (long)kmvp::CUTOFF_MAX_AXIS; }
int hc_tile_bytes() { return (int)sizeof(kmvp::CutoffTile); }
int hc_run_bytes() { return (int)sizeof(kmvp::CutoffRun); }

// nullptr: the plan refused (2^31 sources)
void* hc_build(const double* y, long M, const double* x, long N, int D, double R, double factor) {
  kmvp::CutoffPlan* p = new kmvp::CutoffPlan();
  if (!kmvp::cutoff_plan_build(y, M, x, N, D, R, factor, *p)) {
    delete p;
    return nullptr;
  }
  return p;
}

void hc_free(void* h) { delete (kmvp::CutoffPlan*)h; }

// out[0 .. 12): g[3], n_pad, m_pad, m_alloc, live_tiles, walked, tiles, runs, entries of tmap, entries of smap;
// grid[0 .. 4): lo[3], h
void hc_sizes(const void* h, int64_t* out, double* grid) {
  const kmvp::CutoffPlan& p = *(const kmvp::CutoffPlan*)h;
  for (int d = 0; d < 3; ++d) {
    out[d] = p.g[d];
    grid[d] = p.lo[d];
  }
  grid[3] = p.h;
  out[3] = p.n_pad;
  out[4] = p.m_pad;
  out[5] = p.m_alloc;
  out[6] = p.live_tiles;
  out[7] = p.walked;
  out[8] = (int64_t)p.tiles.size();
  out[9] = (int64_t)p.runs.size();
  out[10] = (int64_t)p.tmap.size();
  out[11] = (int64_t)p.smap.size();
}

// tiles as rows of three int64 (run0, nruns, live), runs as rows of two (rec0, len)
void hc_tables(const void* h, int64_t* tiles, int64_t* runs) {
  const kmvp::CutoffPlan& p = *(const kmvp::CutoffPlan*)h;
  for (size_t t = 0; t < p.tiles.size(); ++t) {
    tiles[3 * t + 0] = p.tiles[t].run0;
    tiles[3 * t + 1] = p.tiles[t].nruns;
    tiles[3 * t + 2] = p.tiles[t].live;
  }
  for (size_t r = 0; r < p.runs.size(); ++r) {
    runs[2 * r + 0] = p.runs[r].rec0;
    runs[2 * r + 1] = p.runs[r].len;
  }
}

void hc_maps(const void* h, int64_t* tmap, int64_t* smap) {
  const kmvp::CutoffPlan& p = *(const kmvp::CutoffPlan*)h;
  for (size_t i = 0; i < p.tmap.size(); ++i) tmap[i] = p.tmap[i];
  for (size_t i = 0; i < p.smap.size(); ++i) smap[i] = p.smap[i];
}

}
