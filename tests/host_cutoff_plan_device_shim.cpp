// Host-side shim for tests/test_host_cutoff_plan_device.py: csrc/kmvp_cutoff_plan_device.hpp (the element-by-element rules of
// the device-side plan build) compiled with a host compiler alone and run the way the kernels of
// csrc/kmvp_cutoff_plan_device.hip run them -- std::stable_sort for the radix sort, plain loops for the scans and one loop
// trip per thread -- behind the C surface of tests/host_cutoff_plan_shim.cpp, plus cutoff_plan_build itself (hd_build_host)
// so that one library answers both.
#include <stddef.h>

#include <algorithm>
#include <numeric>

#include "kmvp_cutoff_plan_device.hpp"

namespace {

using namespace kmvp;

struct SortedCloud {
  std::vector<uint32_t> keys;
  std::vector<int32_t> idx, first;
  CutoffSorted view() const { return CutoffSorted{keys.data(), idx.data(), first.data(), (int64_t)keys.size()}; }
};

void sort_cloud(const double* pts, int64_t n, const CutoffGridView& gv, SortedCloud& s) {
  std::vector<uint32_t> key((size_t)n);
  for (int64_t i = 0; i < n; ++i) key[i] = cutoff_point_key(pts + i * gv.D, gv);
  const uint32_t mask = (uint32_t)(((uint64_t)1 << cutoff_key_bits(gv.ncells)) - 1);  // the sort looks at the low bits only
  s.idx.resize((size_t)n);
  std::iota(s.idx.begin(), s.idx.end(), 0);
  std::stable_sort(s.idx.begin(), s.idx.end(), [&](int32_t a, int32_t b) { return (key[a] & mask) < (key[b] & mask); });
  s.keys.resize((size_t)n);
  for (int64_t p = 0; p < n; ++p) s.keys[p] = key[s.idx[p]];
  s.first.resize((size_t)gv.ncells + 1);
  for (int64_t c = 0; c <= gv.ncells; ++c) s.first[c] = cutoff_lower_bound(s.keys.data(), n, (uint32_t)c);
}

std::vector<int64_t> exclusive_scan(const std::vector<int64_t>& v) {
  std::vector<int64_t> out(v.size());
  int64_t sum = 0;
  for (size_t i = 0; i < v.size(); ++i) {
    out[i] = sum;
    sum += v[i];
  }
  return out;
}

// The plan by the device build's steps.  false: cutoff_device_fits or the source limit refused.
bool build_elementwise(const double* y, int64_t M, const double* x, int64_t N, int D, double R, double factor, CutoffPlan& p) {
  p = CutoffPlan();
  if (M > CUTOFF_MAX_SOURCES) return false;
  const bool same = x == y && N == M;
  CutoffExtent e;
  cutoff_extent_init(e);
  {  // two stages, as the reduction: partial extents of blocks of points, then their merge
    const int64_t total = same ? M : M + N, block = 100;
    std::vector<CutoffExtent> part;
    for (int64_t i0 = 0; i0 < total; i0 += block) {
      CutoffExtent q;
      cutoff_extent_init(q);
      for (int64_t i = i0; i < total && i < i0 + block; ++i) cutoff_extent_point(q, i < M ? y + i * D : x + (i - M) * D, D);
      part.push_back(q);
    }
    for (size_t b = part.size(); b-- > 0;) cutoff_extent_merge(e, part[b], D);  // (backwards: the order must not matter)
  }
  const CutoffGridView gv = cutoff_grid_view(e, M, N, D, R, factor);
  if (!cutoff_device_fits(N, M, gv.ncells)) return false;
  for (int d = 0; d < 3; ++d) {
    p.g[d] = gv.g[d];
    p.lo[d] = gv.lo[d];
  }
  p.h = gv.h;
  SortedCloud sc, tc_own;
  sort_cloud(y, M, gv, sc);
  if (!same) sort_cloud(x, N, gv, tc_own);
  const CutoffSorted s = sc.view(), t = same ? sc.view() : tc_own.view();
  const int64_t g0 = gv.g[0], nrows = gv.nrows;

  std::vector<int64_t> rowlen((size_t)nrows + 1, 0), rowtiles((size_t)nrows + 1, 0);
  for (int64_t r = 0; r < nrows; ++r) {
    rowlen[r] = cutoff_row_padded(s.first, g0, r);
    rowtiles[r] = cutoff_row_tiles(t.first, g0, r);
  }
  const std::vector<int64_t> rowbase = exclusive_scan(rowlen), tilebase = exclusive_scan(rowtiles);
  p.m_pad = rowbase[nrows];
  p.m_alloc = p.m_pad + CUTOFF_RECORDS;
  if (p.m_alloc > cutoff_records_bound(M, nrows)) return false;
  p.smap.assign((size_t)p.m_alloc, -1);
  for (int64_t q = 0; q < s.first[gv.ncells]; ++q) p.smap[cutoff_source_record(s, rowbase.data(), g0, q)] = s.idx[q];

  const int64_t cap = cutoff_tiles_bound(N, nrows);
  const int64_t tiles = cutoff_all_tiles(t, tilebase.data(), gv);
  if (tiles > cap) return false;
  std::vector<int64_t> nruns((size_t)cap + 1, 0);
  for (int64_t k = 0; k < cap; ++k) {
    int64_t len_sum;
    const CutoffTileGeom q = cutoff_tile_geom(k, t, tilebase.data(), gv);
    nruns[k] = cutoff_tile_runs(q, s.first, rowbase.data(), gv, nullptr, &len_sum);
    p.walked += q.live * len_sum;
  }
  const std::vector<int64_t> run0 = exclusive_scan(nruns);
  if (run0[cap] > cutoff_runs_bound(N, nrows, D)) return false;
  p.runs.resize((size_t)run0[cap]);
  p.tiles.resize((size_t)tiles);
  p.tmap.resize((size_t)tiles * CUTOFF_TILE);
  for (int64_t k = 0; k < cap; ++k) {
    int64_t len_sum;
    const CutoffTileGeom q = cutoff_tile_geom(k, t, tilebase.data(), gv);
    if (q.kind == CUTOFF_TILE_NONE) continue;
    p.tiles[k].run0 = run0[k];
    p.tiles[k].nruns = cutoff_tile_runs(q, s.first, rowbase.data(), gv, p.runs.data() + run0[k], &len_sum);
    p.tiles[k].live = q.live;
    for (int l = 0; l < CUTOFF_TILE; ++l) p.tmap[k * CUTOFF_TILE + l] = cutoff_tmap_entry(q, t, l);
  }
  p.live_tiles = cutoff_live_tiles(t, tilebase.data(), gv);
  p.n_pad = tiles * CUTOFF_TILE;
  return true;
}

}  // namespace

extern "C" {

// nullptr: refused
void* hc_build(const double* y, long M, const double* x, long N, int D, double R, double factor) {
  kmvp::CutoffPlan* p = new kmvp::CutoffPlan();
  if (!build_elementwise(y, M, x, N, D, R, factor, *p)) {
    delete p;
    return nullptr;
  }
  return p;
}

// cutoff_plan_build on the same input
void* hd_build_host(const double* y, long M, const double* x, long N, int D, double R, double factor) {
  kmvp::CutoffPlan* p = new kmvp::CutoffPlan();
  if (!kmvp::cutoff_plan_build(y, M, x, N, D, R, factor, *p)) {
    delete p;
    return nullptr;
  }
  return p;
}

int hd_fits(long long N, long long M, long long ncells) { return kmvp::cutoff_device_fits(N, M, ncells) ? 1 : 0; }
int hd_key_bits(long long ncells) { return kmvp::cutoff_key_bits(ncells); }
// out[0 .. 3): the bounds on tiles, runs and records the device build allocates for
void hd_bounds(long long N, long long M, long long nrows, int D, int64_t* out) {
  out[0] = kmvp::cutoff_tiles_bound(N, nrows);
  out[1] = kmvp::cutoff_runs_bound(N, nrows, D);
  out[2] = kmvp::cutoff_records_bound(M, nrows);
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
