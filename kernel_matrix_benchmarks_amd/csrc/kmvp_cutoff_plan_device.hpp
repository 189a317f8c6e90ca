// The cell-list plan of the cutoff-radius entries, element by element: the rules of cutoff_plan_build (kmvp_cutoff_plan.hpp)
// restated so that one thread -- or one trip of a serial loop -- forms one entry from sorted keys and scanned counts alone.
// The device build ("cutoff_plan" = 1, kmvp_cutoff_plan_device.hip) runs them in plain kernels between hipcub's radix sort
// and scans; tests/host_cutoff_plan_device_shim.cpp runs the same text with std::stable_sort and serial loops, and holds it
// to cutoff_plan_build entry for entry.
//
//   extent   lo / hi per axis over the points whose coordinates are all finite (both 0 where there is none), then
//            cutoff_grid: h and g
//   key      a point's cell, row-major with axis 0 fastest, as cutoff_plan_build's cell_of; ncells for a point with a
//            non-finite coordinate, which a STABLE sort by key leaves behind everything in the caller's order
//   first    first[c], c = 0 .. ncells: the first sorted position whose key is >= c (first[ncells]: the finite points)
//   rows     a row's records rounded up to CUTOFF_RECORDS and its tiles of CUTOFF_TILE; their exclusive scans over
//            nrows + 1 entries (the last one 0) are rowbase / tilebase, whose last entries are m_pad and the row tiles
//   sources  the sorted source at position p sits in record cell_start(its cell) + (p - first[its cell])
//   tiles    tile t: a row tile (its row by a search in tilebase), a loose tile, a filler or beyond the table; its
//            candidate runs in the host's order (d2 outer, d1 inner)
// 32-bit keys and indices: cutoff_device_fits decides whether a cloud can take this path at all.
//
// Plain C++ with nothing of HIP in it but the KMVP_HD marks.
#pragma once
#include "kmvp_cutoff_plan.hpp"

namespace kmvp {

constexpr int64_t CUTOFF_DEVICE_MAX = 0x7fffffff;  // points per cloud, and keys (ncells + 1 of them)

// What the tables can hold at most, from the sizes the host knows before the build: tiles (a multiple of CUTOFF_WAVES),
// runs and records (the spare batch included).  A row adds at most one partial tile and CUTOFF_RECORDS - 1 pad records.
inline int64_t cutoff_tiles_bound(int64_t N, int64_t nrows) {
  return cutoff_round_up(N / CUTOFF_TILE + (nrows < N ? nrows : N) + 2, CUTOFF_WAVES);
}
inline int64_t cutoff_runs_bound(int64_t N, int64_t nrows, int D) { return cutoff_tiles_bound(N, nrows) * (D >= 3 ? 9 : D == 2 ? 3 : 1); }
inline int64_t cutoff_records_bound(int64_t M, int64_t nrows) {
  return M + (CUTOFF_RECORDS - 1) * (nrows < M ? nrows : M) + 2 * CUTOFF_RECORDS;
}

// Whether the device build's 32-bit keys, indices and item counts hold this cloud -- the points of either cloud, the keys
// 0 .. ncells and the entries of its longest scan (one per tile the table may hold; a grid has at most ncells rows) --;
// the host build runs where they do not.
inline bool cutoff_device_fits(int64_t N, int64_t M, int64_t ncells) {
  return N <= CUTOFF_DEVICE_MAX && M <= CUTOFF_DEVICE_MAX && ncells <= CUTOFF_DEVICE_MAX - 1 &&
         cutoff_tiles_bound(N, ncells) + 1 <= CUTOFF_DEVICE_MAX;
}

// The low bits of a key the sort has to look at: the smallest b >= 1 with 2^b > ncells.
inline int cutoff_key_bits(int64_t ncells) {
  int b = 1;
  while (b < 32 && ((int64_t)1 << b) <= ncells) ++b;
  return b;
}

struct CutoffExtent {
  double lo[3], hi[3];
  int64_t any;
};

KMVP_HD inline void cutoff_extent_init(CutoffExtent& e) {
  for (int d = 0; d < 3; ++d) e.lo[d] = e.hi[d] = 0.0;
  e.any = 0;
}

// cutoff_plan_build's update for one point p (D doubles)
KMVP_HD inline void cutoff_extent_point(CutoffExtent& e, const double* p, int D) {
  if (!cutoff_point_finite(p, D)) return;
  for (int d = 0; d < D; ++d) {
    if (!e.any || p[d] < e.lo[d]) e.lo[d] = p[d];
    if (!e.any || p[d] > e.hi[d]) e.hi[d] = p[d];
  }
  e.any = 1;
}

// ... and for the extent of a set of points: minima and maxima, so the order of the merges does not matter
KMVP_HD inline void cutoff_extent_merge(CutoffExtent& e, const CutoffExtent& o, int D) {
  if (!o.any) return;
  for (int d = 0; d < D; ++d) {
    if (!e.any || o.lo[d] < e.lo[d]) e.lo[d] = o.lo[d];
    if (!e.any || o.hi[d] > e.hi[d]) e.hi[d] = o.hi[d];
  }
  e.any = 1;
}

struct CutoffGridView {
  int D;
  int64_t g[3];
  double lo[3];
  double h;
  int64_t ncells, nrows;
};

inline CutoffGridView cutoff_grid_view(const CutoffExtent& e, int64_t M, int64_t N, int D, double R, double factor) {
  CutoffGridView gv;
  gv.D = D;
  for (int d = 0; d < 3; ++d) gv.lo[d] = e.lo[d];
  cutoff_grid(e.lo, e.hi, M, N, D, R, factor, gv.h, gv.g);
  gv.ncells = gv.g[0] * gv.g[1] * gv.g[2];
  gv.nrows = gv.g[1] * gv.g[2];
  return gv;
}

// The key of a point p (D doubles).
KMVP_HD inline uint32_t cutoff_point_key(const double* p, const CutoffGridView& gv) {
  if (!cutoff_point_finite(p, gv.D)) return (uint32_t)gv.ncells;
  int64_t c = 0;
  for (int d = gv.D - 1; d >= 0; --d) c = c * gv.g[d] + cutoff_cell_of(p[d], gv.lo[d], gv.h, gv.g[d]);
  return (uint32_t)c;
}

// A cloud sorted by key: keys and caller indices in sorted order, and first[0 .. ncells].
struct CutoffSorted {
  const uint32_t* keys;
  const int32_t* idx;
  const int32_t* first;
  int64_t n;
};

// The first position in keys[0 .. n) whose key is >= key (n: none).
KMVP_HD inline int32_t cutoff_lower_bound(const uint32_t* keys, int64_t n, uint32_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return (int32_t)lo;
}

KMVP_HD inline int64_t cutoff_row_count(const int32_t* first, int64_t g0, int64_t r) {
  return (int64_t)first[(r + 1) * g0] - (int64_t)first[r * g0];
}
// A row's padded length in records, and its tiles.
KMVP_HD inline int64_t cutoff_row_padded(const int32_t* first, int64_t g0, int64_t r) {
  return cutoff_round_up(cutoff_row_count(first, g0, r), CUTOFF_RECORDS);
}
KMVP_HD inline int64_t cutoff_row_tiles(const int32_t* first, int64_t g0, int64_t r) {
  return (cutoff_row_count(first, g0, r) + CUTOFF_TILE - 1) / CUTOFF_TILE;
}

// cutoff_plan_build's cstart[c] and cend[c] from the sources' first[] and the scanned row lengths.
KMVP_HD inline int64_t cutoff_cell_start(const int32_t* sfirst, const int64_t* rowbase, int64_t g0, int64_t c) {
  const int64_t r = c / g0;
  return rowbase[r] + ((int64_t)sfirst[c] - (int64_t)sfirst[r * g0]);
}
KMVP_HD inline int64_t cutoff_cell_end(const int32_t* sfirst, const int64_t* rowbase, int64_t g0, int64_t c) {
  return cutoff_cell_start(sfirst, rowbase, g0, c) + ((int64_t)sfirst[c + 1] - (int64_t)sfirst[c]);
}

// The record of the sorted source at position p < first[ncells].
KMVP_HD inline int64_t cutoff_source_record(const CutoffSorted& s, const int64_t* rowbase, int64_t g0, int64_t p) {
  const int64_t c = (int64_t)s.keys[p];
  return cutoff_cell_start(s.first, rowbase, g0, c) + (p - (int64_t)s.first[c]);
}

enum { CUTOFF_TILE_ROW = 0, CUTOFF_TILE_LOOSE = 1, CUTOFF_TILE_FILLER = 2, CUTOFF_TILE_NONE = 3 };

struct CutoffTileGeom {
  int kind;       // CUTOFF_TILE_*
  int32_t live;   // lanes that own a target
  int64_t row;    // ROW: its row of cells,
  int64_t a, b;   //      the cells [a, b] of a neighbouring row its runs cover
  int64_t s0;     // ROW, LOOSE: sorted position of lane 0's target
};

// Tiles of the table: those with a live lane, and all of them (whole workgroups).
KMVP_HD inline int64_t cutoff_live_tiles(const CutoffSorted& t, const int64_t* tilebase, const CutoffGridView& gv) {
  const int64_t loose = t.n - (int64_t)t.first[gv.ncells];
  return tilebase[gv.nrows] + (loose + CUTOFF_TILE - 1) / CUTOFF_TILE;
}
KMVP_HD inline int64_t cutoff_all_tiles(const CutoffSorted& t, const int64_t* tilebase, const CutoffGridView& gv) {
  return cutoff_round_up(cutoff_live_tiles(t, tilebase, gv), CUTOFF_WAVES);
}

// Tile t >= 0: its kind, row, live, a and b.
KMVP_HD inline CutoffTileGeom cutoff_tile_geom(int64_t t, const CutoffSorted& tg, const int64_t* tilebase, const CutoffGridView& gv) {
  CutoffTileGeom q;
  q.kind = CUTOFF_TILE_NONE;
  q.live = 0;
  q.row = q.a = q.b = q.s0 = 0;
  const int64_t g0 = gv.g[0];
  const int64_t row_tiles = tilebase[gv.nrows], finite = (int64_t)tg.first[gv.ncells];
  const int64_t live_tiles = cutoff_live_tiles(tg, tilebase, gv);
  if (t < row_tiles) {
    // the row r with tilebase[r] <= t < tilebase[r + 1]: rows without a tile are stepped over
    int64_t lo = 0, hi = gv.nrows;
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (tilebase[mid] <= t) lo = mid;
      else hi = mid;
    }
    q.kind = CUTOFF_TILE_ROW;
    q.row = lo;
    q.s0 = (int64_t)tg.first[lo * g0] + (t - tilebase[lo]) * CUTOFF_TILE;
    const int64_t left = (int64_t)tg.first[(lo + 1) * g0] - q.s0;
    q.live = (int32_t)(left < CUTOFF_TILE ? left : CUTOFF_TILE);
    const int64_t cf = (int64_t)tg.keys[q.s0] - lo * g0, cl = (int64_t)tg.keys[q.s0 + q.live - 1] - lo * g0;
    q.a = cf > 0 ? cf - 1 : 0;
    q.b = cl + 1 < g0 ? cl + 1 : g0 - 1;
  } else if (t < live_tiles) {
    q.kind = CUTOFF_TILE_LOOSE;
    q.s0 = finite + (t - row_tiles) * CUTOFF_TILE;
    const int64_t left = tg.n - q.s0;
    q.live = (int32_t)(left < CUTOFF_TILE ? left : CUTOFF_TILE);
  } else if (t < cutoff_round_up(live_tiles, CUTOFF_WAVES)) {
    q.kind = CUTOFF_TILE_FILLER;
  }
  return q;
}

// A tile's candidate runs in cutoff_plan_build's order, those without a record dropped: their number, the sum of their
// lengths in *len_sum, and the runs themselves in out[0 .. number) unless out is null.
KMVP_HD inline int32_t cutoff_tile_runs(const CutoffTileGeom& q, const int32_t* sfirst, const int64_t* rowbase, const CutoffGridView& gv,
                                        CutoffRun* out, int64_t* len_sum) {
  *len_sum = 0;
  if (q.kind != CUTOFF_TILE_ROW) return 0;
  const int64_t g0 = gv.g[0], g1 = gv.g[1], g2 = gv.g[2];
  const int64_t r1 = q.row % g1, r2 = q.row / g1;
  int32_t n = 0;
  for (int64_t d2 = -1; d2 <= 1; ++d2) {
    for (int64_t d1 = -1; d1 <= 1; ++d1) {
      const int64_t n1 = r1 + d1, n2 = r2 + d2;
      if (n1 < 0 || n1 >= g1 || n2 < 0 || n2 >= g2) continue;
      const int64_t row = n1 + g1 * n2;
      const int64_t s = cutoff_cell_start(sfirst, rowbase, g0, row * g0 + q.a), e = cutoff_cell_end(sfirst, rowbase, g0, row * g0 + q.b);
      if (e <= s) continue;  // no record in reach in this row
      CutoffRun run;
      run.rec0 = s / CUTOFF_RECORDS * CUTOFF_RECORDS;
      run.len = (int32_t)(cutoff_round_up(e, CUTOFF_RECORDS) - run.rec0);
      run.zero = 0;
      if (out) out[n] = run;
      *len_sum += run.len;
      ++n;
    }
  }
  return n;
}

// The caller's target index in lane `lane` of a tile, -1 behind its live lanes.
KMVP_HD inline int64_t cutoff_tmap_entry(const CutoffTileGeom& q, const CutoffSorted& tg, int lane) {
  return lane < q.live ? (int64_t)tg.idx[q.s0 + lane] : (int64_t)-1;
}

}  // namespace kmvp
