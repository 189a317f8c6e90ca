// Cell list and launch plan of the cutoff-radius entries (include/kmvp.h kmvp_<kernel>_cutoff, kmvp_radius_count; kernels:
// kmvp_lowd_cutoff.hpp).
//
// A pair (target, source) counts when its squared distance, in the working precision, is <= (real)(R R).  The plan sorts
// both clouds into the cells of a regular grid of side h >= R (1 + 2^-16) so that a wave of 64 targets has to walk the
// sources of neighbouring cells only:
//  * cell side: h = factor R (1 + 2^-16), the same along every axis, enlarged until no axis has more than 2^20 cells and
//    the grid no more than max(1, 2 (N + M)) -- a larger h is always correct.  The margin 2^-16 is there because the
//    device decides "inside" in the working precision: the float32 chain of s is off by (D + 2) 2^-24 relatively, so a
//    pair the device may call inside is closer than R (1 + 2^-17) and never sits two cells apart.
//  * cell index: floor((v - lo) / h) per axis in double -- monotone in v -- with lo the minimum over the points of both
//    clouds whose coordinates are all finite; cells are numbered row-major with axis 0 fastest, and a ROW is the g[0]
//    cells that share their indices along axes 1 and 2.
//  * sources: counting-sorted by cell (ties in the caller's order).  Every row is padded to a multiple of
//    CUTOFF_RECORDS = 8 records (the family's pad records: y = +inf, b = 0), and the array carries one spare batch of 8 at
//    its end: the ping-pong prefetch of the scalar-cache feed reads 4 records past the run it consumes.  A source with a
//    NaN or infinite coordinate is in no cell and in no record.
//  * targets: counting-sorted by cell and cut into wave tiles of up to CUTOFF_TILE = 64 consecutive targets of ONE row --
//    a tile never straddles rows, and lanes stay full when cells hold few points.  Targets with a non-finite coordinate
//    sit in tiles of their own, behind the others, that own no run.  Filler tiles (no live lane, no run) round the table
//    up to whole workgroups.
//  * runs: a tile owns one run per neighbouring row (up to 3^(D-1)) that holds a record of the cells
//    [first cell of the tile - 1, last cell + 1]: those records, the start rounded down and the end rounded up to
//    multiples of 8 -- inside the padded row, which starts and ends on one.  Rounding is harmless: the distance test
//    decides membership.  Runs of one tile lie in different rows, so they are pairwise disjoint, and together they hold
//    every source within one cell of any of the tile's targets along every axis.
// One CutoffTile per wave tile and one CutoffRun per run, 16 bytes each, both read through the scalar cache; tmap / smap are
// the padded -> caller index maps (-1: a pad) of the gather-pack kernels and of the kernels' epilogue.
//
// Plain C++ with nothing of HIP in it: the same text compiles into kmvp_cutoff.hip and, with a host compiler alone, into
// tests/test_host_cutoff_plan.py.  cutoff_plan_build is the host build and the definition of the plan; the device build
// ("cutoff_plan" = 1, kmvp_cutoff_plan_device.hpp) shares cutoff_grid and the per-element rules marked KMVP_HD, and has to
// produce the same plan entry for entry.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#include "kmvp_radius_knn_list.hpp"  // KMVP_HD: the per-element rules below also run in the device build's kernels

namespace kmvp {

constexpr int CUTOFF_TILE = 64;                // targets per wave tile: one per lane
constexpr int CUTOFF_WAVES = 4;                // wave tiles per workgroup (WAVES_PER_BLOCK of the pair-loop kernels)
constexpr int64_t CUTOFF_RECORDS = 8;          // source records per ping-pong round: runs are multiples of it
constexpr int64_t CUTOFF_MAX_AXIS = 1 << 20;   // cells along one axis
constexpr int64_t CUTOFF_MAX_SOURCES = 0x7fffffff - 15;  // a run is at most the padded sources: its length fits 32 bits

struct CutoffTile {
  int64_t run0;   // first run of the tile in the run table
  int32_t nruns;  // its runs: 0 .. 3^(D-1)
  int32_t live;   // lanes that own a target (0 .. CUTOFF_TILE)
};
struct CutoffRun {
  int64_t rec0;  // first record: a multiple of CUTOFF_RECORDS
  int32_t len;   // records: a positive multiple of CUTOFF_RECORDS
  int32_t zero;
};
static_assert(sizeof(CutoffTile) == 16 && sizeof(CutoffRun) == 16, "table entries are 16 bytes");

struct CutoffPlan {
  int64_t g[3] = {1, 1, 1};         // cells per axis (1 for unused axes)
  double lo[3] = {0.0, 0.0, 0.0};   // grid origin
  double h = 0.0;                   // cell side
  int64_t n_pad = 0;                // target slots: tiles.size() * CUTOFF_TILE, whole workgroups
  int64_t m_pad = 0;                // records of all rows
  int64_t m_alloc = 0;              // m_pad + the spare batch: records the array holds
  int64_t live_tiles = 0;           // tiles with a live lane
  int64_t walked = 0;               // sum over the tiles of live x (records of its runs)
  std::vector<CutoffTile> tiles;
  std::vector<CutoffRun> runs;
  std::vector<int64_t> tmap;  // [n_pad]   target slot -> caller's target index, -1 for a pad
  std::vector<int64_t> smap;  // [m_alloc] record      -> caller's source index, -1 for a pad
};

KMVP_HD inline int64_t cutoff_round_up(int64_t v, int64_t q) { return (v + q - 1) / q * q; }

KMVP_HD inline bool cutoff_point_finite(const double* p, int D) {
  for (int d = 0; d < D; ++d)
    if (!std::isfinite(p[d])) return false;
  return true;
}

inline int64_t cutoff_axis_cells(double ext, double h) {
  const double q = std::floor(ext / h);
  if (!(q < (double)CUTOFF_MAX_AXIS)) return CUTOFF_MAX_AXIS;  // (also a NaN quotient; the caller's h rules it out)
  return (int64_t)q + 1;
}

KMVP_HD inline int64_t cutoff_cell_of(double v, double lo, double h, int64_t g) {
  const double q = std::floor((v - lo) / h);
  if (!(q > 0.0)) return 0;
  if (!(q < (double)g)) return g - 1;
  return (int64_t)q;
}

// The grid rule, stated once for the host build below and the device build (kmvp_cutoff_plan_device.hpp): the cell side h
// and the cells per axis g for the extent [lo, hi] of the finite points (both 0 where there is none), D <= 3.
inline void cutoff_grid(const double* lo, const double* hi, int64_t M, int64_t N, int D, double R, double factor, double& h_out,
                        int64_t* g) {
  double ext[3] = {0.0, 0.0, 0.0};
  for (int d = 0; d < D; ++d) ext[d] = hi[d] - lo[d];  // (may overflow to inf: the caps below take care of it)
  double h = factor * R * (1.0 + 1.0 / 65536.0);
  for (int d = 0; d < D; ++d) {
    if (!(ext[d] / h < (double)(CUTOFF_MAX_AXIS - 1))) {
      const double need = ext[d] / (double)(CUTOFF_MAX_AXIS - 1);
      if (need > h) h = need;
    }
  }
  if (!std::isfinite(h)) h = INFINITY;
  const int64_t cap = 2 * (N + M) > 1 ? 2 * (N + M) : 1;
  for (;;) {
    for (int d = 0; d < 3; ++d) g[d] = d < D ? cutoff_axis_cells(ext[d], h) : 1;
    if (g[0] * g[1] * g[2] <= cap || !std::isfinite(h)) break;
    h *= 1.25;
  }
  if (!std::isfinite(h))
    for (int d = 0; d < 3; ++d) g[d] = 1;
  h_out = h;
}

// The plan for sources y (M, D) and targets x (N, D), row-major doubles (x may be y), D <= 3, a finite radius R > 0 and a
// cell factor >= 1.  false: more than CUTOFF_MAX_SOURCES sources; the plan is then unusable.
inline bool cutoff_plan_build(const double* y, int64_t M, const double* x, int64_t N, int D, double R, double factor, CutoffPlan& p) {
  p = CutoffPlan();
  if (M > CUTOFF_MAX_SOURCES) return false;
  // ---- the grid
  double hi[3] = {0.0, 0.0, 0.0};
  bool any = false;
  for (int pass = 0; pass < 2; ++pass) {
    const double* q = pass ? x : y;
    const int64_t n = pass ? N : M;
    for (int64_t i = 0; i < n; ++i) {
      if (!cutoff_point_finite(q + i * D, D)) continue;
      for (int d = 0; d < D; ++d) {
        const double v = q[i * D + d];
        if (!any || v < p.lo[d]) p.lo[d] = v;
        if (!any || v > hi[d]) hi[d] = v;
      }
      any = true;
    }
  }
  cutoff_grid(p.lo, hi, M, N, D, R, factor, p.h, p.g);
  const double h = p.h;
  const int64_t g0 = p.g[0], g1 = p.g[1], g2 = p.g[2];
  const int64_t ncells = g0 * g1 * g2, nrows = g1 * g2;
  auto cell_of = [&](const double* q) {
    int64_t c = 0;
    for (int d = D - 1; d >= 0; --d) c = c * p.g[d] + cutoff_cell_of(q[d], p.lo[d], h, p.g[d]);
    return c;
  };

  // ---- sources: counting sort by cell, every row padded to whole rounds of records
  std::vector<int64_t> scell((size_t)M), cstart((size_t)ncells), cend((size_t)ncells);
  std::vector<int64_t> count((size_t)ncells, 0);
  for (int64_t j = 0; j < M; ++j) {
    scell[j] = cutoff_point_finite(y + j * D, D) ? cell_of(y + j * D) : -1;
    if (scell[j] >= 0) ++count[scell[j]];
  }
  int64_t pos = 0;
  for (int64_t r = 0; r < nrows; ++r) {
    for (int64_t c = r * g0; c < (r + 1) * g0; ++c) {
      cstart[c] = pos;
      pos += count[c];
      cend[c] = pos;
    }
    pos = cutoff_round_up(pos, CUTOFF_RECORDS);
  }
  p.m_pad = pos;
  p.m_alloc = pos + CUTOFF_RECORDS;
  p.smap.assign((size_t)p.m_alloc, -1);
  {
    std::vector<int64_t> fill(cstart);
    for (int64_t j = 0; j < M; ++j)
      if (scell[j] >= 0) p.smap[fill[scell[j]]++] = j;
  }

  // ---- targets: counting sort by cell, tiles of up to 64 consecutive targets of one row, their runs
  std::vector<int64_t> tcell((size_t)N), order, loose;
  std::vector<int64_t> tstart((size_t)ncells + 1, 0);
  for (int64_t i = 0; i < N; ++i) {
    tcell[i] = cutoff_point_finite(x + i * D, D) ? cell_of(x + i * D) : -1;
    if (tcell[i] >= 0) ++tstart[tcell[i] + 1];
    else loose.push_back(i);
  }
  for (int64_t c = 0; c < ncells; ++c) tstart[c + 1] += tstart[c];
  order.resize((size_t)tstart[ncells]);
  {
    std::vector<int64_t> fill(tstart.begin(), tstart.end() - 1);
    for (int64_t i = 0; i < N; ++i)
      if (tcell[i] >= 0) order[fill[tcell[i]]++] = i;
  }
  auto push_tile = [&](const int64_t* idx, int64_t live, int64_t run0, int64_t nruns) {
    CutoffTile t;
    t.run0 = run0;
    t.nruns = (int32_t)nruns;
    t.live = (int32_t)live;
    p.tiles.push_back(t);
    for (int64_t l = 0; l < CUTOFF_TILE; ++l) p.tmap.push_back(l < live ? idx[l] : (int64_t)-1);
  };
  for (int64_t r = 0; r < nrows; ++r) {
    const int64_t t0 = tstart[r * g0], t1 = tstart[(r + 1) * g0];
    const int64_t r1 = r % g1, r2 = r / g1;
    for (int64_t s0 = t0; s0 < t1; s0 += CUTOFF_TILE) {
      const int64_t live = t1 - s0 < CUTOFF_TILE ? t1 - s0 : CUTOFF_TILE;
      const int64_t cf = tcell[order[s0]] - r * g0, cl = tcell[order[s0 + live - 1]] - r * g0;
      const int64_t a = cf > 0 ? cf - 1 : 0, b = cl + 1 < g0 ? cl + 1 : g0 - 1;
      const int64_t run0 = (int64_t)p.runs.size();
      int64_t len_sum = 0;
      for (int64_t d2 = -1; d2 <= 1; ++d2) {
        for (int64_t d1 = -1; d1 <= 1; ++d1) {
          const int64_t n1 = r1 + d1, n2 = r2 + d2;
          if (n1 < 0 || n1 >= g1 || n2 < 0 || n2 >= g2) continue;
          const int64_t row = n1 + g1 * n2;
          const int64_t s = cstart[row * g0 + a], e = cend[row * g0 + b];
          if (e <= s) continue;  // no record in reach in this row
          CutoffRun run;
          run.rec0 = s / CUTOFF_RECORDS * CUTOFF_RECORDS;
          run.len = (int32_t)(cutoff_round_up(e, CUTOFF_RECORDS) - run.rec0);
          run.zero = 0;
          p.runs.push_back(run);
          len_sum += run.len;
        }
      }
      push_tile(order.data() + s0, live, run0, (int64_t)p.runs.size() - run0);
      p.walked += live * len_sum;
    }
  }
  for (size_t s0 = 0; s0 < loose.size(); s0 += CUTOFF_TILE) {
    const int64_t left = (int64_t)(loose.size() - s0);
    push_tile(loose.data() + s0, left < CUTOFF_TILE ? left : CUTOFF_TILE, (int64_t)p.runs.size(), 0);
  }
  p.live_tiles = (int64_t)p.tiles.size();
  while (p.tiles.size() % CUTOFF_WAVES) push_tile(nullptr, 0, (int64_t)p.runs.size(), 0);
  p.n_pad = (int64_t)p.tiles.size() * CUTOFF_TILE;
  return true;
}

}  // namespace kmvp
