// C surface of the fused grid of csrc/kmvp_plan.hpp for tests/test_host_fused_grid.py (host compiler only, no HIP).
#include <cstring>

#include "kmvp_plan.hpp"

using namespace kmvp;

static void put(const CellSplit& s, const FusedCellGrid& g, int64_t* out) {
  const int64_t v[10] = {g.fused ? 1 : 0, g.main_grid, g.rest_grid, g.total, s.grid(0), s.grid(1),
                         s.blocks[0], s.blocks[1], s.segments[0], s.segments[1]};
  std::memcpy(out, v, sizeof(v));
}

extern "C" {

// CELL_REST_TT, WAVES_PER_BLOCK, CELL_TILE, MAX_GRID
void hf_constants(int64_t* out) {
  const int64_t v[4] = {CELL_REST_TT, WAVES_PER_BLOCK, CELL_TILE, MAX_GRID};
  std::memcpy(out, v, sizeof(v));
}

// tiles of the two lists as cell_prepare() counts them, each padded to whole workgroups as cell_tiles_split() builds them
void hf_list_sizes(const unsigned* keys, int64_t n, int TT, int64_t* n_main, int64_t* n_rest) {
  cell_split_count(keys, n, TT, n_main, n_rest);
  *n_main = round_up(*n_main, (int64_t)TT * WAVES_PER_BLOCK);
  *n_rest = round_up(*n_rest, (int64_t)CELL_REST_TT * WAVES_PER_BLOCK);
}

// out: fused, main_grid, rest_grid, total, grid(0), grid(1), blocks[2], segments[2] -- of the split that cell_split() plans
void hf_fused_cell_grid(int64_t N, int64_t m_tiles, int64_t n_main, int64_t n_rest, int tt, int opt_segments, int stage_tiles,
                        int64_t stage_bytes, int64_t min_seg, int64_t l2_seg_bytes, int64_t target_blocks, int opt_fused,
                        int64_t* out) {
  SegmentRule r(stage_bytes, 1);
  r.min_seg = min_seg;
  r.l2_seg_bytes = l2_seg_bytes;
  r.target_blocks = target_blocks;
  const CellSplit s = cell_split(N, m_tiles, n_main, n_rest, tt, opt_segments, stage_tiles, r);
  put(s, fused_cell_grid(s, tt, opt_fused), out);
}

// ... of a split given by its workgroups and segments alone (grids no list of this machine's memory would reach)
void hf_fused_cell_grid_raw(int64_t blocks0, int segments0, int64_t blocks1, int segments1, int tt, int opt_fused, int64_t* out) {
  CellSplit s = {};
  s.blocks[0] = blocks0;
  s.blocks[1] = blocks1;
  s.segments[0] = segments0;
  s.segments[1] = segments1;
  put(s, fused_cell_grid(s, tt, opt_fused), out);
}

// list and local index of workgroups bid0 .. bid0 + n - 1
void hf_fused_cell_work(int64_t bid0, int64_t n, int64_t main_grid, int64_t* list, int64_t* local) {
  for (int64_t i = 0; i < n; ++i) {
    const FusedCellWork w = fused_cell_work(bid0 + i, main_grid);
    list[i] = w.list;
    local[i] = w.local;
  }
}
}
