// C surface of the TAIL list of csrc/kmvp_plan.hpp for tests/test_host_cell_tail.py (host compiler only, no HIP).
#include <cstring>

#include "kmvp_plan.hpp"

using namespace kmvp;

extern "C" {

// CELL_TAIL_MAX_SEGMENTS, CELL_REST_TT, WAVES_PER_BLOCK, CELL_TILE, CELL_TAIL_AUTO
void ht_constants(int64_t* out) {
  const int64_t v[5] = {CELL_TAIL_MAX_SEGMENTS, CELL_REST_TT, WAVES_PER_BLOCK, CELL_TILE, CELL_TAIL_AUTO ? 1 : 0};
  std::memcpy(out, v, sizeof(v));
}

// tiles of the lists of count-cut cells on sorted fine keys (cell_prepare's calls): source tiles, n_main, n_rest
void ht_count_cut_lists(const unsigned* fine, int64_t n, int cap, int tt, int64_t* m_tiles, int64_t* n_main, int64_t* n_rest) {
  const int64_t quantum = (int64_t)CELL_TILE * tt;
  const auto cells = count_cut_cells(fine, n, cap, quantum, quantum * WAVES_PER_BLOCK);
  *m_tiles = (int64_t)count_cell_source_tiles(cells).size();
  count_cell_target_tiles(cells, tt, n_main, n_rest);
}

// out: b_full, b_tail, segments, seg_stages of cell_tail_plan()
void ht_tail_plan(int64_t B, int S, int64_t R, int64_t m_stages, int64_t rest_grid, int64_t min_seg, int64_t* out) {
  const CellTail t = cell_tail_plan(B, S, R, m_stages, rest_grid, min_seg);
  const int64_t v[4] = {t.b_full, t.b_tail, t.segments, t.seg_stages};
  std::memcpy(out, v, sizeof(v));
}

int ht_tail_taken(int opt, int tt, int fused, int64_t N, int64_t M) { return cell_tail_taken(opt, tt, fused != 0, N, M) ? 1 : 0; }

// The lists as run_product_cellmm plans them: cell_split(), fused_cell_grid(), and -- where the launch is fused and
// take_tail says so -- cell_tail_split().  out: tail (0 / 1), fused, main_grid, tail_grid, rest_grid, total, m_stages, n_slots,
// then per list r = 0, 1, 2: blocks, segments, seg_stages, slots, slot_base, region_offset (one column), and part_doubles
void ht_lists(int64_t N, int64_t m_tiles, int64_t n_main, int64_t n_rest, int tt, int opt_segments, int stage_tiles,
              int64_t stage_bytes, int64_t min_seg, int64_t l2_seg_bytes, int64_t target_blocks, int opt_fused, int take_tail,
              int64_t resident, int64_t* out) {
  SegmentRule r(stage_bytes, 1);
  r.min_seg = min_seg;
  r.l2_seg_bytes = l2_seg_bytes;
  r.target_blocks = target_blocks;
  CellSplit s = cell_split(N, m_tiles, n_main, n_rest, tt, opt_segments, stage_tiles, r);
  FusedCellGrid g = fused_cell_grid(s, tt, opt_fused);
  bool tail = false;
  if (take_tail && cell_tail_taken(1, tt, g.fused, N, N)) {
    tail = cell_tail_split(s, tt, resident, small_problem(N) ? 1 : min_seg);
    g = fused_cell_grid(s, tt, opt_fused);
  }
  int64_t* o = out;
  *o++ = tail ? 1 : 0;
  *o++ = g.fused ? 1 : 0;
  *o++ = g.main_grid;
  *o++ = g.tail_grid;
  *o++ = g.rest_grid;
  *o++ = g.total;
  *o++ = s.m_stages;
  *o++ = s.n_slots;
  for (int l = 0; l < CELL_LISTS; ++l) {
    *o++ = s.blocks[l];
    *o++ = s.segments[l];
    *o++ = s.seg_stages[l];
    *o++ = s.slots[l];
    *o++ = s.slot_base(l);
    *o++ = (int64_t)s.region_offset(1, l);
  }
  *o++ = (int64_t)s.part_doubles(1);
}

// list and local index of workgroups bid0 .. bid0 + n - 1 of the fused grid
void ht_fused_cell_work(int64_t bid0, int64_t n, int64_t main_grid, int64_t tail_grid, int64_t* list, int64_t* local) {
  for (int64_t i = 0; i < n; ++i) {
    const FusedCellWork w = fused_cell_work(bid0 + i, main_grid, tail_grid);
    list[i] = w.list;
    local[i] = w.local;
  }
}
}
