// C surface of csrc/kmvp_plan.hpp for tests/test_host_plan.py (host compiler only, no HIP).
#include <cstring>

#include "kmvp_plan.hpp"

using namespace kmvp;

static int64_t copy_out(const TileList& l, int* out, int64_t cap) {
  const int64_t G = (int64_t)l.size();
  if (3 * G > cap) return -1;
  if (G > 0) {
    std::memcpy(out, l.start.data(), G * sizeof(int));
    std::memcpy(out + G, l.count.data(), G * sizeof(int));
    std::memcpy(out + 2 * G, l.key.data(), G * sizeof(int));
  }
  return G;
}

extern "C" {

// WAVES_PER_BLOCK, CELL_TILE, CELL_REST_TT, SMALL_PROBLEM_TARGETS, SEG_SPLIT_FROM, MAX_GRID
void hp_constants(int64_t* out) {
  const int64_t v[6] = {WAVES_PER_BLOCK, CELL_TILE, CELL_REST_TT, SMALL_PROBLEM_TARGETS, SEG_SPLIT_FROM, MAX_GRID};
  std::memcpy(out, v, sizeof(v));
}

int hp_settle_segments(int64_t units, int seg) { return settle_segments(units, seg); }

static SegmentRule rule_of(int64_t stage_bytes, int cols, int64_t min_seg, int64_t l2_seg_bytes, int64_t target_blocks) {
  SegmentRule r(stage_bytes, cols);
  r.min_seg = min_seg;
  r.l2_seg_bytes = l2_seg_bytes;
  r.target_blocks = target_blocks;
  return r;
}

// out: n_pad, tile_blocks, m_stages, segments, seg_stages, grid, ok, TT
void hp_plan_stages(int64_t N, int64_t m_stages, int opt_tiles, int tt_max, int tt_default, int opt_segments,
                    int64_t stage_bytes, int64_t min_seg, int64_t l2_seg_bytes, int64_t target_blocks, int cols, int64_t* out) {
  const StagePlan p = plan_stages(N, m_stages, opt_tiles, tt_max, tt_default, opt_segments,
                                  rule_of(stage_bytes, cols, min_seg, l2_seg_bytes, target_blocks));
  const int64_t v[8] = {p.n_pad, p.tile_blocks, p.m_stages, p.segments, p.seg_stages, p.grid, p.ok ? 1 : 0, p.TT};
  std::memcpy(out, v, sizeof(v));
}

// out: m_stages, n_slots, blocks[2], slots[2], seg_stages[2], segments[2]
void hp_cell_split(int64_t N, int64_t m_tiles, int64_t n_main, int64_t n_rest, int tt, int opt_segments, int cols,
                   int stage_tiles, int64_t stage_bytes, int64_t min_seg, int64_t l2_seg_bytes, int64_t target_blocks,
                   int64_t* out) {
  const CellSplit s = cell_split(N, m_tiles, n_main, n_rest, tt, opt_segments, stage_tiles,
                                 rule_of(stage_bytes, cols, min_seg, l2_seg_bytes, target_blocks));
  const int64_t v[10] = {s.m_stages, s.n_slots, s.blocks[0], s.blocks[1], s.slots[0], s.slots[1],
                         s.seg_stages[0], s.seg_stages[1], s.segments[0], s.segments[1]};
  std::memcpy(out, v, sizeof(v));
}

void hp_cell_split_count(const unsigned* keys, int64_t n, int TT, int64_t* n_main, int64_t* n_rest) {
  cell_split_count(keys, n, TT, n_main, n_rest);
}

// the lists as [start][count][key] in out (capacity cap ints); returns the number of tiles, -1: out too small
int64_t hp_cell_tiles_split(const unsigned* keys, int64_t n, int TT, int* out, int64_t cap, int64_t* n_main, int64_t* n_rest) {
  return copy_out(cell_tiles_split(keys, n, TT, n_main, n_rest), out, cap);
}
int64_t hp_cell_tiles(const unsigned* keys, int64_t n, int tile, int* out, int64_t cap) {
  return copy_out(cell_tiles(keys, n, tile), out, cap);
}

// runs of equal keys as (first, count, key) triples in out; returns their number
int64_t hp_key_runs(const unsigned* keys, int64_t n, int64_t* out, int64_t cap) {
  int64_t runs = 0;
  for_each_key_run(keys, n, [&](int64_t first, int64_t count, unsigned key) {
    if (3 * (runs + 1) <= cap) {
      out[3 * runs] = first;
      out[3 * runs + 1] = count;
      out[3 * runs + 2] = key;
    }
    ++runs;
  });
  return runs;
}
}
