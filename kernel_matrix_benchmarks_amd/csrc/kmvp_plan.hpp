// Launch plans of the product: how (N, M, stage size) become padded sizes, segments and a grid, and how sorted cell keys
// become tile lists.  Pure functions of numbers -- no HIP, no context -- so that they compile into kmvp_product.hip and,
// with a host compiler alone, into tests/test_host_plan.py.  The segment count decides the order of the fp64 partial sums
// (bitwise results) and the L2 behaviour (speed); the tile lists are what the cell kernels index without a bounds check.
// Cells are the lattice's (one key per cell, cell_tiles / cell_tiles_split) or, under the "cell_balance" option, columns of
// the lattice cut along z by point count (count_cut_cells and the two list builders behind it, at the end of this file).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace kmvp {

constexpr int WAVES_PER_BLOCK = 4;
constexpr int CELL_TILE = 32;                     // points per tile of the float32 cell lists
constexpr int CELL_REST_TT = 2;                   // tiles per wavefront of the cell kernels' REST list (the cells' leftover tiles)
constexpr int STAGED_TILE = 32;                   // targets per tile of the staged matrix-core paths (FAST_TILE)
constexpr int64_t SMALL_PROBLEM_TARGETS = 32768;  // below: one target tile per wave, one stage per segment
constexpr int SEG_SPLIT_FROM = 16;                // segments from which the reductions split a sum over SEG_SPLIT lanes
constexpr int64_t MAX_GRID = 0x7fffffff;          // workgroups of one launch

inline int64_t round_up(int64_t v, int64_t q) { return (v + q - 1) / q * q; }
// Few targets (the reference's own datasets have n <= 1e4): one tile per wave and segments of a single stage spread a
// launch over more CUs; from ~3e4 targets on the big tiles win, in longer segments.
inline bool small_problem(int64_t N) { return N < SMALL_PROBLEM_TARGETS; }

// ---- segments ----------------------------------------------------------------------------------------------------

// What a path decides about its segments; everything else follows from the problem's size.
struct SegmentRule {
  int64_t stage_bytes;               // bytes of source image per unit (a stage, a record)
  int cols;                          // columns of fp64 partial sums per segment
  int64_t min_seg = 1;               // shortest segment, in units (the staged and cell plans: on big problems)
  bool small = false;                // few targets: about two rounds of resident blocks (4096 workgroups) are aimed at
  int64_t l2_seg_bytes = 2 << 20;    // L2 budget of one segment
  int64_t target_blocks = 16384;     // workgroups aimed at otherwise
  SegmentRule(int64_t stage_bytes_, int cols_) : stage_bytes(stage_bytes_), cols(cols_) {}
};

// Number of source segments of a launch (specialised kernels).  Three pulls:
//  * L2 residency: with segments % 8 == 0 each XCD streams one segment at a time
//    (block_to_work), so a segment of <= 2 MiB of records stays in its 4 MiB L2;
//  * parallelism: tile_blocks * segments should be many rounds of the 2048 resident
//    blocks (256 CUs x 8), which only matters when there are few target tiles;
//  * the fp64 partial buffer segments * cols * n_pad * 8 bytes stays bounded.
// opt_segments > 0 (the "segments" option) overrides the rule.
inline int choose_segments(int opt_segments, int64_t tile_blocks, int64_t units, int64_t n_pad, const SegmentRule& r) {
  int64_t seg;
  if (opt_segments > 0) {
    seg = opt_segments;
  } else {
    seg = 8 * std::max<int64_t>(1, (units * r.stage_bytes + 8 * r.l2_seg_bytes - 1) / (8 * r.l2_seg_bytes));
    const int64_t target_blocks = r.small ? 4096 : r.target_blocks;  // small problems: about two rounds of resident blocks
    const int64_t for_parallelism = (target_blocks + tile_blocks - 1) / tile_blocks;
    if (for_parallelism > seg) seg = (for_parallelism + 7) / 8 * 8;
    const int64_t cap_len = std::max<int64_t>(1, units / r.min_seg);  // segment >= min_seg units
    const int64_t cap_mem = std::max<int64_t>(1, (int64_t)(4e9 / ((double)r.cols * n_pad * 8)));
    seg = std::min(seg, std::min(cap_len, cap_mem));
    if (seg >= 8) seg = seg / 8 * 8;
  }
  seg = std::max<int64_t>(1, std::min<int64_t>(seg, 65535));
  return (int)seg;
}

// Segments are whole numbers of `units` (stages, tiles): `seg` requested segments become ceil(units / ceil(units / seg)),
// which may be one or two fewer -- and no longer a multiple of 8.  block_to_work() streams one segment per XCD at a time only
// when the count IS a multiple of 8 (measured, cfast_kernel at 2e5 points: 23 segments 5.65 ms, 16: 5.05, 32: 4.94), so the
// nearest multiple of 8 that survives the rounding is taken (the request itself below 8).
inline int settle_segments(int64_t units, int seg) {
  auto settled = [&](int64_t cand) { return (units + (units + cand - 1) / cand - 1) / ((units + cand - 1) / cand); };
  if (seg >= 8 && units >= 8)
    for (int step = 0; step <= 64; step += 8)
      for (int64_t cand : {(int64_t)seg + step, (int64_t)seg - step})
        if (cand >= 8 && cand <= units && cand % 8 == 0 && settled(cand) == cand) return (int)cand;
  seg = (int)std::max<int64_t>(1, std::min<int64_t>(seg, std::max<int64_t>(units, 1)));
  return (int)settled(seg);
}

// segments of whole stages: the rule's choice, settled
inline int stage_segments(int opt_segments, int64_t tile_blocks, int64_t m_stages, int64_t n_pad, const SegmentRule& r) {
  return settle_segments(m_stages, choose_segments(opt_segments, tile_blocks, m_stages, n_pad, r));
}

// ---- the staged matrix-core paths (fast, fastmm, cfast, cfastmm) -----------------------------------------------------

// Targets in workgroups of WAVES_PER_BLOCK wavefronts x TT tiles of 32; sources in m_stages stages, cut into segments of
// seg_stages stages; one workgroup per (target block, segment).  ok == false: more workgroups than a launch takes.
// TT: as requested (opt_tiles > 0, the "fast_tiles" option) up to tt_max, else 1 for few targets, else tt_default.
// Segments: r with single stages for few targets, at least r.min_seg stages otherwise.
struct StagePlan {
  int64_t n_pad, tile_blocks, m_stages, seg_stages, grid;
  int TT, segments;
  bool ok;
};
inline StagePlan plan_stages(int64_t N, int64_t m_stages, int opt_tiles, int tt_max, int tt_default, int opt_segments,
                             SegmentRule r) {
  StagePlan p;
  r.small = small_problem(N);
  if (r.small) r.min_seg = 1;
  p.TT = opt_tiles > 0 ? std::min(opt_tiles, tt_max) : (r.small ? 1 : std::min(tt_default, tt_max));
  const int64_t tile = (int64_t)STAGED_TILE * p.TT * WAVES_PER_BLOCK;
  p.n_pad = round_up(N, tile);
  p.tile_blocks = p.n_pad / tile;
  p.m_stages = m_stages;
  p.segments = stage_segments(opt_segments, p.tile_blocks, m_stages, p.n_pad, r);
  p.seg_stages = (m_stages + p.segments - 1) / p.segments;
  p.grid = p.tile_blocks * p.segments;
  p.ok = p.grid <= MAX_GRID;
  return p;
}

// ---- tile lists of the cell paths -------------------------------------------------------------------------------------

// f(first, count, key) for every run of equal keys in the sorted sequence
template <class F>
void for_each_key_run(const unsigned* keys, int64_t n, F&& f) {
  for (int64_t p = 0; p < n;) {
    int64_t e = p + 1;
    while (e < n && keys[e] == keys[p]) ++e;
    f(p, e - p, keys[p]);
    p = e;
  }
}

// A list of tiles: [start][count][key] per tile, the device layout being the three arrays one after the other.
struct TileList {
  std::vector<int> start, count;
  std::vector<unsigned> key;
  size_t size() const { return start.size(); }
  void reserve(size_t tiles) {
    start.reserve(tiles);
    count.reserve(tiles);
    key.reserve(tiles);
  }
  // `live` tiles of <= tile points covering [at, end) of a cell that starts at `first`, then `empty` tiles of no point
  void add_cell(int64_t first, int64_t at, int64_t end, unsigned k, int64_t live, int64_t empty, int tile) {
    for (int64_t t = 0; t < live; ++t, at += tile) push((int)at, (int)std::min<int64_t>(tile, end - at), k);
    for (int64_t t = 0; t < empty; ++t) push((int)first, 0, k);
  }
  void pad_to(size_t mult) {  // empty tiles that repeat the preceding key
    while (!start.empty() && start.size() % mult) push(start.back(), 0, key.back());
  }
  void append(const TileList& o) {
    start.insert(start.end(), o.start.begin(), o.start.end());
    count.insert(count.end(), o.count.begin(), o.count.end());
    key.insert(key.end(), o.key.begin(), o.key.end());
  }

 private:
  void push(int s, int c, unsigned k) {
    start.push_back(s);
    count.push_back(c);
    key.push_back(k);
  }
};

// Tiles of <= `tile` points that never straddle a cell.
inline TileList cell_tiles(const unsigned* keys, int64_t n, int tile = CELL_TILE) {
  TileList l;
  l.reserve((size_t)n / 24 + 16);
  for_each_key_run(keys, n, [&](int64_t p, int64_t cnt, unsigned k) { l.add_cell(p, p, p + cnt, k, (cnt + tile - 1) / tile, 0, tile); });
  return l;
}

// Target tiles of the float32 cell kernels, in TWO lists.  A wavefront owns TT tiles of ONE cell, so a cell of `tiles`
// tiles used to be padded to a multiple of TT with empty tiles -- at the headline shape (cells of 1000 +- 32 points: 32
// tiles, or 33-34 for a fifth of them) 5.6 % of all tile pairs were such padding, and the kernel is bound by the matrix
// pipe.  Now a cell's tiles are split: whole groups of TT go to the MAIN list; a remainder of at most TT/2 tiles goes to
// the REST list in groups of two (a larger remainder is still padded to a whole group: workgroups with two tiles
// per wavefront are ~1.6x less efficient per tile).
struct CellTiles {
  int64_t main_live, main_empty, rest_live, rest_empty;
};
inline CellTiles split_cell_tiles(int64_t tiles, int TT) {
  const int64_t rem = tiles % TT;
  if (TT > CELL_REST_TT && rem > 0 && rem <= TT / 2) return {tiles - rem, 0, rem, round_up(rem, CELL_REST_TT) - rem};
  return {tiles, round_up(tiles, TT) - tiles, 0, 0};
}

// Tiles of the two lists for groups of TT, before the padding to whole workgroups
inline void cell_split_count(const unsigned* keys, int64_t n, int TT, int64_t* n_main, int64_t* n_rest) {
  *n_main = *n_rest = 0;
  for_each_key_run(keys, n, [&](int64_t, int64_t cnt, unsigned) {
    const CellTiles s = split_cell_tiles((cnt + CELL_TILE - 1) / CELL_TILE, TT);
    *n_main += s.main_live + s.main_empty;
    *n_rest += s.rest_live + s.rest_empty;
  });
}

// Both lists, each padded to whole workgroups (4 wavefronts) with empty tiles, in one list: n_main tiles, then n_rest.
inline TileList cell_tiles_split(const unsigned* keys, int64_t n, int TT, int64_t* n_main, int64_t* n_rest) {
  TileList main, rest;
  main.reserve((size_t)n / 24 + 64);
  for_each_key_run(keys, n, [&](int64_t p, int64_t cnt, unsigned k) {
    const CellTiles s = split_cell_tiles((cnt + CELL_TILE - 1) / CELL_TILE, TT);
    main.add_cell(p, p, p + cnt, k, s.main_live, s.main_empty, CELL_TILE);
    rest.add_cell(p, p + s.main_live * CELL_TILE, p + cnt, k, s.rest_live, s.rest_empty, CELL_TILE);
  });
  main.pad_to((size_t)TT * WAVES_PER_BLOCK);
  rest.pad_to((size_t)CELL_REST_TT * WAVES_PER_BLOCK);
  *n_main = (int64_t)main.size();
  *n_rest = (int64_t)rest.size();
  main.append(rest);
  return main;
}

// The two grids of the float32 cell kernels over the lists of cell_tiles_split(): r = 0 the MAIN list (groups of tt
// tiles per wavefront), r = 1 the REST list (the cells' leftover tiles, two per wavefront -- few workgroups, latency-bound
// each, so its own, finer split of the sources).  Each grid has its own segments and its own region
// [segment][cols][slots] of the partial sums.  cell_kernel and cellmm_kernel run them as two launches, one after the
// other; cellmm16_kernel as ONE launch, the REST grid behind the MAIN grid (fused_cell_grid below).
//
// A third list, r = 2 the TAIL, is empty unless cell_tail_split() (below) cuts it off the MAIN list: the MAIN list's last
// workgroups of target tiles, in more and shorter segments.  In the tile list and in the sums the lists stand MAIN, TAIL,
// REST (CELL_LIST_ORDER): the TAIL's tiles are the MAIN tiles they were, in place.
constexpr int CELL_LISTS = 3;
constexpr int CELL_LIST_ORDER[CELL_LISTS] = {0, 2, 1};  // the lists in the order of their tiles, slots and regions
struct CellSplit {
  int64_t m_stages, n_slots;  // source stages; target slots of all lists
  int64_t blocks[CELL_LISTS], slots[CELL_LISTS], seg_stages[CELL_LISTS];
  int segments[CELL_LISTS];
  int64_t grid(int r) const { return blocks[r] * segments[r]; }
  // first slot of list r among the n_slots (its first tile is slot_base / CELL_TILE)
  int64_t slot_base(int r) const {
    int64_t at = 0;
    for (int o = 0; o < CELL_LISTS && CELL_LIST_ORDER[o] != r; ++o) at += slots[CELL_LIST_ORDER[o]];
    return at;
  }
  size_t region_offset(int cols, int r) const {  // in doubles
    size_t at = 0;
    for (int o = 0; o < CELL_LISTS && CELL_LIST_ORDER[o] != r; ++o) at += (size_t)segments[CELL_LIST_ORDER[o]] * cols * slots[CELL_LIST_ORDER[o]];
    return at;
  }
  size_t part_doubles(int cols) const {
    size_t n = 0;
    for (int r = 0; r < CELL_LISTS; ++r) n += (size_t)segments[r] * slots[r] * cols;
    return n;
  }
};

// N targets in n_main / n_rest tiles; m_tiles source tiles in stages of stage_tiles; `main`: the rule of the main launch
// (single stages for few targets, as plan_stages)
inline CellSplit cell_split(int64_t N, int64_t m_tiles, int64_t n_main, int64_t n_rest, int tt, int opt_segments,
                            int stage_tiles, SegmentRule main) {
  CellSplit s;
  main.small = small_problem(N);
  if (main.small) main.min_seg = 1;
  s.m_stages = (m_tiles + stage_tiles - 1) / stage_tiles;
  s.n_slots = (n_main + n_rest) * CELL_TILE;
  s.blocks[0] = n_main / (tt * WAVES_PER_BLOCK);
  s.blocks[1] = n_rest / (CELL_REST_TT * WAVES_PER_BLOCK);
  s.slots[0] = n_main * CELL_TILE;
  s.slots[1] = n_rest * CELL_TILE;
  s.segments[0] = stage_segments(opt_segments, std::max<int64_t>(1, s.blocks[0]), s.m_stages, s.n_slots, main);
  s.seg_stages[0] = (s.m_stages + s.segments[0] - 1) / s.segments[0];
  s.segments[1] = 0;
  s.seg_stages[1] = 1;
  if (s.blocks[1] > 0) {
    SegmentRule rest = main;  // single stages allowed, ~1536 workgroups
    rest.min_seg = 1;
    rest.target_blocks = 1536;
    const int seg = choose_segments(opt_segments, s.blocks[1], s.m_stages, s.n_slots, rest);
    s.seg_stages[1] = (s.m_stages + seg - 1) / seg;
    s.segments[1] = (int)((s.m_stages + s.seg_stages[1] - 1) / s.seg_stages[1]);
  }
  s.blocks[2] = s.slots[2] = 0;  // no TAIL list (cell_tail_split)
  s.segments[2] = 0;
  s.seg_stages[2] = 1;
  return s;
}

// ---- both lists in one launch (cellmm16_kernel) ------------------------------------------------------------------------

// A second launch for the REST list starts only when the MAIN list's last round of workgroups has drained, and the chip
// stands partly idle through that tail (headline shape: 8000 workgroups in rounds of 512, the last one 320; then 1664 short
// workgroups, 0.65 ms for 1.3 % of the work).  In one grid the REST list's workgroups come LAST in index order and so are
// dispatched into the slots the last MAIN round leaves empty.  Nothing else changes: every workgroup does what it did in
// its own launch, on the same list, segments and region of the partial sums, so the sums are the same bit for bit.
//
// workgroup `bid` of the fused grid -> list (0 MAIN, 1 REST) and the workgroup's index in that list's own grid.  With
// main_grid a multiple of 8 (it is whenever the MAIN list has a multiple of 8 segments), (bid - main_grid) & 7 == bid & 7:
// the REST workgroups that share an XCD in the fused grid are those that shared one in their own launch, and the XCD
// affinity of block_to_work() holds for them.
// (constexpr: the kernel calls the very function the host tests hold to its properties)
//
// With a TAIL list (cell_tail_split below) the order is MAIN, TAIL, REST: list 2 stands between the two, tail_grid
// workgroups of it.  main_grid and tail_grid are both multiples of 8 then, so the same holds for TAIL and REST alike.
struct FusedCellWork {
  int list;
  int64_t local;
};
constexpr FusedCellWork fused_cell_work(int64_t bid, int64_t main_grid, int64_t tail_grid = 0) {
  return bid < main_grid               ? FusedCellWork{0, bid}
         : bid < main_grid + tail_grid ? FusedCellWork{2, bid - main_grid}
                                       : FusedCellWork{1, bid - main_grid - tail_grid};
}

// The fused grid of a split `s` with tt tiles per wavefront in the MAIN list.  opt_fused: the "cell_fused" option, -1 =
// automatic and 1 = one launch where it applies, 0 = always two launches.  It applies when there is a REST list (which
// needs tt > CELL_REST_TT: split_cell_tiles) and the two grids together are a grid a launch takes; a MAIN list that is
// empty while the REST list is not is a fused grid with main_grid = 0.  fused == false: the two grids are two launches.
struct FusedCellGrid {
  bool fused;
  int64_t main_grid, rest_grid, total, tail_grid;
};
inline FusedCellGrid fused_cell_grid(const CellSplit& s, int tt, int opt_fused) {
  FusedCellGrid g;
  g.main_grid = s.grid(0);
  g.rest_grid = s.grid(1);
  g.tail_grid = s.grid(2);
  g.total = g.main_grid + g.tail_grid + g.rest_grid;
  g.fused = opt_fused != 0 && tt > CELL_REST_TT && s.blocks[1] > 0 && g.total <= MAX_GRID;
  return g;
}

// ---- the last round of the fused grid in short segments (the TAIL list) -------------------------------------------------

// The MAIN list's workgroups are equally long and come in rounds of R resident workgroups (two per CU at eight tiles per
// wavefront).  B target blocks x S segments are seldom whole rounds: at the headline shape 978 x 8 = 7824 workgroups are
// 15 rounds of 512 and 144 more, which run their full length with 368 of 512 slots idle.  So the blocks of the whole
// rounds stay as they are, and the blocks left over are cut into k times as many segments, k times shorter, as many as
// fit the chip at once together with the REST list behind them:
//  * b_full, the largest count of blocks with b_full S a multiple of R (and of 8), keeps S segments;
//  * the last b_tail = B - b_full blocks take `segments` = S k segments of whole stages, k the largest integer with
//    b_tail S k + rest_grid <= R; capped at CELL_TAIL_MAX_SEGMENTS and at m_stages / min_seg (no segment shorter than the
//    rule's minimum), then settled (settle_segments) -- a k whose settled count is no multiple of 8 or no longer fits
//    gives way to k - 1;
//  * no TAIL (b_tail == 0) without whole rounds (b_full == 0), without blocks left over, or when k < 2.
// rest_grid: the slots of a round kept for the REST list -- cell_tail_split() passes its weight, not its number of
// workgroups (cell_rest_weight).
// The fused grid is MAIN (b_full S), TAIL (b_tail S k), REST: each part starts at a multiple of 8, so that a workgroup's
// index in its own list and its index in the grid agree modulo 8 and block_to_work()'s XCD affinity holds for every list.
// Every (target block, stage) pair is still taken exactly once; the TAIL blocks' sums see other segment cuts (more folds,
// another order of the fp64 partial sums), all other rows are bit for bit what they were.  Order decides speed alone.
constexpr int CELL_TAIL_MAX_SEGMENTS = 64;
struct CellTail {
  int64_t b_full, b_tail, seg_stages;
  int segments;
};
inline CellTail cell_tail_plan(int64_t B, int S, int64_t R, int64_t m_stages, int64_t rest_grid, int64_t min_seg) {
  const CellTail none = {B, 0, 1, 0};
  if (B <= 0 || S <= 0 || R <= 0) return none;
  int64_t gcd = R, t = S;
  while (t) {
    const int64_t u = gcd % t;
    gcd = t;
    t = u;
  }
  const int64_t q = R / gcd;  // blocks per smallest number of whole rounds
  const int64_t b_full = B / q * q, b_tail = B - b_full;
  if (b_full == 0 || b_tail == 0 || (b_full * S) % 8 != 0 || rest_grid >= R) return none;
  const int64_t cap = std::min<int64_t>(CELL_TAIL_MAX_SEGMENTS, m_stages / std::max<int64_t>(min_seg, 1));
  for (int64_t k = (R - rest_grid) / (b_tail * S); k >= 2; --k) {
    const int64_t want = std::min<int64_t>(S * k, cap);
    if (want <= S) break;
    const int64_t seg = settle_segments(m_stages, (int)want);
    if (seg % 8 == 0 && seg > S && seg <= cap && b_tail * seg + rest_grid <= R)
      return {b_full, b_tail, (m_stages + seg - 1) / seg, (int)seg};
  }
  return none;
}

// Is the TAIL list taken?  opt: the "cell_tail" option, -1 = automatic, 0 = never, 1 = wherever it applies: a fused launch
// (fused_cell_grid) with more than CELL_REST_TT tiles per wavefront.  Automatic: at eight tiles per wavefront, from the sizes
// from which cellmm16_kernel is taken by itself (as cell_balance_taken: below them no result changes unless asked for).
// KMVP_CELL_TAIL_AUTO=0 builds a library whose automatic is off (the arm it was measured against).
#ifndef KMVP_CELL_TAIL_AUTO
#define KMVP_CELL_TAIL_AUTO 1
#endif
constexpr bool CELL_TAIL_AUTO = KMVP_CELL_TAIL_AUTO != 0;
constexpr int CELL_TAIL_AUTO_TT = 8;
constexpr int64_t CELL_TAIL_AUTO_N = 500000, CELL_TAIL_AUTO_M = 100000;  // CELLMM16_AUTO_N, CELLMM16_AUTO_M (below)
constexpr bool cell_tail_taken(int opt, int tt, bool fused, int64_t N, int64_t M) {
  return fused && tt > CELL_REST_TT &&
         (opt > 0 || (opt < 0 && CELL_TAIL_AUTO && tt == CELL_TAIL_AUTO_TT && N >= CELL_TAIL_AUTO_N && M >= CELL_TAIL_AUTO_M));
}

// The REST list beside the TAIL, in workgroups of the MAIN list's length.  Its own workgroups are many and short (headline
// shape: 17 blocks x 94 segments = 1598 workgroups of 28 stages x 2 tiles per wavefront, against 327 stages x 8 tiles): by
// their number they would never fit a round, by their work they are 35 of its 512 slots.
inline int64_t cell_rest_weight(const CellSplit& s, int tt) {
  const int64_t main_work = std::max<int64_t>(1, s.seg_stages[0] * tt);
  return (s.grid(1) * s.seg_stages[1] * CELL_REST_TT + main_work - 1) / main_work;
}

// Cuts the TAIL list off the MAIN list of a split `s` (tt tiles per wavefront in both); `resident`: R.  Returns whether
// there is one.  The TAIL's tiles, slots and region of the partial sums follow the MAIN list's (CELL_LIST_ORDER).
inline bool cell_tail_split(CellSplit& s, int tt, int64_t resident, int64_t min_seg) {
  const CellTail t = cell_tail_plan(s.blocks[0], s.segments[0], resident, s.m_stages, cell_rest_weight(s, tt), min_seg);
  if (t.b_tail == 0) return false;
  const int64_t block_slots = (int64_t)tt * WAVES_PER_BLOCK * CELL_TILE;
  s.blocks[0] = t.b_full;
  s.slots[0] = t.b_full * block_slots;
  s.blocks[2] = t.b_tail;
  s.slots[2] = t.b_tail * block_slots;
  s.segments[2] = t.segments;
  s.seg_stages[2] = t.seg_stages;
  return true;
}

// ---- one-cell workgroups (cellmm16_kernel's shared operand build) -------------------------------------------------------

constexpr int CELL_SHARED_TT = 8;  // tiles per wavefront from which cellmm16_kernel holds the shared-build body

// Does a MAIN launch with tt tiles per wavefront ask its one-cell workgroups for the shared build?  opt: the
// "cell_shared_build" option, -1 = automatic and 1 = wherever the kernel holds that body, 0 = never.  At four tiles per
// wavefront the second body would cost the kernel its fourth wavefront per SIMD (118 -> 142 registers) for every workgroup,
// shared or not, so it is not instantiated there.
constexpr bool cell_shared_build(int tt, int opt) { return opt != 0 && tt >= CELL_SHARED_TT; }

// One-cell workgroups of a MAIN list: a workgroup is WAVES_PER_BLOCK wavefronts of tt tiles each, and one-cell when the
// first tiles of its wavefronts carry the same cell key (a wavefront's tiles are of one cell by construction).  The kernel
// compares the tiles' stored centres instead (cellmm16_one_cell); on one grid a key and a centre name the same cell.
// `keys`: the keys of the list's n_main tiles (a multiple of tt * WAVES_PER_BLOCK).  Returns the number of one-cell
// workgroups; the others are n_main / (tt * WAVES_PER_BLOCK) minus that.
inline int64_t count_one_cell_blocks(const unsigned* keys, int64_t n_main, int tt) {
  const int64_t per_block = (int64_t)tt * WAVES_PER_BLOCK;
  int64_t one = 0;
  for (int64_t t = 0; t + per_block <= n_main; t += per_block) {
    bool same = true;
    for (int w = 1; w < WAVES_PER_BLOCK; ++w) same = same && keys[t + (int64_t)w * tt] == keys[t];
    one += same ? 1 : 0;
  }
  return one;
}

// ---- count-cut cells (the "cell_balance" option) ------------------------------------------------------------------------

// A lattice cell holds whatever falls into it -- 1000 +- 32 points at the headline shape, never a multiple of a tile (32)
// or of a workgroup's targets (1024) -- so the last source tile of every cell is half empty and every cell's target tiles
// are padded or spill into the REST list: 5.4 % of the MFMAs multiply padding.  The kernels do not care how a cell is
// defined: they see a centre and a key per tile and offsets from that centre; only |2 d.e| <= CELL_T_MAX and the f16 operand
// range tie a cell to a size.  So the lattice is kept in x and y, and each (x, y) column is cut along z BY POINT COUNT.
//
// A fine key is (column << CELL_ZQ_BITS) | zq: `column` the 20 bits of the lattice's x and y cell indices, zq the point's z
// in CELL_ZQ equal buckets of the grid's z-extent.  Walking a column of the sorted fine keys, a cell takes points until it
// holds `full` points (32 TT WAVES_PER_BLOCK targets: one whole workgroup) or until its bucket range [zlo, zhi] would be
// wider than `cap` buckets.  A cell the cap stopped with at least `quantum` points (32 TT: a wavefront's tiles; 32 for a
// cloud that is only a source) is cut back to a multiple of `quantum`, so that it ends on a full tile or tile group; the
// points cut off start the next cell.  A cell is shorter only there and at the column's end.  Points of one bucket come in
// arbitrary order, and a cell boundary may fall inside a bucket: both neighbours' ranges then include that bucket, and
// a bucket of more than `full` points gives several cells of one range and one centre (harmless: a centre is only a point of
// expansion, and each cell has its own id).  A cell's id is its index, < 2^30: bit 30 and -1 keep their meanings in tile
// keys.  Deterministic: a function of the sorted keys alone.
constexpr int CELL_ZQ_BITS = 12;
constexpr int CELL_ZQ = 1 << CELL_ZQ_BITS;
constexpr int CELL_BALANCE_MIN_CAP = 16;  // buckets the z-cap must span for the cut to be fine enough (<= ~256 lattice cells along z)

struct CountCell {
  int64_t first, count;  // points [first, first + count) of the sorted order
  int zlo, zhi;          // bucket range, both ends included: zhi - zlo + 1 <= cap
  unsigned column;       // the lattice's x and y cell indices (x | y << 10)
};

inline std::vector<CountCell> count_cut_cells(const unsigned* fine, int64_t n, int cap, int64_t quantum, int64_t full) {
  std::vector<CountCell> cells;
  cells.reserve((size_t)(n / std::max<int64_t>(full, 1)) + 16);
  const unsigned zmask = (unsigned)CELL_ZQ - 1u;
  for (int64_t p = 0; p < n;) {
    const unsigned column = fine[p] >> CELL_ZQ_BITS;
    const int zlo = (int)(fine[p] & zmask);
    int64_t e = p + 1;
    while (e < n && e - p < full && (fine[e] >> CELL_ZQ_BITS) == column && (int)(fine[e] & zmask) - zlo < cap) ++e;
    const bool by_cap = e < n && e - p < full && (fine[e] >> CELL_ZQ_BITS) == column;
    int64_t count = e - p;
    if (by_cap && count >= quantum) count = count / quantum * quantum;
    cells.push_back({p, count, zlo, (int)(fine[p + count - 1] & zmask), column});
    p += count;
  }
  return cells;
}

// z-centre of a bucket range: the midpoint of [zlo, zhi + 1) buckets of width bw above lo, rounded once to the float32 the
// device stores (buckets are cut in double precision, so a point is within half the range's width of it to half an ulp)
inline float count_cell_zcentre(double lo, double bw, int zlo, int zhi) { return (float)(lo + 0.5 * (double)(zlo + zhi + 1) * bw); }

// Source tiles of count-cut cells: as cell_tiles(), in cell order, the cell's id as the key
inline TileList count_cell_source_tiles(const std::vector<CountCell>& cells, int tile = CELL_TILE) {
  TileList l;
  l.reserve(cells.size() * 33 + 16);
  for (size_t i = 0; i < cells.size(); ++i) {
    const CountCell& c = cells[i];
    l.add_cell(c.first, c.first, c.first + c.count, (unsigned)i, (c.count + tile - 1) / tile, 0, tile);
  }
  return l;
}

// Target tiles of count-cut cells: split_cell_tiles() per cell, both lists padded to whole workgroups, n_main tiles then
// n_rest (as cell_tiles_split).  The MAIN list is cut into workgroups of TT WAVES_PER_BLOCK tiles in list order, and a short
// cell (the last of a column, or one the cap stopped) would shift every later cell off the workgroup boundary -- in cell
// order only a fifth of the headline shape's workgroups are one-cell and take the shared operand build.  So cells whose
// MAIN tiles fill whole workgroups come first, the others behind them, each class in cell order; slot_of maps the results
// back, whatever the order of the list.
inline TileList count_cell_target_tiles(const std::vector<CountCell>& cells, int TT, int64_t* n_main, int64_t* n_rest) {
  TileList main, rest;
  main.reserve(cells.size() * 33 + 64);
  const int64_t per_block = (int64_t)TT * WAVES_PER_BLOCK;
  for (int pass = 0; pass < 2; ++pass)
    for (size_t i = 0; i < cells.size(); ++i) {
      const CountCell& c = cells[i];
      const CellTiles s = split_cell_tiles((c.count + CELL_TILE - 1) / CELL_TILE, TT);
      const int64_t m = s.main_live + s.main_empty;
      if ((m > 0 && m % per_block == 0) != (pass == 0)) continue;
      main.add_cell(c.first, c.first, c.first + c.count, (unsigned)i, s.main_live, s.main_empty, CELL_TILE);
      rest.add_cell(c.first, c.first + s.main_live * CELL_TILE, c.first + c.count, (unsigned)i, s.rest_live, s.rest_empty, CELL_TILE);
    }
  main.pad_to((size_t)per_block);
  rest.pad_to((size_t)CELL_REST_TT * WAVES_PER_BLOCK);
  *n_main = (int64_t)main.size();
  *n_rest = (int64_t)rest.size();
  main.append(rest);
  return main;
}

// Does the count cut apply to a float32 cell list with tt tiles per wavefront, and is it taken?  opt: the "cell_balance"
// option, -1 = automatic, 0 = never, 1 = wherever it applies.  It applies in three dimensions, at eight tiles per
// wavefront (a cell is then one workgroup of the MAIN list), when the z-cap spans enough buckets.  Automatic also asks for
// the sizes from which the 16x16x32 kernel is taken by itself: below them no result changes unless asked for.
constexpr bool cell_balance_applies(int D, bool f32, int tt, int cap) {
  return D == 3 && f32 && tt == CELL_SHARED_TT && cap >= CELL_BALANCE_MIN_CAP;
}
constexpr int64_t CELLMM16_AUTO_N = 500000, CELLMM16_AUTO_M = 100000;  // from here cellmm16_kernel is taken by itself (at TT = 8)
static_assert(CELL_TAIL_AUTO_N == CELLMM16_AUTO_N && CELL_TAIL_AUTO_M == CELLMM16_AUTO_M, "one size rule");
constexpr bool cell_balance_taken(int opt, bool applies, int64_t N, int64_t M) {
  return opt != 0 && applies && (opt > 0 || (N >= CELLMM16_AUTO_N && M >= CELLMM16_AUTO_M));
}

}  // namespace kmvp
