// C surface of the count-cut cells of csrc/kmvp_plan.hpp for tests/test_host_cell_balance.py (host compiler only, no HIP).
#include <cstring>
#include <vector>

#include "kmvp_plan.hpp"

using namespace kmvp;

static std::vector<CountCell> g_cells;
static TileList g_sources, g_targets;

static void copy_list(const TileList& l, int* start, int* count, unsigned* key) {
  std::memcpy(start, l.start.data(), l.size() * sizeof(int));
  std::memcpy(count, l.count.data(), l.size() * sizeof(int));
  std::memcpy(key, l.key.data(), l.size() * sizeof(unsigned));
}

extern "C" {

// CELL_ZQ_BITS, CELL_ZQ, CELL_BALANCE_MIN_CAP, CELL_TILE, WAVES_PER_BLOCK, CELL_REST_TT, CELL_SHARED_TT
void hb_constants(int64_t* out) {
  const int64_t v[7] = {CELL_ZQ_BITS, CELL_ZQ, CELL_BALANCE_MIN_CAP, CELL_TILE, WAVES_PER_BLOCK, CELL_REST_TT, CELL_SHARED_TT};
  std::memcpy(out, v, sizeof(v));
}

// count_cut_cells() on sorted fine keys; the cells stay here for the calls below.  Returns their number.
int64_t hb_cut(const unsigned* fine, int64_t n, int cap, int64_t quantum, int64_t full) {
  g_cells = count_cut_cells(fine, n, cap, quantum, full);
  return (int64_t)g_cells.size();
}

// per cell: first, count, zlo, zhi, column
void hb_cells(int64_t* first, int64_t* count, int* zlo, int* zhi, unsigned* column) {
  for (size_t i = 0; i < g_cells.size(); ++i) {
    first[i] = g_cells[i].first;
    count[i] = g_cells[i].count;
    zlo[i] = g_cells[i].zlo;
    zhi[i] = g_cells[i].zhi;
    column[i] = g_cells[i].column;
  }
}

float hb_zcentre(double lo, double bucket, int zlo, int zhi) { return count_cell_zcentre(lo, bucket, zlo, zhi); }

// the source list and the target lists (n_main tiles, then n_rest) of the cells of the last hb_cut()
int64_t hb_source_tiles() {
  g_sources = count_cell_source_tiles(g_cells);
  return (int64_t)g_sources.size();
}
void hb_source_list(int* start, int* count, unsigned* key) { copy_list(g_sources, start, count, key); }
void hb_target_tiles(int TT, int64_t* n_main, int64_t* n_rest) { g_targets = count_cell_target_tiles(g_cells, TT, n_main, n_rest); }
void hb_target_list(int* start, int* count, unsigned* key) { copy_list(g_targets, start, count, key); }

int64_t hb_one_cell_blocks(const unsigned* keys, int64_t n_main, int tt) { return count_one_cell_blocks(keys, n_main, tt); }

int hb_applies(int D, int f32, int tt, int cap) { return cell_balance_applies(D, f32 != 0, tt, cap) ? 1 : 0; }
int hb_taken(int opt, int applies, int64_t N, int64_t M) { return cell_balance_taken(opt, applies != 0, N, M) ? 1 : 0; }
}
