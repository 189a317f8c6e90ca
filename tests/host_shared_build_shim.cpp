// C surface of the one-cell workgroup count of csrc/kmvp_plan.hpp for tests/test_host_shared_build.py (host compiler only,
// no HIP).
#include <cstring>

#include "kmvp_plan.hpp"

using namespace kmvp;

extern "C" {

// CELL_SHARED_TT, WAVES_PER_BLOCK, CELL_TILE, CELL_REST_TT
void hs_constants(int64_t* out) {
  const int64_t v[4] = {CELL_SHARED_TT, WAVES_PER_BLOCK, CELL_TILE, CELL_REST_TT};
  std::memcpy(out, v, sizeof(v));
}

// The two tile lists as cell_prepare() builds them from the sorted cell keys of n points (cell_tiles_split), and the MAIN
// list's workgroups.  out: n_main, n_rest (tiles), workgroups of the MAIN list, one-cell workgroups among them
void hs_one_cell_blocks(const unsigned* keys, int64_t n, int TT, int64_t* out) {
  int64_t n_main = 0, n_rest = 0;
  const TileList l = cell_tiles_split(keys, n, TT, &n_main, &n_rest);
  out[0] = n_main;
  out[1] = n_rest;
  out[2] = n_main / ((int64_t)TT * WAVES_PER_BLOCK);
  out[3] = count_one_cell_blocks(l.key.data(), n_main, TT);
}

// cell_shared_build(tt, opt)
int hs_shared_build(int tt, int opt) { return cell_shared_build(tt, opt) ? 1 : 0; }
}
