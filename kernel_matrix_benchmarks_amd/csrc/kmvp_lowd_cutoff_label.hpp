// DBSCAN's two pair loops on the cell list (include/kmvp.h kmvp_dbscan; driver: kmvp_dbscan.hip).
//
// lowd_cutoff_count_kernel's walk (kmvp_lowd_cutoff.hpp) with a label per lane in place of the counter: the tile of the
// wave, the outer loop over its runs, two SGPR batches of U = 4 records in ping-pong, one target per lane, no LDS, no
// barrier, no partial result.  Beside every batch of records the wave reads the U labels of those records from
// lab_rec[m_alloc], an int32 array in record order, at a wave-uniform address -- the way lowd_cutoff_knn_kernel reads
// smap32: one scalar load of four dwords per batch.  The record of a source that is no core point and a pad record both
// hold LABEL_NONE = INT32_MAX (N < 2^31 is a plan condition).
//
//   MODE = LABEL_SWEEP   mine = min(mine, s <= r2 ? lab_rec : LABEL_NONE): one select and one v_min_i32 on top of the
//                        count's pair.  A core lane writes nxt[i], i its caller's index, and raises the changed word (a
//                        vector atomic) where the value fell below its own label.  A core point's own pair has s = 0
//                        exactly, so nxt[i] <= lab[i].
//   MODE = LABEL_BORDER  s = (s <= r2 && lab_rec != LABEL_NONE) ? s : +inf, then rknn_insert1 on (s, smap32): the nearest
//                        inside core point under the order of kmvp_radius_knn_list.hpp, (s, caller's index).  A lane that
//                        is no core point writes the winning index to attach[i], or -1.
// The inside test is the count's: s = knn_sqdist in the working precision against r2 = (real)(R R); a NaN s is outside.
//
// lab_rec (and lab, which a lane reads once for its own point) is written by other launches only, never by the launch
// that reads it: the scalar data cache sees no line change under it, and a sweep is a Jacobi step -- nxt depends on the
// labels before the launch alone, whatever the order the waves run in.
//
// Reads past a run are the count kernel's: U records, U labels and (BORDER) U indices behind the run; the plan keeps
// rec0 + len + U <= m_alloc for every run and both int32 arrays hold m_alloc entries.  A tile without runs reads neither.
#pragma once
#include "kmvp_lowd_cutoff.hpp"
#include "kmvp_radius_knn_list.hpp"

namespace kmvp {

enum : int { LABEL_SWEEP = 0, LABEL_BORDER = 1 };
constexpr int32_t LABEL_NONE = INT32_MAX;

template <typename real>
struct LowdCutoffLabelArgs {
  const real* xs;           // targets, SoA over the padded slots: xs[d * n_pad + slot]
  const real* rec;          // source records [m_alloc][R], the density layout
  const CutoffTile* tiles;  // [n_pad / 64]
  const CutoffRun* runs;
  const int64_t* tmap;      // [n_pad] slot -> caller's index, -1 for a pad
  int64_t n_pad;
  real r2;                  // (real)(R R)
  const int32_t* lab_rec;   // [m_alloc] the label of every record's source; LABEL_NONE: no core point, or a pad
  const int32_t* smap32;    // [m_alloc] record -> caller's index, -1 for a pad (BORDER)
  const int32_t* lab;       // [N] the label of every point; LABEL_NONE: no core point
  int32_t* nxt;             // [N] SWEEP: the smallest label among the inside core points, core points only
  int32_t* changed;         // SWEEP: one word, raised where a label fell
  int32_t* attach;          // [N] BORDER: the nearest inside core point or -1, points that are no core points only
};

template <int D, int MODE, typename real>
__global__ void __launch_bounds__(BLOCK_THREADS) lowd_cutoff_label_kernel(const LowdCutoffLabelArgs<real> a) {
  constexpr int R = RecLayout<D, 1, SIG_DENSITY>::R;
  constexpr int U = 4;
  constexpr bool BORDER = MODE == LABEL_BORDER;
  static_assert(2 * U == CUTOFF_RECORDS, "two ping-pong batches per round");

  const int lane = threadIdx.x & 63;
  int64_t slot0;
  const CutoffTile t = cutoff_tile_of_wave(a.tiles, slot0);

  real x[D];
#pragma unroll
  for (int d = 0; d < D; ++d) x[d] = a.xs[(int64_t)d * a.n_pad + slot0 + lane];  // < n_pad by construction; pads are 0
  const real r2 = a.r2;
  const real inf = (real)INFINITY;

  int32_t mine = LABEL_NONE;  // SWEEP
  real s0 = inf;              // BORDER
  int32_t j0 = -1;

  auto run_batch = [&](const real (&rb)[U * R], const int32_t (&lb)[U], const int32_t (&jb)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      real s = knn_sqdist<D, real>(x, rb + u * R);
      if constexpr (BORDER) {
        s = (s <= r2 && lb[u] != LABEL_NONE) ? s : inf;
        rknn_insert1<real>(s0, j0, s, jb[u]);
      } else {
        mine = min(mine, s <= r2 ? lb[u] : LABEL_NONE);
      }
    }
  };

  for (int q = 0; q < t.nruns; ++q) {
    const CutoffRun run = a.runs[t.run0 + q];
    const real* __restrict__ segp = a.rec + run.rec0 * R;
    const int32_t* __restrict__ segl = a.lab_rec + run.rec0;
    const int32_t* __restrict__ segj = a.smap32 + run.rec0;
    const int seg_n = run.len;
    real ra[U * R], rb[U * R];
    int32_t la[U], lb[U], ja[U], jb[U];
#pragma unroll
    for (int i = 0; i < U * R; ++i) ra[i] = segp[i];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      la[i] = segl[i];
      ja[i] = BORDER ? segj[i] : 0;
    }
    for (int j = 0; j < seg_n; j += 2 * U) {
      const real* __restrict__ pb = segp + (int64_t)(j + U) * R;
#pragma unroll
      for (int i = 0; i < U * R; ++i) rb[i] = pb[i];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        lb[i] = segl[j + U + i];
        jb[i] = BORDER ? segj[j + U + i] : 0;
      }
      run_batch(ra, la, ja);
      const real* __restrict__ pa = segp + (int64_t)(j + 2 * U) * R;
#pragma unroll
      for (int i = 0; i < U * R; ++i) ra[i] = pa[i];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        la[i] = segl[j + 2 * U + i];
        ja[i] = BORDER ? segj[j + 2 * U + i] : 0;
      }
      run_batch(rb, lb, jb);
    }
  }

  if (lane < t.live) {
    const int64_t i = a.tmap[slot0 + lane];
    const int32_t own = a.lab[i];
    if constexpr (BORDER) {
      if (own == LABEL_NONE) a.attach[i] = j0;
    } else {
      if (own != LABEL_NONE) {
        a.nxt[i] = mine;
        if (mine < own) atomicOr(a.changed, 1);
      }
    }
  }
}

// kmvp_lowd_cutoff_label_inst.hip, one unit per precision: D = 1 .. CUTOFF_MAX_D in both modes.  hipErrorInvalidValue
// where nothing is instantiated.
hipError_t launch_lowd_cutoff_label_f32(int D, int mode, const LowdCutoffLabelArgs<float>& args, dim3 grid, hipStream_t stream,
                                        const char** kernel_name);
hipError_t launch_lowd_cutoff_label_f64(int D, int mode, const LowdCutoffLabelArgs<double>& args, dim3 grid, hipStream_t stream,
                                        const char** kernel_name);

}  // namespace kmvp
