// K nearest sources within a radius on the cell list (include/kmvp.h kmvp_radius_nearest): for every target the K smallest
// (s_ij, j) among the sources with s_ij <= r2, j the caller's source index.
//
// lowd_cutoff_count_kernel's walk (kmvp_lowd_cutoff.hpp) with a sorted list per lane in place of the counter: the tile of
// the wave, the outer loop over its runs, two SGPR batches of U = 4 records in ping-pong, one target per lane, no LDS, no
// barrier, no partial result, no atomic.  Beside every batch of records the wave reads the U caller's indices of those
// records from an int32 copy of the plan's smap (M < 2^31 is a plan condition; -1: a pad) at a wave-uniform address: one
// scalar load of four dwords per batch.
//
// Per pair: s = knn_sqdist (the value kmvp_nearest and kmvp_radius_count compare), s = s <= r2 ? s : +inf -- the select
// removes the pairs outside, a NaN s (a NaN target) and the pad records (s = +inf) -- and then the insertion of (s, j) into
// the list of kmvp_radius_knn_list.hpp, ordered by the pair: the walk does not meet the sources in ascending index.
// The insertion runs under a wave-uniform gate PER RECORD, __any(s <= r2 && !(bound < s)): `<=` in both places, since a
// tie in s may still enter on its index.  bound is the lane's K-th [+ 1] smallest so far: the list keeps the entries the
// row needs at the END of its KT positions (rknn_init), so the bound is its last entry whatever K is.  Per batch the gate
// would be open whenever one of 256 (lane, record) pairs passes, per record one of 64; it costs one scalar and-ing of the
// two compares and one scalar branch per record.  KT = 1 keeps no list and no gate.
//
// Issue slots per walked record, float32, D = 3, from the disassembly (the count: 6 for the distance, v_cmp, v_addc = 8):
//   KT = 1: 14 VALU (distance 6, 4 v_cmp, 3 v_cndmask, 1 v_mov) and 5 scalar, no branch;
//   KT = 4, 16, gate closed: 8 VALU (distance 6, v_cmp against r2, v_cmp against the bound), s_and, the branch -- the
//   mask select is sunk into the insertion;
//   an open gate adds 37 VALU + 23 scalar at KT = 4 and 129 VALU + 84 scalar at KT = 16.
// Measured ratios to the count and what they say about the gate: LAB_NOTES.md section 36.
//
// A lane finishes its own row at tmap[slot]: rknn_finish writes K (index, squared distance) pairs, the distance widened to
// float64.  A NaN target coordinate gives (-1, NaN) in all K entries where there is a source at all (nan_rows; kmvp_nearest's
// M = 0 answer is the empty list also for such a row).
//
// Reads past a run are the count kernel's: U records, and here U indices, behind the run; the plan keeps
// rec0 + len + U <= m_alloc for every run and the index copy holds m_alloc entries.  A tile without runs reads neither.
#pragma once
#include "kmvp_lowd_cutoff.hpp"
#include "kmvp_radius_knn_list.hpp"

namespace kmvp {

template <int D, int KT, typename real>
__global__ void __launch_bounds__(BLOCK_THREADS) lowd_cutoff_knn_kernel(const LowdCutoffArgs<real> a) {
  constexpr int R = RecLayout<D, 1, SIG_DENSITY>::R;
  constexpr int U = 4;
  static_assert(2 * U == CUTOFF_RECORDS, "two ping-pong batches per round");

  const int lane = threadIdx.x & 63;
  int64_t slot0;
  const CutoffTile t = cutoff_tile_of_wave(a.tiles, slot0);

  real x[D];
  bool x_nan = false;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    x[d] = a.xs[(int64_t)d * a.n_pad + slot0 + lane];  // < n_pad by construction; pads are 0
    x_nan = x_nan || (x[d] != x[d]);
  }
  const real r2 = a.r2;
  const real inf = (real)INFINITY;

  real sl[KT];
  int32_t jl[KT];
  // the list keeps kc = K (+ 1 with exclude_self) <= KT entries at its end: its last entry is the lane's bound whatever K
  // is, so K = 5 in a list of 16 gates on its 5th smallest, not on its 16th
  rknn_init<KT, real>(sl, jl, a.knn_k + (a.exclude_self != 0 ? 1 : 0));

  auto run_batch = [&](const real (&rb)[U * R], const int32_t (&jb)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      real s = knn_sqdist<D, real>(x, rb + u * R);
      const bool inside = s <= r2;
      s = inside ? s : inf;
      if constexpr (KT == 1) {
        rknn_insert1<real>(sl[0], jl[0], s, jb[u]);
      } else {
        if (__any(inside && !(sl[KT - 1] < s))) rknn_insert<KT, real>(sl, jl, s, jb[u]);  // wave-uniform
      }
    }
  };

  for (int q = 0; q < t.nruns; ++q) {
    const CutoffRun run = a.runs[t.run0 + q];
    const real* __restrict__ segp = a.rec + run.rec0 * R;
    const int32_t* __restrict__ segj = a.smap32 + run.rec0;
    const int seg_n = run.len;
    real ra[U * R], rb[U * R];
    int32_t ja[U], jb[U];
#pragma unroll
    for (int i = 0; i < U * R; ++i) ra[i] = segp[i];
#pragma unroll
    for (int i = 0; i < U; ++i) ja[i] = segj[i];
    for (int j = 0; j < seg_n; j += 2 * U) {
      const real* __restrict__ pb = segp + (int64_t)(j + U) * R;
#pragma unroll
      for (int i = 0; i < U * R; ++i) rb[i] = pb[i];
#pragma unroll
      for (int i = 0; i < U; ++i) jb[i] = segj[j + U + i];
      run_batch(ra, ja);
      const real* __restrict__ pa = segp + (int64_t)(j + 2 * U) * R;
#pragma unroll
      for (int i = 0; i < U * R; ++i) ra[i] = pa[i];
#pragma unroll
      for (int i = 0; i < U; ++i) ja[i] = segj[j + 2 * U + i];
      run_batch(rb, jb);
    }
  }

  if (lane < t.live) {
    const int64_t i = a.tmap[slot0 + lane];
    rknn_finish<KT, real>(sl, jl, a.knn_k, a.exclude_self != 0, i, x_nan && a.knn_nan_rows != 0, a.knn_idx + i * a.knn_k,
                          a.knn_sqdist + i * a.knn_k);
  }
}

// kmvp_lowd_cutoff_knn_inst.hip, one unit per precision: D = 1 .. CUTOFF_MAX_D, list capacities KT = 1, 4, 16.
// hipErrorInvalidValue where nothing is instantiated.
hipError_t launch_lowd_cutoff_knn_f32(int D, int KT, const LowdCutoffArgs<float>& args, dim3 grid, hipStream_t stream,
                                      const char** kernel_name);
hipError_t launch_lowd_cutoff_knn_f64(int D, int KT, const LowdCutoffArgs<double>& args, dim3 grid, hipStream_t stream,
                                      const char** kernel_name);

}  // namespace kmvp
