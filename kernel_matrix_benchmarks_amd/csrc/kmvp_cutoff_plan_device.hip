// The cell-list plan of the cutoff-radius entries built on the device ("cutoff_plan" = 1; include/kmvp.h).  Every entry is
// formed by a rule of kmvp_cutoff_plan_device.hpp, one thread per entry; the kernels here are loops over those rules between
// hipcub's radix sort (stable: ties keep the caller's order, as the host's counting sort), exclusive scans and one integer
// sum.  No atomics, so the tables are the host build's entry for entry and the same from run to run.
//   extent       two stages: per-block partial extents of the finite points of both clouds, then one block
//                -> read back: 6 doubles and the "any finite point" flag; the host runs cutoff_grid
//   keys         one thread per point, then DeviceRadixSort::SortPairs of (key, caller index) per cloud (one cloud when
//                the targets are the sources)
//   first        one thread per cell: the first sorted position of the cell, by bisection of the sorted keys
//   rows         padded records and tiles per row, DeviceScan::ExclusiveSum of each
//   sources      smap filled with -1, then one thread per sorted source writes its record
//   tiles        one thread per tile counts its runs; ExclusiveSum gives run0; one thread per tile writes its runs and its
//                table entry; one thread per slot writes tmap; DeviceReduce::Sum adds up the walked records
//                -> read back: m_pad, tiles, runs, walked, live tiles
// The tables are sized before the build from bounds the host can state (cutoff_tiles_bound and its like) -- a grow-only
// ensure() of ct_tiles, ct_runs, ct_tmap and ct_smap -- and every index a kernel forms is held against those capacities.
#include <chrono>

#include <hipcub/hipcub.hpp>

#include "kmvp_ctx.hpp"
#include "kmvp_cutoff_plan_device.hpp"

namespace kmvp {
namespace {

constexpr int CTP_THREADS = 256;
constexpr int CTP_EXTENT_BLOCKS = 512;  // partial extents of stage one at most

// The block's extent in thread 0's e: a tree over LDS, the merge order fixed by the thread numbers.
__device__ void extent_block_reduce(CutoffExtent& e, int D) {
  __shared__ CutoffExtent sh[CTP_THREADS];
  sh[threadIdx.x] = e;
  __syncthreads();
  for (int step = CTP_THREADS / 2; step > 0; step >>= 1) {
    if ((int)threadIdx.x < step) cutoff_extent_merge(sh[threadIdx.x], sh[threadIdx.x + step], D);
    __syncthreads();
  }
  e = sh[0];
}

// Stage one: part[blockIdx.x] is the extent of the points this block strides over; point i < M is source i, the others
// are targets (N = 0 when the targets are the sources).
template <typename real>
__global__ void cutoff_extent_partial_kernel(const real* __restrict__ y, int64_t M, const real* __restrict__ x, int64_t N, int D,
                                             CutoffExtent* __restrict__ part) {
  CutoffExtent e;
  cutoff_extent_init(e);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M + N; i += (int64_t)gridDim.x * blockDim.x) {
    const real* q = i < M ? y + i * D : x + (i - M) * D;
    double p[3] = {0.0, 0.0, 0.0};
    for (int d = 0; d < D; ++d) p[d] = (double)q[d];
    cutoff_extent_point(e, p, D);
  }
  extent_block_reduce(e, D);
  if (threadIdx.x == 0) part[blockIdx.x] = e;
}

// Stage two, one block: out[0] is the extent of the nparts partial ones.
__global__ void cutoff_extent_final_kernel(const CutoffExtent* __restrict__ part, int nparts, int D, CutoffExtent* __restrict__ out) {
  CutoffExtent e;
  cutoff_extent_init(e);
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) cutoff_extent_merge(e, part[i], D);
  extent_block_reduce(e, D);
  if (threadIdx.x == 0) out[0] = e;
}

template <typename real>
__global__ void cutoff_keys_kernel(const real* __restrict__ pts, int64_t n, CutoffGridView gv, uint32_t* __restrict__ keys,
                                   int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double p[3] = {0.0, 0.0, 0.0};
  for (int d = 0; d < gv.D; ++d) p[d] = (double)pts[i * gv.D + d];
  keys[i] = cutoff_point_key(p, gv);
  idx[i] = (int32_t)i;
}

// first[c], c = 0 .. ncells
__global__ void cutoff_first_kernel(const uint32_t* __restrict__ keys, int64_t n, int64_t ncells, int32_t* __restrict__ first) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > ncells) return;
  first[c] = cutoff_lower_bound(keys, n, (uint32_t)c);
}

// rowlen[r], rowtiles[r], r = 0 .. nrows: a row's padded records and its tiles, 0 behind the last row
__global__ void cutoff_rows_kernel(const int32_t* __restrict__ sfirst, const int32_t* __restrict__ tfirst, int64_t g0, int64_t nrows,
                                   int64_t* __restrict__ rowlen, int64_t* __restrict__ rowtiles) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > nrows) return;
  rowlen[r] = r < nrows ? cutoff_row_padded(sfirst, g0, r) : 0;
  rowtiles[r] = r < nrows ? cutoff_row_tiles(tfirst, g0, r) : 0;
}

__global__ void cutoff_fill_kernel(int64_t* __restrict__ a, int64_t n, int64_t value) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = value;
}

// One thread per sorted source with finite coordinates: its record's entry of smap (cap entries).
__global__ void cutoff_smap_kernel(CutoffSorted s, const int64_t* __restrict__ rowbase, int64_t g0, int64_t ncells,
                                   int64_t* __restrict__ smap, int64_t cap) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)s.first[ncells] || p >= s.n) return;
  const int64_t rec = cutoff_source_record(s, rowbase, g0, p);
  if (rec >= 0 && rec < cap) smap[rec] = (int64_t)s.idx[p];
}

// One thread per tile of the table's capacity: nruns[t] and walk[t] = live x (records of its runs); nruns[cap] = 0 closes
// the scan, whose last entry is then the number of runs.
__global__ void cutoff_tile_count_kernel(CutoffSorted tg, const int64_t* __restrict__ tilebase, const int32_t* __restrict__ sfirst,
                                         const int64_t* __restrict__ rowbase, CutoffGridView gv, int64_t cap,
                                         int64_t* __restrict__ nruns, int64_t* __restrict__ walk) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t > cap) return;
  if (t == cap) {
    nruns[t] = 0;
    return;
  }
  const CutoffTileGeom q = cutoff_tile_geom(t, tg, tilebase, gv);
  int64_t len_sum;
  nruns[t] = cutoff_tile_runs(q, sfirst, rowbase, gv, nullptr, &len_sum);
  walk[t] = (int64_t)q.live * len_sum;
}

// One thread per tile: its runs from run0[t] on (run_cap entries in all), and its entry of the tile table.
__global__ void cutoff_tile_write_kernel(CutoffSorted tg, const int64_t* __restrict__ tilebase, const int32_t* __restrict__ sfirst,
                                         const int64_t* __restrict__ rowbase, CutoffGridView gv, int64_t cap,
                                         const int64_t* __restrict__ run0, int64_t run_cap, CutoffTile* __restrict__ tiles,
                                         CutoffRun* __restrict__ runs) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cap) return;
  const CutoffTileGeom q = cutoff_tile_geom(t, tg, tilebase, gv);
  if (q.kind == CUTOFF_TILE_NONE) return;
  CutoffRun mine[9];
  int64_t len_sum;
  const int32_t n = cutoff_tile_runs(q, sfirst, rowbase, gv, mine, &len_sum);
  const int64_t r0 = run0[t];
  for (int32_t k = 0; k < n; ++k)
    if (r0 + k >= 0 && r0 + k < run_cap) runs[r0 + k] = mine[k];
  CutoffTile e;
  e.run0 = r0;
  e.nruns = n;
  e.live = q.live;
  tiles[t] = e;
}

// One thread per target slot of the table's capacity.
__global__ void cutoff_tmap_kernel(CutoffSorted tg, const int64_t* __restrict__ tilebase, CutoffGridView gv, int64_t cap,
                                   int64_t* __restrict__ tmap) {
  const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= cap * CUTOFF_TILE) return;
  const CutoffTileGeom q = cutoff_tile_geom(slot / CUTOFF_TILE, tg, tilebase, gv);
  if (q.kind == CUTOFF_TILE_NONE) return;
  const int lane = (int)(slot % CUTOFF_TILE);
  int64_t v = -1;
  if (lane < q.live && q.s0 + lane < tg.n) v = cutoff_tmap_entry(q, tg, lane);
  tmap[slot] = v;
}

// sizes[0 .. 5): m_pad, tiles, runs, walked, live tiles
__global__ void cutoff_sizes_kernel(CutoffSorted tg, const int64_t* __restrict__ tilebase, const int64_t* __restrict__ rowbase,
                                    CutoffGridView gv, const int64_t* __restrict__ run0, int64_t cap, const int64_t* __restrict__ walked,
                                    int64_t* __restrict__ sizes) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  sizes[0] = rowbase[gv.nrows];
  sizes[1] = cutoff_all_tiles(tg, tilebase, gv);
  sizes[2] = run0[cap];
  sizes[3] = walked[0];
  sizes[4] = cutoff_live_tiles(tg, tilebase, gv);
}

// A region of the work buffer: `bytes` from the running offset, which moves on in steps of 256.
struct Carver {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) / 256 * 256;
    return at;
  }
};

template <typename real>
int cutoff_plan_device_t(kmvp_ctx* c, double radius, CutoffBuilt* out, bool* fits) {
  const int D = c->D;
  const int64_t M = c->M, N = c->N;
  const bool same = c->same_points;
  *fits = false;
  if (M > CUTOFF_MAX_SOURCES)
    return fail(c, KMVP_E_UNSUPPORTED, "cutoff radius: 2^31 sources or more (the pair loop counts positions within a run in 32 bits)");
  if (!cutoff_device_fits(N, M, 1)) return KMVP_OK;
  const real* y = (const real*)c->y_raw.p;
  const real* x = same ? y : (const real*)c->x_raw.p;
  hipStream_t st = c->stream;
  int rc;

  // ---- the extent, then the grid on the host
  const int64_t total = same ? M : M + N;
  const int nparts = (int)std::max<int64_t>(1, std::min<int64_t>(CTP_EXTENT_BLOCKS, (total + CTP_THREADS - 1) / CTP_THREADS));
  if ((rc = ensure(c, c->ct_work, (size_t)(nparts + 1) * sizeof(CutoffExtent)))) return rc;
  CutoffExtent* d_part = (CutoffExtent*)c->ct_work.p;
  hipLaunchKernelGGL((cutoff_extent_partial_kernel<real>), dim3(nparts), dim3(CTP_THREADS), 0, st, y, M, x, same ? (int64_t)0 : N, D, d_part);
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(cutoff_extent_final_kernel, dim3(1), dim3(CTP_THREADS), 0, st, (const CutoffExtent*)d_part, nparts, D, d_part + nparts);
  HIP_TRY(c, hipGetLastError());
  CutoffExtent ext;
  HIP_TRY(c, hipMemcpyAsync(&ext, d_part + nparts, sizeof(ext), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const CutoffGridView gv = cutoff_grid_view(ext, M, N, D, radius, c->opt_cutoff_factor);
  if (!cutoff_device_fits(N, M, gv.ncells)) return KMVP_OK;
  *fits = true;
  const int64_t ncells = gv.ncells, nrows = gv.nrows, g0 = gv.g[0];

  // ---- the tables at their bounds, the work buffer
  const int64_t tile_cap = cutoff_tiles_bound(N, nrows), run_cap = cutoff_runs_bound(N, nrows, D), rec_cap = cutoff_records_bound(M, nrows);
  if ((rc = ensure(c, c->ct_tiles, (size_t)tile_cap * sizeof(CutoffTile)))) return rc;
  if ((rc = ensure(c, c->ct_runs, (size_t)run_cap * sizeof(CutoffRun)))) return rc;
  if ((rc = ensure(c, c->ct_tmap, (size_t)tile_cap * CUTOFF_TILE * sizeof(int64_t)))) return rc;
  if ((rc = ensure(c, c->ct_smap, (size_t)rec_cap * sizeof(int64_t)))) return rc;
  const int bits = cutoff_key_bits(ncells);
  size_t tmp_bytes = 16, need = 0;
  uint32_t* nk = nullptr;
  int32_t* ni = nullptr;
  int64_t* nl = nullptr;
  if (M > 0) {
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, need, nk, nk, ni, ni, (int)M, 0, bits, st));
    tmp_bytes = std::max(tmp_bytes, need);
  }
  if (!same && N > 0) {
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, need, nk, nk, ni, ni, (int)N, 0, bits, st));
    tmp_bytes = std::max(tmp_bytes, need);
  }
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, need, nl, nl, (int)(nrows + 1), st));
  tmp_bytes = std::max(tmp_bytes, need);
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, need, nl, nl, (int)(tile_cap + 1), st));
  tmp_bytes = std::max(tmp_bytes, need);
  HIP_TRY(c, hipcub::DeviceReduce::Sum(nullptr, need, nl, nl, (int)tile_cap, st));
  tmp_bytes = std::max(tmp_bytes, need);

  Carver cv;
  const size_t o_skey_in = cv.take((size_t)M * 4), o_sidx_in = cv.take((size_t)M * 4), o_skey = cv.take((size_t)M * 4), o_sidx = cv.take((size_t)M * 4);
  const size_t o_sfirst = cv.take((size_t)(ncells + 1) * 4);
  const size_t tn = same ? 0 : (size_t)N;
  const size_t o_tkey_in = cv.take(tn * 4), o_tidx_in = cv.take(tn * 4), o_tkey = cv.take(tn * 4), o_tidx = cv.take(tn * 4);
  const size_t o_tfirst = cv.take(same ? 0 : (size_t)(ncells + 1) * 4);
  const size_t o_rowlen = cv.take((size_t)(nrows + 1) * 8), o_rowbase = cv.take((size_t)(nrows + 1) * 8);
  const size_t o_rowtiles = cv.take((size_t)(nrows + 1) * 8), o_tilebase = cv.take((size_t)(nrows + 1) * 8);
  const size_t o_nruns = cv.take((size_t)(tile_cap + 1) * 8), o_run0 = cv.take((size_t)(tile_cap + 1) * 8), o_walk = cv.take((size_t)tile_cap * 8);
  const size_t o_walked = cv.take(8), o_sizes = cv.take(5 * 8), o_tmp = cv.take(tmp_bytes);
  if ((rc = ensure(c, c->ct_work, cv.off))) return rc;
  char* w = (char*)c->ct_work.p;
  uint32_t *skey_in = (uint32_t*)(w + o_skey_in), *skey = (uint32_t*)(w + o_skey);
  int32_t *sidx_in = (int32_t*)(w + o_sidx_in), *sidx = (int32_t*)(w + o_sidx), *sfirst = (int32_t*)(w + o_sfirst);
  uint32_t *tkey_in = (uint32_t*)(w + o_tkey_in), *tkey = same ? skey : (uint32_t*)(w + o_tkey);
  int32_t *tidx_in = (int32_t*)(w + o_tidx_in), *tidx = same ? sidx : (int32_t*)(w + o_tidx), *tfirst = same ? sfirst : (int32_t*)(w + o_tfirst);
  int64_t *rowlen = (int64_t*)(w + o_rowlen), *rowbase = (int64_t*)(w + o_rowbase), *rowtiles = (int64_t*)(w + o_rowtiles);
  int64_t *tilebase = (int64_t*)(w + o_tilebase), *nruns = (int64_t*)(w + o_nruns), *run0 = (int64_t*)(w + o_run0);
  int64_t *walk = (int64_t*)(w + o_walk), *walked = (int64_t*)(w + o_walked), *d_sizes = (int64_t*)(w + o_sizes);
  void* tmp = w + o_tmp;

  // ---- keys, sort, first positions
  if (M > 0) {
    hipLaunchKernelGGL((cutoff_keys_kernel<real>), dim3(blocks_for(M)), dim3(CTP_THREADS), 0, st, y, M, gv, skey_in, sidx_in);
    HIP_TRY(c, hipGetLastError());
    size_t tb = tmp_bytes;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(tmp, tb, (const uint32_t*)skey_in, skey, (const int32_t*)sidx_in, sidx, (int)M, 0, bits, st));
  }
  hipLaunchKernelGGL(cutoff_first_kernel, dim3(blocks_for(ncells + 1)), dim3(CTP_THREADS), 0, st, (const uint32_t*)skey, M, ncells, sfirst);
  HIP_TRY(c, hipGetLastError());
  if (!same) {
    if (N > 0) {
      hipLaunchKernelGGL((cutoff_keys_kernel<real>), dim3(blocks_for(N)), dim3(CTP_THREADS), 0, st, x, N, gv, tkey_in, tidx_in);
      HIP_TRY(c, hipGetLastError());
      size_t tb = tmp_bytes;
      HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(tmp, tb, (const uint32_t*)tkey_in, tkey, (const int32_t*)tidx_in, tidx, (int)N, 0, bits, st));
    }
    hipLaunchKernelGGL(cutoff_first_kernel, dim3(blocks_for(ncells + 1)), dim3(CTP_THREADS), 0, st, (const uint32_t*)tkey, N, ncells, tfirst);
    HIP_TRY(c, hipGetLastError());
  }
  const CutoffSorted sv{skey, sidx, sfirst, M}, tv{tkey, tidx, tfirst, N};

  // ---- rows and their scans
  hipLaunchKernelGGL(cutoff_rows_kernel, dim3(blocks_for(nrows + 1)), dim3(CTP_THREADS), 0, st, (const int32_t*)sfirst, (const int32_t*)tfirst, g0,
                     nrows, rowlen, rowtiles);
  HIP_TRY(c, hipGetLastError());
  {
    size_t tb = tmp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(tmp, tb, (const int64_t*)rowlen, rowbase, (int)(nrows + 1), st));
    tb = tmp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(tmp, tb, (const int64_t*)rowtiles, tilebase, (int)(nrows + 1), st));
  }

  // ---- sources
  hipLaunchKernelGGL(cutoff_fill_kernel, dim3(blocks_for(rec_cap)), dim3(CTP_THREADS), 0, st, (int64_t*)c->ct_smap.p, rec_cap, (int64_t)-1);
  HIP_TRY(c, hipGetLastError());
  if (M > 0) {
    hipLaunchKernelGGL(cutoff_smap_kernel, dim3(blocks_for(M)), dim3(CTP_THREADS), 0, st, sv, (const int64_t*)rowbase, g0, ncells,
                       (int64_t*)c->ct_smap.p, rec_cap);
    HIP_TRY(c, hipGetLastError());
  }

  // ---- tiles, runs, tmap
  hipLaunchKernelGGL(cutoff_tile_count_kernel, dim3(blocks_for(tile_cap + 1)), dim3(CTP_THREADS), 0, st, tv, (const int64_t*)tilebase,
                     (const int32_t*)sfirst, (const int64_t*)rowbase, gv, tile_cap, nruns, walk);
  HIP_TRY(c, hipGetLastError());
  {
    size_t tb = tmp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(tmp, tb, (const int64_t*)nruns, run0, (int)(tile_cap + 1), st));
    tb = tmp_bytes;
    HIP_TRY(c, hipcub::DeviceReduce::Sum(tmp, tb, (const int64_t*)walk, walked, (int)tile_cap, st));
  }
  hipLaunchKernelGGL(cutoff_tile_write_kernel, dim3(blocks_for(tile_cap)), dim3(CTP_THREADS), 0, st, tv, (const int64_t*)tilebase,
                     (const int32_t*)sfirst, (const int64_t*)rowbase, gv, tile_cap, (const int64_t*)run0, run_cap, (CutoffTile*)c->ct_tiles.p,
                     (CutoffRun*)c->ct_runs.p);
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(cutoff_tmap_kernel, dim3(blocks_for(tile_cap * CUTOFF_TILE)), dim3(CTP_THREADS), 0, st, tv, (const int64_t*)tilebase, gv,
                     tile_cap, (int64_t*)c->ct_tmap.p);
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(cutoff_sizes_kernel, dim3(1), dim3(64), 0, st, tv, (const int64_t*)tilebase, (const int64_t*)rowbase, gv,
                     (const int64_t*)run0, tile_cap, (const int64_t*)walked, d_sizes);
  HIP_TRY(c, hipGetLastError());
  int64_t sizes[5] = {0, 0, 0, 0, 0};
  HIP_TRY(c, hipMemcpyAsync(sizes, d_sizes, sizeof(sizes), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (sizes[0] + CUTOFF_RECORDS > rec_cap || sizes[1] > tile_cap || sizes[2] > run_cap || sizes[0] < 0 || sizes[1] < 0 || sizes[2] < 0)
    return fail(c, KMVP_E_DEVICE, "cutoff radius: the device-built plan is beyond the bounds its tables were sized for");

  for (int d = 0; d < 3; ++d) {
    out->g[d] = gv.g[d];
    out->lo[d] = gv.lo[d];
  }
  out->h = gv.h;
  out->m_pad = sizes[0];
  out->m_alloc = sizes[0] + CUTOFF_RECORDS;
  out->tiles = sizes[1];
  out->n_pad = sizes[1] * CUTOFF_TILE;
  out->runs = sizes[2];
  out->walked = sizes[3];
  out->live_tiles = sizes[4];
  return KMVP_OK;
}

}  // namespace

int cutoff_plan_device(kmvp_ctx* c, double radius, CutoffBuilt* out, bool* fits) {
  return c->dtype == KMVP_F64 ? cutoff_plan_device_t<double>(c, radius, out, fits) : cutoff_plan_device_t<float>(c, radius, out, fits);
}

}  // namespace kmvp
