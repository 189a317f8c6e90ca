// The integer rules of DBSCAN's rounds and of its renumbering (include/kmvp.h kmvp_dbscan; driver: kmvp_dbscan.hip).
//
// State per point, int32 (N < 2^31): lab[i] is a core index of i's component with lab[i] <= i for a core point, DB_NONE
// otherwise.  Between rounds every label is a ROOT: lab[lab[i]] == lab[i].  One round, after the sweep has left
// nxt[i] = the smallest label among i's inside core points (nxt[i] <= lab[i], the point's own pair is inside):
//   db_hook    a core point whose nxt fell asks its root to hook below: par[lab[i]] = min(par[lab[i]], nxt[i]), par a copy
//              of lab.  nxt[i] is a label, hence a root smaller than lab[i]: roots only ever hook to smaller roots, par
//              has no cycle, and since only minima are taken its final state does not depend on the order of the requests.
//   db_chase   every core point follows par, read-only, to the root r with par[r] == r: its new label.
// A round that hooks nothing leaves lab constant on every component and equal to the component's smallest core index: the
// fixed point.  Every other round removes at least one root, so there are at most N rounds.
// After the fixed point: db_root flags the roots, an exclusive scan of the flags numbers the clusters 0 .. C - 1 in
// ascending order of their roots, db_core_of and db_label write a point's row.
//
// Plain C++ with the device attributes behind a macro: the same text runs in kmvp_dbscan.hip's kernels and, compiled with
// a host compiler alone, in tests/test_host_dbscan_step.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KMVP_HD __host__ __device__
#else
#define KMVP_HD
#endif

namespace kmvp {

constexpr int32_t DB_NONE = INT32_MAX;  // the label of a point that is no core point (LABEL_NONE of the pair loop)

// counts[i] is kmvp_radius_count's value (the point itself included, -1 for a NaN point); min_samples >= 1
KMVP_HD inline int32_t db_initial_label(int64_t count, int64_t min_samples, int64_t i) {
  return count >= min_samples ? (int32_t)i : DB_NONE;
}

// The request of point i: true where par[*slot] is to fall to *value (a minimum: atomicMin on the device).
KMVP_HD inline bool db_hook(int32_t lab_i, int32_t nxt_i, int32_t* slot, int32_t* value) {
  if (lab_i == DB_NONE || !(nxt_i < lab_i)) return false;
  *slot = lab_i;
  *value = nxt_i;
  return true;
}

// The root of core point i in par.  par[i] <= i along the way, strictly until the root: the walk ends.
KMVP_HD inline int32_t db_chase(const int32_t* par, int32_t i) {
  int32_t r = par[i];
  while (par[r] != r) r = par[r];
  return r;
}

KMVP_HD inline int32_t db_root(int32_t lab_i, int64_t i) { return lab_i != DB_NONE && (int64_t)lab_i == i ? 1 : 0; }

// core_of[i]: the point itself for a core point, the core point a border point was attached to (attach_i, -1: none
// inside), -1 for noise.
KMVP_HD inline int64_t db_core_of(int32_t lab_i, int32_t attach_i, int64_t i) {
  return lab_i != DB_NONE ? i : (int64_t)attach_i;
}

// labels[i] from core_of[i]: the cluster number of that core point's root; cid is the exclusive scan of db_root.
KMVP_HD inline int64_t db_label(int64_t core_of_i, const int32_t* lab, const int32_t* cid) {
  return core_of_i < 0 ? (int64_t)-1 : (int64_t)cid[lab[core_of_i]];
}

}  // namespace kmvp
