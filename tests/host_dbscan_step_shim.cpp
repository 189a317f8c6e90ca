// Host-side shim for tests/test_host_dbscan_step.py: csrc/kmvp_dbscan_step.hpp (the integer rules of DBSCAN's rounds and of
// its renumbering) compiled with a host compiler alone, behind a C surface.  The launches of csrc/kmvp_dbscan.hip are
// restated as loops over the points; the hook's atomicMin is a minimum taken in the order `order` visits the points, so
// that a test can show that the order does not matter.
#include "kmvp_dbscan_step.hpp"

extern "C" {

int hs_none(void) { return kmvp::DB_NONE; }

void hs_init(const int64_t* counts, int64_t min_samples, int32_t* lab, int64_t n) {
  for (int64_t i = 0; i < n; ++i) lab[i] = kmvp::db_initial_label(counts[i], min_samples, i);
}

// par = lab, then every point's request in the order given; returns the number of requests
int64_t hs_hook(const int32_t* lab, const int32_t* nxt, int32_t* par, const int64_t* order, int64_t n) {
  int64_t asked = 0;
  for (int64_t i = 0; i < n; ++i) par[i] = lab[i];
  for (int64_t t = 0; t < n; ++t) {
    const int64_t i = order[t];
    int32_t slot, value;
    if (kmvp::db_hook(lab[i], nxt[i], &slot, &value)) {
      par[slot] = value < par[slot] ? value : par[slot];
      ++asked;
    }
  }
  return asked;
}

void hs_chase(const int32_t* par, int32_t* lab, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (par[i] != kmvp::DB_NONE) lab[i] = kmvp::db_chase(par, (int32_t)i);
}

// flags, their exclusive scan, core_of and labels; returns the number of clusters
int64_t hs_renumber(const int32_t* lab, const int32_t* attach, int32_t* flag, int32_t* cid, int64_t* labels, int64_t* core_of,
                    int64_t n) {
  int32_t run = 0;
  for (int64_t i = 0; i < n; ++i) {
    flag[i] = kmvp::db_root(lab[i], i);
    cid[i] = run;
    run += flag[i];
  }
  for (int64_t i = 0; i < n; ++i) {
    core_of[i] = kmvp::db_core_of(lab[i], attach[i], i);
    labels[i] = kmvp::db_label(core_of[i], lab, cid);
  }
  return run;
}

}
