// wfair_kat.cpp — TEST-ONLY host build of the weighted-fair arithmetic of gym-sparksched_amd/csrc/policy.h
// (wfair_weight, wfair_total, wfair_cap) behind one C function, for the known-answer test against numpy
// (tests/test_weighted_fair.py). The device runs the same functions through ssim_debug_wfair.
#define __device__
#define __host__
#define __forceinline__ inline
#define __constant__
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "engine.h"
#include "policy.h"
#include "units.h"

using namespace ssim;

// The weighted-fair row of the kernel-unit rule (units.h): the unit's name for a layout.
extern "C" const char* wk_unit_name(const ssim_layout* L, int lds_resident, int generic) {
  return wfair_unit_name(wfair_unit(*L, lds_resident != 0, generic != 0));
}

struct WaveOne {  // the one-lane wave of the host build: wfair_total folds a local array per block of 64
  static constexpr int kWidth = 1;
  static int lane() { return 0; }
};

extern "C" int wk_run(const double* W, int32_t n, int32_t alpha2, int32_t num_executors, double* p, double* P,
                      int32_t* cap) {
  if (n < 1 || alpha2 < -4 || alpha2 > 4 || num_executors < 1) return -1;
  double keep[kWfairKeep];
  const double tot = wfair_total<WaveOne>(n, [&](int k) { return wfair_weight(W[k], alpha2); }, keep);
  for (int k = 0; k < n; ++k) {
    p[k] = wfair_weight(W[k], alpha2);
    cap[k] = tot > 0.0 ? wfair_cap(num_executors, p[k], tot) : 0;
  }
  *P = tot;
  return 0;
}
