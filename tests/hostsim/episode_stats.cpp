// episode_stats.cpp — TEST-ONLY host restatement of ssim_episode_stats (gym-sparksched_amd/csrc/sparksched.hip
// k_episode_stats) as a serial loop over a state arena of the host build of the engine (hostsim.cpp: the arena starts
// with its Params). Built on its own (tests/host_episode_stats.py); not part of the product.
#define __device__
#define __host__
#define __forceinline__ inline
#define __constant__
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "engine.h"

using namespace ssim;

// out [num_envs][4] = sum over arrived jobs of min(t_completed, wall) - t_arrival, arrived jobs, completed jobs, wall
extern "C" void hs_episode_stats(const uint8_t* state, double* out) {
  const Params* P = reinterpret_cast<const Params*>(state);
  const int J = P->L.job_cap;
  for (int e = 0; e < P->L.num_envs; ++e) {
    const uint8_t* hot = state + kParamsReserve + (int64_t)e * P->L.env_bytes;
    const double wall = reinterpret_cast<const EnvHeader*>(hot)->wall;
    const JobRec* jr = reinterpret_cast<const JobRec*>(hot + P->O.jobs);
    const JobTimes* jt = reinterpret_cast<const JobTimes*>(hot + P->O.jtimes);
    double sum = 0.0;
    int arrived = 0, completed = 0;
    for (int j = 0; j < J; ++j) {
      if (jr[j].state == kJobPending) continue;
      sum += (jt[j].tdone < wall ? jt[j].tdone : wall) - jt[j].tarr;
      ++arrived;
      completed += jr[j].state == kJobDone;
    }
    out[4 * e + 0] = sum;
    out[4 * e + 1] = arrived;
    out[4 * e + 2] = completed;
    out[4 * e + 3] = wall;
  }
}
