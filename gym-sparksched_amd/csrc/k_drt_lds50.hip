// k_drt_lds50.hip — fixed-duration persistent Decima rollout (decima_rollout.h k_decima_rollout_timed): hot block
// LDS-resident, 50 executors / 200 jobs, with the exec-score helper waves: the 16 rows of a PPO iteration with
// rollout_duration set. Compiled as k_dr_lds50.hip is, in its own unit so that one is unchanged by it.
#define SSIM_DP_PIPELINE 1  // (one wave per SIMD: decima_policy.h dp_layer_in_p)
#include "decima_rollout.h"

DecimaTimedFn decima_timed_lds50() { return k_decima_rollout_timed<true, 50, 200, true>; }
