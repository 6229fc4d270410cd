// k_drg_lds50.hip — greedy persistent Decima rollout (decima_rollout.h k_decima_rollout_greedy): hot block
// LDS-resident, 50 executors / 200 jobs, with the exec-score helper waves (evaluating a policy on a PPO iteration's 16
// envs). Compiled as k_dr_lds50.hip is, in its own unit so that one is unchanged by it.
#define SSIM_DP_PIPELINE 1  // (one wave per SIMD: decima_policy.h dp_layer_in_p)
#include "decima_rollout.h"

DecimaRolloutFn decima_greedy_lds50() { return k_decima_rollout_greedy<true, 50, 200, true>; }
