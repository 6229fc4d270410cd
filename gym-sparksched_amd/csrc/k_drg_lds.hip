// k_drg_lds.hip — greedy persistent Decima rollout (decima_rollout.h k_decima_rollout_greedy): hot block LDS-resident,
// any shape. Compiled as k_dr_lds.hip is, in its own unit so that one is unchanged by it.
#define SSIM_DP_PIPELINE 1  // (one wave per SIMD: decima_policy.h dp_layer_in_p)
#include "decima_rollout.h"

DecimaRolloutFn decima_greedy_lds() { return k_decima_rollout_greedy<true>; }
