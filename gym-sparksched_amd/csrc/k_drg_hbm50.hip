// k_drg_hbm50.hip — greedy persistent Decima rollout (decima_rollout.h k_decima_rollout_greedy): hot block in HBM,
// 50 executors / 200 jobs. Compiled as k_dr_hbm50.hip is, in its own unit so that one is unchanged by it.
#define SSIM_OPAQUE_LANE 1
#include "decima_rollout.h"

DecimaRolloutFn decima_greedy_hbm50() { return k_decima_rollout_greedy<false, 50, 200>; }
