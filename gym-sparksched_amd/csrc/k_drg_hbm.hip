// k_drg_hbm.hip — greedy persistent Decima rollout (decima_rollout.h k_decima_rollout_greedy): hot block in HBM, any
// shape. Compiled as k_dr_hbm.hip is, in its own unit so that one is unchanged by it.
#define SSIM_OPAQUE_LANE 1
#define SSIM_EV_PAGES_GENERIC 2
#include "decima_rollout.h"

DecimaRolloutFn decima_greedy_hbm() { return k_decima_rollout_greedy<false>; }
