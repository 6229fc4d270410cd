// k_tr_hbm.hip — teacher rollout kernel (teacher_rollout.h): hot block in HBM, any shape (the flags of k_prio_hbm.hip /
// k_wfair_hbm.hip / k_hbm.hip: register event slots for up to 128 executors, the lane index opaque at every use).
#define SSIM_OPAQUE_LANE 1
#define SSIM_EV_PAGES_GENERIC 2
#include "teacher_rollout.h"

TeacherRolloutFn teacher_rollout_hbm() { return k_teacher_rollout<false>; }
