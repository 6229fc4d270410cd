// k_tr_lds.hip — teacher rollout kernel (teacher_rollout.h): LDS-resident, any shape (the flags of k_prio_lds.hip /
// k_wfair_lds.hip / k_lds.hip).
#include "teacher_rollout.h"

TeacherRolloutFn teacher_rollout_lds() { return k_teacher_rollout<true>; }
