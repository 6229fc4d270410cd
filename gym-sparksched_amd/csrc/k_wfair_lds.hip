// k_wfair_lds.hip — weighted-fair rollout kernel: LDS-resident, any shape (the flags of k_prio_lds.hip / k_lds.hip).
#include "kernels.h"

RolloutFn rollout_wfair_lds() { return k_rollout_wfair<true>; }
