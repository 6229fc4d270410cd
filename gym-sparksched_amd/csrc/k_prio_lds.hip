// k_prio_lds.hip — SJF / SJF-CP rollout kernel: LDS-resident, any shape (the flags of k_lds.hip).
#include "kernels.h"

RolloutFn rollout_prio_lds() { return k_rollout_prio<true>; }
