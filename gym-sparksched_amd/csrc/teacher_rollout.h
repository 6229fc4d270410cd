// teacher_rollout.h — teacher rollouts: a device heuristic drives the env in ONE persistent launch and every decision is
// left in a Decima sample arena (sparksched.h ssim_decima_samples), in the form the PPO learner consumes.
//
// The heuristic drivers of rollout.h (HeuristicPolicy, PrioPolicy, WfairPolicy) read only the hot block and never form
// the Decima observation; the persistent Decima rollout (decima_rollout.h DecimaPolicy) records it, but only for the
// GNN policy's own actions. TeacherPolicy is the driver between them: per decision the Decima features of the current
// observation (decima.h DecimaView, the path of ssim_decima_features and decima_decide), the action of any heuristic
// kind (policy.h sim_policy: fair / FIFO / random / SJF / SJF-CP / weighted fair), and one ssim_decima_sample with the
// observation's node, edge and DAG rows, laid out exactly as DecimaPolicy::act lays them out. No GNN runs, so there is
// no policy plan and no packed weights: the only per-decision scratch is the features' (10 B per node), in the wave's
// LDS when the observation fits the Decima rollout's LDS plan (so a teacher collection runs the features where a Decima
// collection of the same observations runs them), else in the env's block of the global workspace.
//
// The recorded action, in Decima's action space: stage_idx the heuristic's (already an index among the schedulable
// stages), num_exec the value handed to the step, job_idx the active-job (DAG) index of the chosen stage's node row,
// exec_idx = num_exec - 1, lgprob = 0. A NO-OP decision (the heuristic returns stage_idx = -1: nothing schedulable it
// wants) IS recorded, as stage_idx = -1, job_idx = -1, exec_idx = 0 and the num_exec passed to the step, so the
// trajectory, its times and rewards stay complete; the behaviour-cloning trainer masks those samples out.
//
// The arena is written through sample_arena.h, as DecimaPolicy writes it.
//
// The driver is independent of the wave type (the test-only host build runs it on the one-lane wave,
// tests/hostsim/teacher.cpp); the kernels at the end are device-only.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include "engine.h"
#include "policy.h"
#include "rollout.h"
#include "decima.h"
#include "sample_arena.h"

namespace ssim {

struct TeacherArgs : DecimaFeatArrays {  // (the [num_envs] feature arrays, in the workspace)
  uint8_t* work;    // the global workspace: env e's feature scratch at work + e * stride (decima_rollout.h decima_work)
  int64_t stride;
  float num_tasks_scale, work_scale;
  int32_t kind;     // SSIM_POLICY_*
  uint64_t seed;    // (the random kind's counter-based stream)
  // An observation of at most plan_cap nodes and plan_dags DAGs (the rule of the Decima rollout's LDS plan,
  // decima_rollout.h DecimaPolicy::act) runs the features' scratch in the wave's LDS, at byte plan_off of its scratch
  // block (that plan's offset); larger ones use the env's global block.
  int32_t plan_cap, plan_off, plan_dags;
  ssim_decima_samples smp;
};

// The wave's LDS at byte `off` of the env's scratch block. Device: as an offset from the LDS base, so the features'
// scratch accesses compile to ds instructions (decima_rollout.h passes its plan the same way).
template <class S>
__device__ __forceinline__ uint8_t* teacher_lds(const S& s, int32_t off);

// The active-job (DAG) index of the `rank`-th schedulable node row of the observation (-1: no such row).
template <class W>
__device__ __forceinline__ int teacher_job_of(const float* nodes, const int32_t* ptr, int n, int nj, int rank) {
  int row = -1, seen = 0;
  for (int i0 = 0; i0 < n && row < 0; i0 += W::kWidth) {
    const int i = i0 + W::lane();
    uint64_t m = W::ballot(i < n && nodes[3 * i + 2] != 0.0f);
    const int c = W::popc(m);
    if (rank < seen + c) {
      for (int t = rank - seen; t > 0; --t) m &= m - 1;
      row = i0 + W::ffs(m);
    }
    seen += c;
  }
  if (row < 0) return -1;
  int job = -1;
  for (int k0 = 0; k0 < nj && job < 0; k0 += W::kWidth) {
    const int k = k0 + W::lane();
    const uint64_t m = W::ballot(k < nj && ptr[k] <= row && row < ptr[k + 1]);
    if (m != 0) job = k0 + W::ffs(m);
  }
  return job;
}

struct TeacherPolicy {
  static constexpr bool kTimedMode = false;
  static constexpr bool kLazyRows = false;  // the features and the samples read the arena rows at every decision
  const Params* P;
  const uint8_t* obs;
  TeacherArgs a;

  // Collection mode only: not when the episode is over (terminated, past its time limit, frozen, never reset), and not
  // when the sample arena cannot hold the current observation (the host grows the arena and launches again).
  template <class S>
  __device__ __forceinline__ bool can_act(const S& s) const {
    using W = typename S::WT;
    if (s.h.terminated || s.frozen() || s.h.wall >= s.h.time_limit || s.h.num_jobs == 0) return false;
    return arena_has_room<W>(a.smp, P->L, obs, s.eid);
  }

  template <class S>
  __device__ __forceinline__ bool act(S& s, int /*k*/, StepIn* out) const {
    using W = typename S::WT;
    const ssim_layout& L = P->L;
    const int eid = s.eid;
    const ArenaSlot at = arena_slot<W>(a.smp, L, obs, eid);
    // 1. the Decima features of the observation
    if (at.n <= a.plan_cap && at.nj <= a.plan_dags)
      DecimaView<W>{L, obs, eid}.template run<false>(a.num_tasks_scale, a.work_scale, teacher_lds(s, a.plan_off),
                                                     a.feats, a.ccap, a.emask, a.depth, a.plan_cap);
    else
      DecimaView<W>{L, obs, eid}.template run<true>(a.num_tasks_scale, a.work_scale, a.work + (int64_t)eid * a.stride,
                                                    a.feats, a.ccap, a.emask, a.depth);
    // 2. the heuristic's action
    const StepIn act = sim_policy(s, a.kind, a.seed);
    *out = act;
    // 3. the sample: the action in Decima's action space (a no-op as stage_idx = job_idx = -1, exec_idx = 0)
    const float* nodes = reinterpret_cast<const float*>(obs + L.ob_nodes) + (int64_t)eid * L.stage_cap * 3;
    const int32_t* ptr = reinterpret_cast<const int32_t*>(obs + L.ob_dag_ptr) + (int64_t)eid * (L.job_cap + 1);
    const int stage = W::uni(act.stage_idx), nexec = W::uni(act.num_exec);
    const int job = stage >= 0 ? teacher_job_of<W>(nodes, ptr, at.n, at.nj, stage) : -1;
    arena_push<W>(a.smp, L, obs, eid, a, at,
                  {stage >= 0 ? stage : -1, stage >= 0 ? job : -1, stage >= 0 ? nexec - 1 : 0, nexec, 0.0f}, s.h.wall);
    return true;
  }

  // the decision's reward (observe() wrote it to the obs arena) into its sample
  template <class S>
  __device__ __forceinline__ void done(S& s) const {
    arena_reward<typename S::WT>(a.smp, P->L, obs, s.eid);
  }

  // The env refused the recorded action (it is frozen with SSIM_ERR_INVARIANT): the sample and its rows come off the
  // arena.
  template <class S>
  __device__ __forceinline__ void rejected(S& s) const {
    arena_take_back<typename S::WT>(a.smp, s.eid);
  }
};

}  // namespace ssim

#ifdef __HIPCC__
#include "kernels.h"

namespace ssim {
template <class S>
__device__ __forceinline__ uint8_t* teacher_lds(const S& s, int32_t off) {
  return g_smem + (uint32_t)(s.scr + off - g_smem);
}
}  // namespace ssim

// The teacher rollout of one residency, any shape, all policy kinds (k_tr_lds.hip, k_tr_hbm.hip: the flags of their
// k_prio_* / k_wfair_* siblings). The engine runs as under the persistent Decima rollout: eager arena rows, observe()'s
// row map in the cold block of an HBM-resident env (the LDS the layout leaves goes to the features' scratch), the
// executor records where SSIM_DR_EX_LDS puts them, so the LDS plan offset of that rollout holds here too.
#ifndef SSIM_DR_EX_LDS
#define SSIM_DR_EX_LDS 0
#endif
template <bool kRes>
__global__ __attribute__((amdgpu_flat_work_group_size(1, 64), amdgpu_waves_per_eu(SSIM_ROLLOUT_WAVES(kRes)))) void k_teacher_rollout(
    const Params* __restrict__ P, uint8_t* state, uint8_t* obs, TeacherArgs a, int num_steps, uint8_t* reset,
    int32_t* action_log) {
  const TeacherPolicy pol{P, obs, a};
  rollout_body<kRes, 0, 0, 0, TeacherPolicy>(P, state, obs, pol, num_steps, 0, nullptr, reset, action_log, nullptr, 0,
                                             nullptr, !kRes, SSIM_DR_EX_LDS != 0);
}

using TeacherRolloutFn = void (*)(const Params*, uint8_t*, uint8_t*, TeacherArgs, int, uint8_t*, int32_t*);
TeacherRolloutFn teacher_rollout_lds();  // k_tr_lds.hip: LDS-resident, any shape
TeacherRolloutFn teacher_rollout_hbm();  // k_tr_hbm.hip: hot block in HBM, any shape
#endif
