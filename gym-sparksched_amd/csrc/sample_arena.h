// sample_arena.h — the learner's sample arena (sparksched.h ssim_decima_samples) as a persistent rollout writes it: the
// contract between the rollout kernels (decima_rollout.h DecimaPolicy, teacher_rollout.h TeacherPolicy) and the PPO /
// behaviour-cloning learners, once, for any wave type (the test-only host build runs it on the one-lane wave).
//
// Per env: a cursor of kCurStride words, cap_samples records, and cap_nodes / cap_edges / cap_dags observation rows.
// Before a decision the driver asks arena_has_room (an env without room is marked full with what it needs; the host
// grows the arena and launches again), reads where the sample goes (arena_slot), decides, and arena_push writes the
// observation and the action there. After the step arena_reward completes the record; arena_take_back takes the sample
// of an action the env refused off again.
#pragma once
#include <stdint.h>

#include "engine.h"
#include "decima.h"

namespace ssim {

// The cursor words of one env (spark_sched_sim/_abi.py CUR_*; sparksched.h ssim_decima_samples::cursor): the records
// and node / edge / DAG rows used, the full mark (the env stopped: its next observation does not fit) and the rows that
// observation takes.
enum ArenaCursor : int {
  kCurSamples, kCurNodes, kCurEdges, kCurDags, kCurFull, kCurNeedNodes, kCurNeedEdges, kCurNeedDags, kCurStride
};
// The feature arrays of all envs (the ssim_decima_features layout), in the rollout's global workspace.
struct DecimaFeatArrays {
  float* feats;
  int32_t* ccap;
  uint32_t* emask;
  int32_t* depth;
};
// The recorded action, in Decima's action space.
struct ArenaAction {
  int32_t stage_idx, job_idx, exec_idx, num_exec;
  float lgprob;
};
// Where a sample goes: the sizes of the env's current observation and the cursor before it.
struct ArenaSlot {
  int n, ne, nj, cs, cn, ce, cg;
};

__device__ __forceinline__ int32_t* arena_cursor(const ssim_decima_samples& sm, int eid) {
  return sm.cursor + (int64_t)eid * kCurStride;
}
__device__ __forceinline__ const int32_t* arena_counts(const ssim_layout& L, const uint8_t* obs, int eid) {
  return reinterpret_cast<const int32_t*>(obs + L.ob_counts) + (int64_t)eid * SSIM_NUM_COUNTS;
}

// Whether the arena can take the env's current observation (one sample and its rows). If not: the full mark and the
// needs, for the host.
template <class W>
__device__ __forceinline__ bool arena_has_room(const ssim_decima_samples& sm, const ssim_layout& L, const uint8_t* obs,
                                               int eid) {
  const int32_t* cnt = arena_counts(L, obs, eid);
  int32_t* cur = arena_cursor(sm, eid);
  if (W::uni(cur[kCurSamples]) + 1 > sm.cap_samples ||
      W::uni(cur[kCurNodes]) + W::uni(cnt[SSIM_OC_NUM_NODES]) > sm.cap_nodes ||
      W::uni(cur[kCurEdges]) + W::uni(cnt[SSIM_OC_NUM_EDGES]) > sm.cap_edges ||
      W::uni(cur[kCurDags]) + W::uni(cnt[SSIM_OC_NUM_JOBS]) > sm.cap_dags) {
    W::sync();
    if (W::lane() == 0) {  // region full: the host grows the arena (to fit what is recorded here), launches again
      cur[kCurFull] = 1;
      cur[kCurNeedNodes] = W::uni(cnt[SSIM_OC_NUM_NODES]);
      cur[kCurNeedEdges] = W::uni(cnt[SSIM_OC_NUM_EDGES]);
      cur[kCurNeedDags] = W::uni(cnt[SSIM_OC_NUM_JOBS]);
    }
    W::sync();
    return false;
  }
  return true;
}

// Where the env's next sample goes; `have_arena` false (a driver that records nothing): the sizes only, cursor zero.
template <class W>
__device__ __forceinline__ ArenaSlot arena_slot(const ssim_decima_samples& sm, const ssim_layout& L, const uint8_t* obs,
                                                int eid, bool have_arena = true) {
  const int32_t* cnt = arena_counts(L, obs, eid);
  ArenaSlot at{W::uni(cnt[SSIM_OC_NUM_NODES]), W::uni(cnt[SSIM_OC_NUM_EDGES]), W::uni(cnt[SSIM_OC_NUM_JOBS]),
               0, 0, 0, 0};
  if (have_arena) {
    const int32_t* cur = arena_cursor(sm, eid);
    at.cs = W::uni(cur[kCurSamples]);
    at.cn = W::uni(cur[kCurNodes]);
    at.ce = W::uni(cur[kCurEdges]);
    at.cg = W::uni(cur[kCurDags]);
  }
  return at;
}

// The env's current observation as the learner's DagBatch rows (schedulers/decima.py build_batch: per node the features
// and the schedulable flag, per edge the links and the mask word, per DAG its size and executor cap), the record, and
// the cursor past them. `fa`: the features of this observation (decima.h DecimaView::run).
template <class W>
__device__ __forceinline__ void arena_push(const ssim_decima_samples& sm, const ssim_layout& L, const uint8_t* obs,
                                           int eid, const DecimaFeatArrays& fa, const ArenaSlot& at,
                                           const ArenaAction& act, double wall_before) {
  const int n = at.n, ne = at.ne, nj = at.nj;
  const int cs = at.cs, cn = at.cn, ce = at.ce, cg = at.cg;
  const float* f = fa.feats + (int64_t)eid * L.stage_cap * kDecimaFeatures;
  const float* nodes = reinterpret_cast<const float*>(obs + L.ob_nodes) + (int64_t)eid * L.stage_cap * 3;
  const int64_t* links = reinterpret_cast<const int64_t*>(obs + L.ob_edge_links) + (int64_t)eid * L.edge_cap * 2;
  const int32_t* ptr = reinterpret_cast<const int32_t*>(obs + L.ob_dag_ptr) + (int64_t)eid * (L.job_cap + 1);
  const int32_t* cc = fa.ccap + (int64_t)eid * L.job_cap;
  const uint32_t* em = fa.emask + (int64_t)eid * L.edge_cap;
  float* xn = sm.nodes + ((int64_t)eid * sm.cap_nodes + cn) * 6;
  for (int i = W::lane(); i < n; i += W::kWidth) {
#pragma unroll
    for (int c = 0; c < kDecimaFeatures; ++c) xn[(int64_t)i * 6 + c] = f[(int64_t)i * kDecimaFeatures + c];
    xn[(int64_t)i * 6 + 5] = nodes[3 * i + 2];
  }
  int32_t* ed = sm.edges + ((int64_t)eid * sm.cap_edges + ce) * 4;
  for (int e = W::lane(); e < ne; e += W::kWidth) {
    ed[4 * e + 0] = (int32_t)links[2 * e];
    ed[4 * e + 1] = (int32_t)links[2 * e + 1];
    ed[4 * e + 2] = (int32_t)em[e];
    ed[4 * e + 3] = 0;
  }
  int32_t* dg = sm.dags + ((int64_t)eid * sm.cap_dags + cg) * 2;
  for (int k = W::lane(); k < nj; k += W::kWidth) {
    dg[2 * k + 0] = ptr[k + 1] - ptr[k];
    dg[2 * k + 1] = cc[k];
  }
  const int dep = W::uni(fa.depth[eid]);
  W::sync();
  if (W::lane() == 0) {
    int32_t* cur = arena_cursor(sm, eid);
    // (the record's fields in order: sizes, depth, row offsets, the action, wall_before, the reward arena_reward fills)
    sm.rec[(int64_t)eid * sm.cap_samples + cs] = ssim_decima_sample{
        n, ne, nj, dep, cn, ce, cg, act.stage_idx, act.job_idx, act.exec_idx, act.num_exec, act.lgprob, wall_before,
        0.0};
    cur[kCurSamples] = cs + 1;
    cur[kCurNodes] = cn + n;
    cur[kCurEdges] = ce + ne;
    cur[kCurDags] = cg + nj;
  }
  W::sync();
}

// The decision's reward (observe() wrote it to the obs arena) into its sample, the env's last.
template <class W>
__device__ __forceinline__ void arena_reward(const ssim_decima_samples& sm, const ssim_layout& L, const uint8_t* obs,
                                             int eid) {
  const int cs = W::uni(arena_cursor(sm, eid)[kCurSamples]);
  const double r = W::uni(reinterpret_cast<const double*>(obs + L.ob_reward)[eid]);
  W::sync();
  if (W::lane() == 0 && cs > 0) sm.rec[(int64_t)eid * sm.cap_samples + cs - 1].reward = r;
  W::sync();
}

// The env refused the recorded action (it is frozen with SSIM_ERR_INVARIANT, the collector raises): the env's last
// sample and its observation rows come off the arena, so no sample ever holds an action the env did not take.
template <class W>
__device__ __forceinline__ void arena_take_back(const ssim_decima_samples& sm, int eid) {
  W::sync();
  if (W::lane() == 0) {
    int32_t* cur = arena_cursor(sm, eid);
    const int cs = cur[kCurSamples];
    if (cs > 0) {
      const ssim_decima_sample& r = sm.rec[(int64_t)eid * sm.cap_samples + cs - 1];
      cur[kCurNodes] -= r.num_nodes;
      cur[kCurEdges] -= r.num_edges;
      cur[kCurDags] -= r.num_dags;
      cur[kCurSamples] = cs - 1;
    }
  }
  W::sync();
}

}  // namespace ssim
