// teacher.cpp — TEST-ONLY host build of the teacher rollout's driver (csrc/teacher_rollout.h TeacherPolicy) under the
// fused rollouts' decision loop (rollout.h rollout_loop) on the eager engine, with a one-lane wave and no budget: what
// the device's k_teacher_rollout runs per env. Shares hostsim.cpp's handle and wave type (one shared object:
// teacher_driver.py).
#include "hostsim.cpp"
#include "teacher_rollout.h"

namespace ssim {
template <class S>
uint8_t* teacher_lds(const S& s, int32_t off) {
  return s.scr + off;
}

// The step's reward in the DEVICE's summation order. engine.h jobtime adds the jobs' time shares per lane (lane l takes
// jobs l, l + 64, ... in order) and then folds the 64 lane sums with the xor butterfly of WaveHip::sum_d (offsets 32, 16,
// ..., 1); the one-lane wave adds the same terms serially, which rounds differently in the last bit now and then (the
// oracle audits compare rewards at 1e-9 relative for that reason). A sample arena is a device artefact, so the host
// build records the reward as the device rounds it: the same terms, the device's order. Only for beta = 0, where every
// term is an exact float64 difference on both sides (with beta > 0 the terms themselves go through exp, and the serial
// value stands). t0: the wall time before the step (the sample's wall_before); state as finish_step left it.
template <class S>
double wave_order_reward(S& s, double t0, double serial) {
  if (serial == 0.0 || s.C.beta != 0.0) return serial;  // (no term, or all zero: any order gives 0)
  const double wall = s.h.wall;
  const int dec = s.h.decisions;
  double x[64] = {0.0};
  for (int j = 0; j < s.h.arrivals; ++j) {
    const JobRec jr = s.job(j);
    const JobTimes jt = s.jtimes(j);
    const int st = jr.state;
    if (!(st == kJobActive || (st == kJobDone && jr.done_dec == dec && jr.arr_dec < dec))) continue;
    const double a = jt.tarr > t0 ? jt.tarr : t0;
    const double tc = st == kJobDone ? jt.tdone : wall;
    const double b = tc < wall ? tc : wall;
    x[j & 63] += b - a;
  }
  for (int off = 32; off > 0; off >>= 1) {
    double y[64];
    for (int l = 0; l < 64; ++l) y[l] = x[l] + x[l ^ off];
    memcpy(x, y, sizeof(x));
  }
  return -x[0];
}

// TeacherPolicy whose samples carry the reward in the device's summation order (above); everything else is the driver.
struct HostTeacherPolicy : TeacherPolicy {
  template <class S>
  void done(S& s) const {
    TeacherPolicy::done(s);
    const int cs = arena_cursor(a.smp, s.eid)[kCurSamples];
    if (cs <= 0) return;
    ssim_decima_sample& r = a.smp.rec[(int64_t)s.eid * a.smp.cap_samples + cs - 1];
    r.reward = wave_order_reward(s, r.wall_before, r.reward);
  }
};
}  // namespace ssim

extern "C" {

// ssim_teacher_rollout: `work` holds what the device workspace holds for the driver (teacher_driver.py lays it out):
// per env `stride` bytes of global feature scratch, then the four feature arrays at the given byte offsets. An
// observation of at most plan_cap nodes and plan_dags DAGs keeps the features' scratch in the emulated LDS, after the
// engine's scratch.
int hs_teacher_rollout(hs_handle* h, int kind, uint64_t seed, float nts, float ws, int max_steps, uint8_t* work,
                       int64_t stride, int64_t feats, int64_t ccap, int64_t emask, int64_t depth, int plan_cap, int plan_dags,
                       const ssim_decima_samples* samples, int32_t* action_log) {
  using SimT = Sim<WaveSerial, 0, 0, 0, false>;
  const Params* P = h->params;
  const int B = P->L.num_envs;
  if (samples == nullptr || work == nullptr || max_steps < 0) return -1;
  const int32_t plan_off = (int32_t)align16(P->L.scratch_bytes);
  const int64_t lds_bytes = (h->resident ? P->O.hot_bytes : 0) + plan_off + decima_scratch_bytes(plan_cap > 0 ? plan_cap : 1);
  uint8_t* lds = (uint8_t*)malloc((size_t)lds_bytes);
  TeacherArgs a{};
  a.work = work;
  a.stride = stride;
  a.feats = reinterpret_cast<float*>(work + feats);
  a.ccap = reinterpret_cast<int32_t*>(work + ccap);
  a.emask = reinterpret_cast<uint32_t*>(work + emask);
  a.depth = reinterpret_cast<int32_t*>(work + depth);
  a.num_tasks_scale = nts;
  a.work_scale = ws;
  a.kind = kind;
  a.seed = seed;
  a.plan_cap = plan_cap;
  a.plan_off = plan_off;
  a.plan_dags = plan_dags;
  a.smp = *samples;
  for (int e = 0; e < B; ++e) {
    memset(lds, kPoison, (size_t)lds_bytes);  // (as resident_lds: a read of what the copy does not cover shows up)
    SimT s(P, h->state, lds, h->obs, e, h->resident != 0, /*row_cold=*/h->resident == 0, /*ex_lds=*/false);
    uint8_t* rec = h->reset + (int64_t)e * P->L.reset_stride;
    const auto reset_in_place = [&](SimT& x) { x.reset_sampled(SSIM_RESET_CONTINUE, 0ull, __builtin_inf(), rec); };
    RolloutCursor c{0, 0, 0};
    const NoBudget stop;
    const HostTeacherPolicy pol{{P, h->obs, a}};
    s.load_hot();
    rollout_loop(s, pol, stop, c, B, e, max_steps, false, action_log, reset_in_place);
    s.save_hot();
  }
  free(lds);
  return 0;
}

// One call of sample_arena.h on the one-lane wave, no engine: env `eid` of a hand-made observation arena `obs` (byte
// offsets ob = {counts, nodes, edge_links, dag_ptr, reward}, row caps = {stage, edge, job}) and feature arrays `fa`.
// op 0: arena_has_room (returned), 1: arena_push of `act` = {stage_idx, job_idx, exec_idx, num_exec}, lgprob and
// wall_before at the cursor, 2: arena_reward, 3: arena_take_back.
int hs_arena_op(int op, const ssim_decima_samples* sm, int eid, const uint8_t* obs, const int64_t* ob,
                const int32_t* caps, float* feats, int32_t* ccap, uint32_t* emask, int32_t* depth, const int32_t* act,
                float lgprob, double wall_before) {
  using W = WaveSerial;
  ssim_layout L{};
  L.ob_counts = ob[0], L.ob_nodes = ob[1], L.ob_edge_links = ob[2], L.ob_dag_ptr = ob[3], L.ob_reward = ob[4];
  L.stage_cap = caps[0], L.edge_cap = caps[1], L.job_cap = caps[2];
  switch (op) {
    case 0: return arena_has_room<W>(*sm, L, obs, eid);
    case 1:
      arena_push<W>(*sm, L, obs, eid, {feats, ccap, emask, depth}, arena_slot<W>(*sm, L, obs, eid),
                    {act[0], act[1], act[2], act[3], lgprob}, wall_before);
      return 0;
    case 2: arena_reward<W>(*sm, L, obs, eid); return 0;
    case 3: arena_take_back<W>(*sm, eid); return 0;
  }
  return -1;
}

}  // extern "C"
