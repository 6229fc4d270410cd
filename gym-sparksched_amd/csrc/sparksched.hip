// sparksched.hip — gfx950 kernels and the C ABI (include/sparksched.h).
//
// One 64-lane wavefront per env (one workgroup = one wave; no workgroup barriers needed). Per-env state
// lives in the caller's state arena in HBM (env-major SoA, layout.h); per-launch scratch (node row map,
// temporary CPython-set tables, commitment plan) lives in LDS. Kernels:
//   k_reset   : env init from a host-sampled job sequence + _load_initial_jobs + first observation
//   k_step    : one env.step per env from device action arrays (obs written to the obs arena)
//   k_policy  : device action driver (fair / FIFO / random / SJF / SJF-CP / weighted fair) reading the obs arena
//   k_rollout : `num_steps` x (policy -> step) fused into one launch (no host round trips); k_rollout_prio for the
//               SJF / SJF-CP kinds, k_rollout_wfair for the weighted-fair kinds
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdlib.h>

#include <mutex>
#include <stdio.h>
#include <string.h>

#include "kernels.h"
#include "decima.h"
#include "decima_policy.h"
#include "decima_rollout.h"
#include "teacher_rollout.h"
#include "units.h"

// ------------------------------------------------------------------------------------------ kernels

__global__ __launch_bounds__(64) void k_reset(const Params* __restrict__ P, uint8_t* state, uint8_t* obs,
                                              const uint8_t* __restrict__ reset) {
  const int eid = blockIdx.x;
  Sim<WaveHip> s(P, state, g_smem, obs, eid, false);
  s.reset(reset + (int64_t)eid * P->L.reset_stride);
}

// Device-sampled reset of the envs with mode != SSIM_RESET_SKIP (hot block in HBM, like k_reset).
__global__ __launch_bounds__(64) void k_reset_sampled(const Params* __restrict__ P, uint8_t* state, uint8_t* obs,
                                                      uint8_t* reset, const uint8_t* __restrict__ mode,
                                                      const uint64_t* __restrict__ seeds,
                                                      const double* __restrict__ limits) {
  const int eid = blockIdx.x;
  const int m = mode[eid];
  if (m == SSIM_RESET_SKIP) return;
  Sim<WaveHip> s(P, state, g_smem, obs, eid, false);
  s.load_header();
  s.reset_sampled(m, seeds != nullptr ? seeds[eid] : 0ull, limits != nullptr ? limits[eid] : __builtin_inf(),
                  reset + (int64_t)eid * P->L.reset_stride);
}

__global__ __launch_bounds__(64) void k_policy(const Params* __restrict__ P, const uint8_t* obs, int kind,
                                               uint64_t seed, uint64_t counter, int32_t* stage_idx,
                                               int32_t* num_exec) {
  const int eid = blockIdx.x;
  PolicyView<WaveHip> v{P->L, obs, eid};
  const StepIn a = v.act(kind, seed, counter);
  if (WaveHip::lane() == 0) {
    stage_idx[eid] = a.stage_idx;
    num_exec[eid] = a.num_exec;
  }
}

// ssim_debug_wfair: the weighted-fair weight, sum and cap of policy.h on given job works, one wave
__global__ __launch_bounds__(64) void k_debug_wfair(const double* __restrict__ Wk, int n, int alpha2, int N, double* p,
                                                    double* P, int32_t* cap) {
  double keep[kWfairKeep];
  const double tot = wfair_total<WaveHip>(n, [&](int k) { return wfair_weight(Wk[k], alpha2); }, keep);
  for (int k = WaveHip::lane(); k < n; k += 64) {
    const double pk = wfair_weight(Wk[k], alpha2);
    p[k] = pk;
    cap[k] = tot > 0.0 ? wfair_cap(N, pk, tot) : 0;
  }
  if (WaveHip::lane() == 0) *P = tot;
}

__global__ __launch_bounds__(64) void k_decima(const Params* __restrict__ P, const uint8_t* obs, float nts,
                                               float ws, float* feats, int32_t* ccap, uint32_t* emask,
                                               int32_t* depth) {
  DecimaView<WaveHip> v{P->L, obs, (int)blockIdx.x};
  v.run(nts, ws, g_smem, feats, ccap, emask, depth);
}

// The policy parameters (DecimaScheduler.parameters() order, nn.Linear layout) into the matrix cores' packed layout
// (decima_policy.h Mlp3P); one thread per packed float.
__global__ __launch_bounds__(256) void k_decima_pack(const float* __restrict__ params, float* __restrict__ packed) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= 4 * kDpPacked) return;
  const int src = dp_pack_src(f);
  packed[f] = src >= 0 ? params[src] : 0.0f;
}

// `plan` null: the plan in LDS (dynamic shared memory); else a per-env region of global memory (stride plan_stride),
// for node caps whose plan exceeds the LDS of a workgroup.
template <bool kGlobal>
__global__ __launch_bounds__(64) void k_decima_policy(const Params* __restrict__ P, const uint8_t* __restrict__ obs,
                                                      const float* __restrict__ feats, const int32_t* __restrict__ ccap,
                                                      const uint32_t* __restrict__ emask,
                                                      const int32_t* __restrict__ depth, const dp_f32x4* __restrict__ Wt,
                                                      int node_cap, uint64_t seed, uint64_t counter,
                                                      const uint8_t* __restrict__ env_mask, DecimaPolicyOut o,
                                                      int32_t* overflow, uint8_t* plan, int64_t plan_stride) {
  const int eid = blockIdx.x;
  if (env_mask != nullptr && env_mask[eid] == 0) {
    if (WaveHip::lane() == 0) {
      o.stage_idx[eid] = -1;
      o.num_exec[eid] = 1;
      o.job_idx[eid] = -1;
      o.exec_idx[eid] = 0;
      o.lgprob[eid] = 0.0f;
    }
    return;
  }
  uint8_t* lds = kGlobal ? plan + (int64_t)eid * plan_stride : g_smem;
  if (!decima_policy_env<kGlobal>(P, obs, feats, ccap, emask, depth, DpWGlobal{Wt}, node_cap, seed, counter, eid, lds,
                                  o) &&
      WaveHip::lane() == 0 && overflow != nullptr)
    atomicAdd(overflow, 1);
}

// per-job arrival/completion times and state (JobRec/JobTimes in the hot block) -> [num_envs][job_cap]
__global__ __launch_bounds__(64) void k_job_times(const Params* __restrict__ P, const uint8_t* state,
                                                  double* ta, double* tc, int32_t* st) {
  const int eid = blockIdx.x, J = P->L.job_cap;
  const uint8_t* hot = state + kParamsReserve + (int64_t)eid * P->L.env_bytes;
  const JobRec* jr = reinterpret_cast<const JobRec*>(hot + P->O.jobs);
  const JobTimes* jt = reinterpret_cast<const JobTimes*>(hot + P->O.jtimes);
  for (int j = threadIdx.x; j < J; j += 64) {
    const int64_t o = (int64_t)eid * J + j;
    if (ta) ta[o] = jt[j].tarr;
    if (tc) tc[o] = jt[j].tdone;
    if (st) st[o] = jr[j].state;
  }
}

// Per-env episode statistics (ssim_episode_stats): one wave per env, lanes stride the job records. out[eid][0] = the
// sum over arrived jobs of min(t_completed, wall) - t_arrival in ms (per-lane partial sums, then a wave tree-sum, f64),
// [1] = arrived jobs, [2] = completed jobs, [3] = the wall time.
__global__ __launch_bounds__(64) void k_episode_stats(const Params* __restrict__ P, const uint8_t* state,
                                                      double* __restrict__ out) {
  using W = WaveHip;
  const int eid = blockIdx.x, J = P->L.job_cap;
  const uint8_t* hot = state + kParamsReserve + (int64_t)eid * P->L.env_bytes;
  const double wall = W::uni(reinterpret_cast<const EnvHeader*>(hot)->wall);
  const JobRec* jr = reinterpret_cast<const JobRec*>(hot + P->O.jobs);
  const JobTimes* jt = reinterpret_cast<const JobTimes*>(hot + P->O.jtimes);
  double sum = 0.0;
  int arrived = 0, completed = 0;
  for (int j = W::lane(); j < J; j += 64) {
    const int st = jr[j].state;
    if (st != kJobPending) {
      const double td = jt[j].tdone;
      sum += (td < wall ? td : wall) - jt[j].tarr;
      ++arrived;
      completed += st == kJobDone;
    }
  }
  sum = W::sum_d(sum);
  arrived = (int)W::sum_d((double)arrived);  // (counts <= job_cap: exact)
  completed = (int)W::sum_d((double)completed);
  if (W::lane() == 0) {
    double* o = out + (int64_t)eid * 4;
    o[0] = sum;
    o[1] = (double)arrived;
    o[2] = (double)completed;
    o[3] = wall;
  }
}

// Kernel unit of a layout: units.h has the rule and the names, the tables here the kernels, one row per unit.
// Diagnostic switch: SSIM_GENERIC=1 runs the generic (run-time shape) kernels where units.h says so.
static bool generic_forced() {
  static const int on = [] {
    const char* v = getenv("SSIM_GENERIC");
    return (v != nullptr && v[0] == '1') ? 1 : 0;
  }();
  return on != 0;
}
template <class Unit>
static Unit unit_of(const Params& p, Unit (*rule)(const ssim_layout&, bool, bool)) {
  return rule(p.L, p.O.lds_resident != 0, generic_forced());
}
static const KernelSet& pick_kernels(const Params& p) {
  struct Table {
    KernelSet row[kNumEngineUnits];
    Table() {
      row[kEngBench900] = kernels_bench900(), row[kEngBench] = kernels_bench(), row[kEngLds] = kernels_lds();
      row[kEngHbm] = kernels_hbm(), row[kEngHbmN100] = kernels_hbm_n100(), row[kEngHbmN50] = kernels_hbm_n50();
      row[kEngHbmN10] = kernels_hbm_n10();
    }
  };
  static const Table t;
  return t.row[unit_of(p, engine_unit)];
}
static_assert(kDecimaHelpWaves == kDpHelpWaves, "units.h states the helper waves of dr_lds50");
static const DecimaUnitRow& pick_decima(const Params& p) {
  struct Table {
    DecimaUnitRow row[kNumDecimaUnits];
    void set(DecimaUnit u, DecimaRolloutFns k, DecimaTimedFn timed, DecimaRolloutFn greedy) {
      row[u] = DecimaUnitRow{k.rollout, k.rollout_warmup, timed, greedy, k.set_trace, decima_unit_waves(u)};
    }
    Table() {
      set(kDrHbm, decima_rollout_hbm(), decima_timed_hbm(), decima_greedy_hbm());
      set(kDrHbm50, decima_rollout_hbm50(), decima_timed_hbm50(), decima_greedy_hbm50());
      set(kDrLds, decima_rollout_lds(), decima_timed_lds(), decima_greedy_lds());
      set(kDrLds50, decima_rollout_lds50(), decima_timed_lds50(), decima_greedy_lds50());
    }
  };
  static const Table t;
  return t.row[unit_of(p, decima_unit)];
}
// The priority kinds (SJF / SJF-CP) run k_rollout_prio, which exists for the two run-time-shape engines only; the
// weighted-fair kinds k_rollout_wfair, likewise.
static bool prio_kind(int32_t kind) { return kind == SSIM_POLICY_SJF || kind == SSIM_POLICY_SJF_CP; }
static bool wfair_kind(int32_t kind) { return kind >= SSIM_POLICY_WFAIR_BASE && kind <= SSIM_POLICY_WFAIR_LAST; }
static RolloutFn pick_prio(const Params& p) {
  return unit_of(p, prio_unit) == kPrioLds ? rollout_prio_lds() : rollout_prio_hbm();
}
static RolloutFn pick_wfair(const Params& p) {
  return unit_of(p, wfair_unit) == kWfairLds ? rollout_wfair_lds() : rollout_wfair_hbm();
}
static bool known_kind(int32_t kind) {
  return kind == SSIM_POLICY_FAIR || kind == SSIM_POLICY_FIFO || kind == SSIM_POLICY_RANDOM || prio_kind(kind) ||
         wfair_kind(kind);
}

// ------------------------------------------------------------------------------------------ C ABI
struct ssim_handle {
  Params params;  // host copy (device copy at the start of the state arena)
  uint8_t* state;
  uint8_t* obs;
  uint8_t* reset;
  int ticket_slot;  // budget-launch decision counter in use next (k_rollout kFlagTicketSlot)
  uint64_t* prof_next = nullptr;  // -DSSIM_PROFILE builds: per-wave phase sums of the next Decima rollout launch
  uint8_t* policy_plan = nullptr;  // ssim_decima_policy's global plan when a node cap's plan exceeds the LDS
  int64_t policy_plan_bytes = 0;
  void* policy_packed = nullptr;   // ssim_decima_policy's packed weights (kDpPackedBytes)
};

static thread_local char g_err[512] = "";

static int set_err(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// (the weighted-fair kinds encode 2 * alpha + 4 in 0..8 above their base: a kind just past them gets the range)
static int unknown_kind(const char* who, int32_t kind) {
  if (kind > SSIM_POLICY_WFAIR_LAST && kind < SSIM_POLICY_WFAIR_BASE + 0x100)
    return set_err(SSIM_E_ARG, "%s: unknown policy %d (weighted fair is 0x%x..0x%x: alpha in [-2, 2])", who, kind,
                   SSIM_POLICY_WFAIR_BASE, SSIM_POLICY_WFAIR_LAST);
  return set_err(SSIM_E_ARG, "%s: unknown policy %d", who, kind);
}

static int hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) return set_err(SSIM_E_HIP, "%s: %s", what, hipGetErrorString(e));
  return SSIM_OK;
}

static int decima_pack(const float* params, void* packed, void* stream) {
  hipLaunchKernelGGL(k_decima_pack, dim3((4 * kDpPacked + 255) / 256), dim3(256), 0, (hipStream_t)stream, params,
                     static_cast<float*>(packed));
  return hip_check(hipGetLastError(), "k_decima_pack launch");
}

// A launch with more than 64 KB of dynamic LDS (layout.h kLdsBudgetBig) needs the kernel's opt-in attribute. It is
// per-device, per-function state: the raised limit is remembered per (device, kernel) so the attribute call is made
// once, not before every step launch. The cache is shared by every host thread that launches, so it is guarded by a
// mutex (an unguarded entry could pair one kernel with another thread's larger limit and skip a needed call).
static std::mutex g_lds_mu;
static int lds_opt_in(const void* fn, int64_t lds) {
  if (lds <= kLdsBudget) return SSIM_OK;
  struct Entry {
    int dev;
    const void* fn;
    int64_t lds;
  };
  static Entry cache[64];
  static int n_cache = 0;
  int dev = 0;
  int rc = hip_check(hipGetDevice(&dev), "hipGetDevice");
  if (rc != SSIM_OK) return rc;
  std::lock_guard<std::mutex> lk(g_lds_mu);
  for (int i = 0; i < n_cache; ++i)
    if (cache[i].dev == dev && cache[i].fn == fn && cache[i].lds >= lds) return SSIM_OK;
  rc = hip_check(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                 "engine kernel LDS attribute");
  if (rc == SSIM_OK && n_cache < 64) cache[n_cache++] = Entry{dev, fn, lds};
  return rc;
}

// Compute units of the current device (the layout's LDS-residency threshold, layout.h compute_layout); a whole MI355X
// when there is no device (host-only use of ssim_layout_for).
static int64_t device_cus() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      n <= 0) {
    (void)hipGetLastError();  // (clear the sticky error of a host without a device)
    return kChipCus;
  }
  return n;
}

extern "C" int ssim_layout_for(const ssim_config* cfg, ssim_layout* out) {
  StateOffsets O;
  if (cfg == nullptr || out == nullptr || !compute_layout(*cfg, out, &O, device_cus()))
    return set_err(SSIM_E_ARG, "ssim_layout_for: invalid config");
  return SSIM_OK;
}

extern "C" int ssim_create(const ssim_config* cfg, const ssim_dataset* dataset, void* state_arena,
                           void* obs_arena, void* reset_arena, ssim_handle** out) {
  if (cfg == nullptr || dataset == nullptr || state_arena == nullptr || obs_arena == nullptr ||
      reset_arena == nullptr || out == nullptr)
    return set_err(SSIM_E_ARG, "ssim_create: null argument");
  ssim_handle* h = new ssim_handle();
  if (!compute_layout(*cfg, &h->params.L, &h->params.O, device_cus())) {
    delete h;
    return set_err(SSIM_E_ARG, "ssim_create: invalid config");
  }
  if (h->params.O.lds_bytes > (h->params.O.lds_resident ? kLdsBudgetBig : kLdsBudget)) {
    delete h;
    return set_err(SSIM_E_ARG, "ssim_create: per-env scratch %lld B exceeds the LDS budget",
                   (long long)h->params.O.lds_bytes);
  }
  if (dataset->num_template_stages >= 32768 || dataset->num_templates >= 32768) {
    delete h;
    return set_err(SSIM_E_ARG, "ssim_create: dataset too large for int16 stage/template ids");
  }
  h->params.D = *dataset;
  h->params.C = *cfg;
  fill_hot_params(&h->params);
  h->state = static_cast<uint8_t*>(state_arena);
  h->obs = static_cast<uint8_t*>(obs_arena);
  h->reset = static_cast<uint8_t*>(reset_arena);
  {  // executor-key table for the sampler, from the dataset's executor_intervals
    const int N = cfg->num_executors;
    double* iv = new double[2 * (N + 1)];
    int rc0 = hip_check(hipMemcpy(iv, dataset->intervals, sizeof(double) * 2 * (N + 1), hipMemcpyDeviceToHost),
                        "intervals download");
    if (rc0 == SSIM_OK && !fill_interval_table(&h->params, iv, N))
      rc0 = set_err(SSIM_E_ARG, "ssim_create: executor_intervals values are not EXEC_LEVELS integers");
    delete[] iv;
    if (rc0 != SSIM_OK) {
      delete h;
      return rc0;
    }
  }
  {  // the duration-descriptor cache (engine.h) packs offset << 8 | length: usable when every list fits
    const int64_t nd = (int64_t)dataset->num_template_stages * 3 * kNumLevels;
    int32_t* dl = new int32_t[nd > 0 ? nd : 1];
    int32_t* dof = new int32_t[nd > 0 ? nd : 1];
    int rc0 = nd <= 0 ? SSIM_OK : hip_check(hipMemcpy(dl, dataset->dur_len, sizeof(int32_t) * nd, hipMemcpyDeviceToHost),
                                            "dur_len download");
    if (rc0 == SSIM_OK && nd > 0)
      rc0 = hip_check(hipMemcpy(dof, dataset->dur_off, sizeof(int32_t) * nd, hipMemcpyDeviceToHost), "dur_off download");
    bool fits = rc0 == SSIM_OK;
    for (int64_t i = 0; fits && i < nd; ++i)
      if (dl[i] > 255 || (dl[i] > 0 && (dof[i] < 0 || dof[i] >= (1 << 24)))) fits = false;
    h->params.hp.dcache = fits ? 1 : 0;
    delete[] dl;
    delete[] dof;
    if (rc0 != SSIM_OK) {
      delete h;
      return rc0;
    }
  }
  int rc = hip_check(hipMemcpy(h->state, &h->params, sizeof(Params), hipMemcpyHostToDevice), "params upload");
  if (rc == SSIM_OK)  // both budget slots start zeroed (each budget launch then zeroes the other, TicketStop)
    rc = hip_check(hipMemset(h->state + kTicketOffset, 0, (size_t)(2 * kTicketSlotBytes)), "budget slots clear");
  if (rc == SSIM_OK) rc = hip_check(hipMemset(h->obs, 0, (size_t)h->params.L.obs_bytes), "obs clear");
  if (rc == SSIM_OK)
    rc = hip_check(hipMemset(h->state + kParamsReserve, 0, (size_t)(h->params.L.state_bytes - kParamsReserve)),
                   "state clear");
  if (rc != SSIM_OK) {
    delete h;
    return rc;
  }
  *out = h;
  return SSIM_OK;
}

extern "C" int ssim_destroy(ssim_handle* h) {
  if (h != nullptr && h->policy_plan != nullptr) (void)hipFree(h->policy_plan);
  if (h != nullptr && h->policy_packed != nullptr) (void)hipFree(h->policy_packed);
  delete h;
  return SSIM_OK;
}

static const Params* dparams(const ssim_handle* h) { return reinterpret_cast<const Params*>(h->state); }

extern "C" int ssim_reset(ssim_handle* h, void* stream) {
  if (h == nullptr) return set_err(SSIM_E_ARG, "ssim_reset: null handle");
  const ssim_layout& L = h->params.L;
  hipLaunchKernelGGL(k_reset, dim3(L.num_envs), dim3(64), (size_t)L.scratch_bytes, (hipStream_t)stream,
                     dparams(h), h->state, h->obs, h->reset);
  return hip_check(hipGetLastError(), "k_reset launch");
}

extern "C" int ssim_step(ssim_handle* h, const int32_t* stage_idx, const int32_t* num_exec, void* stream) {
  if (h == nullptr || stage_idx == nullptr || num_exec == nullptr) return set_err(SSIM_E_ARG, "ssim_step: null");
  const ssim_layout& L = h->params.L;
  const StepFn fn = pick_kernels(h->params).step;
  const int rc = lds_opt_in((const void*)fn, h->params.O.lds_bytes);
  if (rc != SSIM_OK) return rc;
  hipLaunchKernelGGL(fn, dim3(L.num_envs), dim3(64), (size_t)h->params.O.lds_bytes, (hipStream_t)stream,
                     dparams(h), h->state, h->obs, stage_idx, num_exec);
  return hip_check(hipGetLastError(), "k_step launch");
}

extern "C" int ssim_policy(ssim_handle* h, int32_t kind, uint64_t seed, uint64_t counter, int32_t* stage_idx,
                           int32_t* num_exec, void* stream) {
  if (h == nullptr || stage_idx == nullptr || num_exec == nullptr) return set_err(SSIM_E_ARG, "ssim_policy: null");
  if (!known_kind(kind)) return unknown_kind("ssim_policy", kind);
  if (kind == SSIM_POLICY_SJF_CP && h->params.C.max_stages > kPrioMaxStages)
    return set_err(SSIM_E_ARG, "ssim_policy: SSIM_POLICY_SJF_CP supports at most %d stages per job (max_stages %d)",
                   kPrioMaxStages, h->params.C.max_stages);
  const ssim_layout& L = h->params.L;
  hipLaunchKernelGGL(k_policy, dim3(L.num_envs), dim3(64), 0, (hipStream_t)stream, dparams(h), h->obs, kind,
                     seed, counter, stage_idx, num_exec);
  return hip_check(hipGetLastError(), "k_policy launch");
}

// The flag checks every rollout entry shares (`who` names the entry in messages, `allowed` its flag bits).
static int check_rollout_flags(const char* who, const ssim_handle* h, int32_t flags, int32_t allowed, int64_t budget) {
  if ((flags & ~allowed) != 0) return set_err(SSIM_E_ARG, "%s: unknown flags 0x%x", who, flags);
  if ((flags & SSIM_ROLLOUT_PREEMPT) && budget <= 0)
    return set_err(SSIM_E_ARG, "%s: SSIM_ROLLOUT_PREEMPT needs a decision budget", who);
  if ((flags & SSIM_ROLLOUT_AUTORESET) && !(h->params.C.job_arrival_gap > 0.0))
    return set_err(SSIM_E_ARG, "%s: auto-reset needs job_arrival_gap in the config", who);
  return SSIM_OK;
}

// prof_out: -DSSIM_PROFILE builds' per-wave phase cycle sums, [num_envs][kNumPhases] (else null).
static int rollout_launch(ssim_handle* h, int32_t kind, uint64_t seed, int32_t num_steps, int64_t budget,
                          int32_t flags, const double* time_limits, int32_t* action_log, void* stream,
                          const int32_t* env_steps = nullptr, uint64_t* prof_out = nullptr) {
  if (h == nullptr || num_steps < 0 || budget < 0) return set_err(SSIM_E_ARG, "ssim_rollout: bad argument");
  if (!known_kind(kind)) return unknown_kind("ssim_rollout", kind);
  if (kind == SSIM_POLICY_SJF_CP && h->params.C.max_stages > kPrioMaxStages)
    return set_err(SSIM_E_ARG, "ssim_rollout: SSIM_POLICY_SJF_CP supports at most %d stages per job (max_stages %d)",
                   kPrioMaxStages, h->params.C.max_stages);
  if (flags & SSIM_ROLLOUT_GREEDY)
    return set_err(SSIM_E_ARG, "ssim_rollout_ex: SSIM_ROLLOUT_GREEDY is a flag of ssim_decima_rollout only (the "
                   "heuristic kinds have no sampled / greedy modes; flags 0x%x)", flags);
  const int rc0 = check_rollout_flags("ssim_rollout_ex", h, flags,
                                      SSIM_ROLLOUT_AUTORESET | SSIM_ROLLOUT_PREEMPT | SSIM_ROLLOUT_WARMUP, budget);
  if (rc0 != SSIM_OK) return rc0;
  const ssim_layout& L = h->params.L;
  const KernelSet& ks = pick_kernels(h->params);
  const RolloutFn fn = prio_kind(kind)    ? pick_prio(h->params)  // (one symbol: warm-up launches included)
                       : wfair_kind(kind) ? pick_wfair(h->params)  // (likewise)
                       : (flags & SSIM_ROLLOUT_WARMUP) ? ks.rollout_warmup : ks.rollout;
  const int64_t lds = h->params.O.lds_bytes;
  const int rc = lds_opt_in((const void*)fn, lds);
  if (rc != SSIM_OK) return rc;
  // the budget slot this launch claims from; flipped only once the launch is enqueued (a failed launch leaves the
  // slot it would have zeroed dirty, so the next launch must use the same one again)
  if (budget > 0 && h->ticket_slot) flags |= kFlagTicketSlot;
  hipLaunchKernelGGL(fn, dim3(L.num_envs), dim3(64),
                     (size_t)lds, (hipStream_t)stream,
                     dparams(h), h->state, h->obs, kind, seed, num_steps, flags, time_limits, h->reset, action_log,
                     prof_out, budget, env_steps);
  const int rc2 = hip_check(hipGetLastError(), "k_rollout launch");
  if (rc2 == SSIM_OK && budget > 0) h->ticket_slot ^= 1;
  return rc2;
}

extern "C" int ssim_rollout_ex(ssim_handle* h, int32_t kind, uint64_t seed, int32_t num_steps, int32_t flags,
                               const double* time_limits, int32_t* action_log, void* stream) {
  return rollout_launch(h, kind, seed, num_steps, 0, flags, time_limits, action_log, stream);
}

extern "C" int ssim_rollout_budget(ssim_handle* h, int32_t kind, uint64_t seed, int32_t max_steps,
                                   int64_t total_decisions, int32_t flags, const double* time_limits,
                                   int32_t* action_log, void* stream) {
  if (total_decisions <= 0) return set_err(SSIM_E_ARG, "ssim_rollout_budget: total_decisions must be > 0");
  return rollout_launch(h, kind, seed, max_steps, total_decisions, flags, time_limits, action_log, stream);
}

extern "C" int ssim_rollout_steps(ssim_handle* h, int32_t kind, uint64_t seed, const int32_t* env_steps,
                                  int32_t max_steps, int32_t flags, const double* time_limits, int32_t* action_log,
                                  void* stream) {
  if (env_steps == nullptr) return set_err(SSIM_E_ARG, "ssim_rollout_steps: null env_steps");
  return rollout_launch(h, kind, seed, max_steps, 0, flags, time_limits, action_log, stream, env_steps);
}

extern "C" int ssim_rollout(ssim_handle* h, int32_t kind, uint64_t seed, int32_t num_steps, int32_t* action_log,
                            void* stream) {
  return ssim_rollout_ex(h, kind, seed, num_steps, 0, nullptr, action_log, stream);
}

extern "C" int ssim_reset_sampled(ssim_handle* h, const uint8_t* mode, const uint64_t* seeds, const double* time_limits,
                                  void* stream) {
  if (h == nullptr || mode == nullptr) return set_err(SSIM_E_ARG, "ssim_reset_sampled: null argument");
  if (!(h->params.C.job_arrival_gap > 0.0))
    return set_err(SSIM_E_ARG, "ssim_reset_sampled: the config has no job_arrival_gap");
  const ssim_layout& L = h->params.L;
  hipLaunchKernelGGL(k_reset_sampled, dim3(L.num_envs), dim3(64), (size_t)L.scratch_bytes, (hipStream_t)stream,
                     dparams(h), h->state, h->obs, h->reset, mode, seeds, time_limits);
  return hip_check(hipGetLastError(), "k_reset_sampled launch");
}

#ifdef SSIM_PROFILE
// Diagnostic build only: same rollout, per-wave phase cycle sums -> prof_out[num_envs][kNumPhases].
extern "C" int ssim_rollout_profiled(ssim_handle* h, int32_t kind, uint64_t seed, int32_t num_steps,
                                     uint64_t* prof_out, void* stream) {
  return rollout_launch(h, kind, seed, num_steps, 0, 0, nullptr, nullptr, stream, nullptr, prof_out);
}
// Diagnostic build only: the budget rollout (as bench.py) with per-wave phase sums and realtime stamps.
extern "C" int ssim_rollout_budget_profiled(ssim_handle* h, int32_t kind, uint64_t seed, int32_t max_steps,
                                            int64_t total_decisions, int32_t flags, uint64_t* prof_out,
                                            const double* time_limits, void* stream) {
  if (total_decisions <= 0) return set_err(SSIM_E_ARG, "ssim_rollout_budget_profiled: total_decisions must be > 0");
  return rollout_launch(h, kind, seed, max_steps, total_decisions, flags, time_limits, nullptr, stream, nullptr,
                        prof_out);
}
// Diagnostic build only: the next ssim_decima_rollout launch on `h` writes its per-wave phase sums to prof_out.
extern "C" int ssim_decima_profile_next(ssim_handle* h, uint64_t* prof_out) {
  h->prof_next = prof_out;
  return SSIM_OK;
}
#endif

extern "C" int ssim_episode_stats(ssim_handle* h, double* out, void* stream) {
  if (h == nullptr || out == nullptr) return set_err(SSIM_E_ARG, "ssim_episode_stats: null argument");
  hipLaunchKernelGGL(k_episode_stats, dim3(h->params.L.num_envs), dim3(64), 0, (hipStream_t)stream, dparams(h),
                     h->state, out);
  return hip_check(hipGetLastError(), "k_episode_stats launch");
}

extern "C" int ssim_job_times(ssim_handle* h, double* t_arrival, double* t_completed, int32_t* state, void* stream) {
  if (h == nullptr) return set_err(SSIM_E_ARG, "ssim_job_times: null handle");
  hipLaunchKernelGGL(k_job_times, dim3(h->params.L.num_envs), dim3(64), 0, (hipStream_t)stream, dparams(h), h->state,
                     t_arrival, t_completed, state);
  return hip_check(hipGetLastError(), "k_job_times launch");
}

// The unit a launch on this handle runs, by its units.h name (null: the variant does not apply to the layout), and the
// set KAT (tests/test_gpu_sets.py) through that unit's engine instantiation (`fn` null: a name only). SSIM_DEBUG_ENGINE:
// the step / rollout kernels'; SSIM_DEBUG_DECIMA: the persistent Decima rollout's; SSIM_DEBUG_KAT_BAD: the test-only
// known-bad page assembly (N = 100 / J = 200, HBM-resident layouts).
static const char* debug_variant(const ssim_handle* h, int32_t variant, SetTraceFn* fn) {
  const Params& p = h->params;
  const DecimaUnit du = unit_of(p, decima_unit);
  *fn = nullptr;
  switch (variant) {
    case SSIM_DEBUG_ENGINE:
      *fn = pick_kernels(p).set_trace;
      return engine_unit_name(unit_of(p, engine_unit));
    case SSIM_DEBUG_DECIMA:
      *fn = pick_decima(p).set_trace;
      return decima_unit_name(du);
    case SSIM_DEBUG_DECIMA_GREEDY: return decima_unit_name(du, true);
    case SSIM_DEBUG_PRIO: return prio_unit_name(unit_of(p, prio_unit));
    case SSIM_DEBUG_WFAIR: return wfair_unit_name(unit_of(p, wfair_unit));
    case SSIM_DEBUG_TEACHER: return teacher_unit_name(unit_of(p, teacher_unit));
    case SSIM_DEBUG_KAT_BAD:
      if (!shape_n100(p.L) || p.O.lds_resident) return nullptr;
      *fn = set_trace_kat_bad();
      return kKatBadName;
  }
  return nullptr;
}

extern "C" const char* ssim_debug_kernel_name(const ssim_handle* h, int32_t variant) {
  SetTraceFn fn;
  const char* n = h != nullptr ? debug_variant(h, variant, &fn) : nullptr;
  return n != nullptr ? n : "";
}

extern "C" int ssim_debug_set_trace_ex(ssim_handle* h, const int32_t* ops, int32_t n_ops, int32_t width,
                                       int32_t* orders, int32_t variant, void* stream) {
  if (h == nullptr || ops == nullptr || orders == nullptr || n_ops < 0 || width <= 0)
    return set_err(SSIM_E_ARG, "ssim_debug_set_trace: bad argument");
  if (h->params.L.num_executors > 127 || h->params.L.job_cap < 1)
    return set_err(SSIM_E_ARG, "ssim_debug_set_trace: needs 1..127 executors and a job cap >= 1");
  SetTraceFn fn = nullptr;
  if (debug_variant(h, variant, &fn) == nullptr || fn == nullptr)
    return set_err(SSIM_E_ARG, "ssim_debug_set_trace: variant %d does not apply to this layout", variant);
  const int64_t lds = h->params.O.lds_bytes;
  const int rc = lds_opt_in((const void*)fn, lds);
  if (rc != SSIM_OK) return rc;
  hipLaunchKernelGGL(fn, dim3(1), dim3(64), (size_t)lds, (hipStream_t)stream, dparams(h), h->state, h->obs, ops, n_ops,
                     width, orders);
  return hip_check(hipGetLastError(), "k_set_trace launch");
}

extern "C" int ssim_debug_set_trace(ssim_handle* h, const int32_t* ops, int32_t n_ops, int32_t width, int32_t* orders,
                                    void* stream) {
  return ssim_debug_set_trace_ex(h, ops, n_ops, width, orders, SSIM_DEBUG_ENGINE, stream);
}

extern "C" int ssim_debug_wfair(const double* W, int32_t n, int32_t alpha2, int32_t num_executors, double* p, double* P,
                                int32_t* cap, void* stream) {
  if (W == nullptr || p == nullptr || P == nullptr || cap == nullptr || n < 1 || n > 4096 || alpha2 < -4 ||
      alpha2 > 4 || num_executors < 1)
    return set_err(SSIM_E_ARG, "ssim_debug_wfair: bad argument");
  hipLaunchKernelGGL(k_debug_wfair, dim3(1), dim3(64), 0, (hipStream_t)stream, W, n, alpha2, num_executors, p, P, cap);
  return hip_check(hipGetLastError(), "k_debug_wfair launch");
}

extern "C" int ssim_decima_features(ssim_handle* h, float num_tasks_scale, float work_scale, float* node_feats,
                                    int32_t* commit_cap, uint32_t* edge_mask, int32_t* depth, void* stream) {
  if (h == nullptr || node_feats == nullptr || commit_cap == nullptr || edge_mask == nullptr || depth == nullptr)
    return set_err(SSIM_E_ARG, "ssim_decima_features: null argument");
  const ssim_layout& L = h->params.L;
  if (h->params.C.max_stages > kDecimaMaxDepth)
    return set_err(SSIM_E_ARG, "ssim_decima_features: max_stages %d > %d (edge-mask word)", h->params.C.max_stages,
                   kDecimaMaxDepth);
  const int64_t lds = decima_scratch_bytes(L.stage_cap);
  if (lds > kLdsBudget) return set_err(SSIM_E_ARG, "ssim_decima_features: stage_cap %d too large", L.stage_cap);
  hipLaunchKernelGGL(k_decima, dim3(L.num_envs), dim3(64), (size_t)lds, (hipStream_t)stream, dparams(h), h->obs,
                     num_tasks_scale, work_scale, node_feats, commit_cap, edge_mask, depth);
  return hip_check(hipGetLastError(), "k_decima launch");
}

extern "C" int ssim_decima_policy(ssim_handle* h, const float* node_feats, const int32_t* commit_cap,
                                  const uint32_t* edge_mask, const int32_t* depth, const float* params,
                                  int32_t num_params, int32_t node_cap, uint64_t seed, uint64_t counter,
                                  const uint8_t* env_mask, int32_t* stage_idx, int32_t* num_exec, int32_t* job_idx,
                                  int32_t* exec_idx, float* lgprob, float* stage_scores, float* exec_scores,
                                  int32_t* overflow, void* stream) {
  if (h == nullptr || node_feats == nullptr || commit_cap == nullptr || edge_mask == nullptr || depth == nullptr ||
      params == nullptr || stage_idx == nullptr || num_exec == nullptr || job_idx == nullptr ||
      exec_idx == nullptr || lgprob == nullptr)
    return set_err(SSIM_E_ARG, "ssim_decima_policy: null argument");
  if (num_params != kDecimaParams)
    return set_err(SSIM_E_ARG, "ssim_decima_policy: %d parameters, the fused kernel implements the "
                   "decima_tpch.yaml architecture (%d)", num_params, kDecimaParams);
  const ssim_layout& L = h->params.L;
  if (L.num_executors > 64 * kDpExecChunks)
    return set_err(SSIM_E_ARG, "ssim_decima_policy: more than %d executors", 64 * kDpExecChunks);
  if (node_cap <= 0 || node_cap > L.stage_cap) node_cap = L.stage_cap;
  if (node_cap < (L.num_executors + kDpEmb - 1) / kDpEmb) node_cap = (L.num_executors + kDpEmb - 1) / kDpEmb;
  const int64_t lds = decima_policy_lds_bytes(node_cap, L.job_cap);
  DecimaPolicyOut o{stage_idx, num_exec, job_idx, exec_idx, lgprob, stage_scores, exec_scores};
  if (h->policy_packed == nullptr) {
    const int rc = hip_check(hipMalloc(&h->policy_packed, (size_t)kDpPackedBytes), "packed weights allocation");
    if (rc != SSIM_OK) return rc;
  }
  {
    const int rc = decima_pack(params, h->policy_packed, stream);
    if (rc != SSIM_OK) return rc;
  }
  const dp_f32x4* wpk = static_cast<const dp_f32x4*>(h->policy_packed);
  if (lds > kDecimaPolicyLdsMax) {  // the plan in a handle-owned global region (grown on demand)
    const int64_t stride = (lds + 255) & ~int64_t(255), need = stride * L.num_envs;
    if (need > h->policy_plan_bytes) {
      if (h->policy_plan != nullptr) {
        int rc = hip_check(hipStreamSynchronize((hipStream_t)stream), "policy plan resize sync");
        if (rc != SSIM_OK) return rc;
        (void)hipFree(h->policy_plan);
        h->policy_plan = nullptr;
        h->policy_plan_bytes = 0;
      }
      int rc = hip_check(hipMalloc(&h->policy_plan, (size_t)need), "policy plan allocation");
      if (rc != SSIM_OK) return rc;
      h->policy_plan_bytes = need;
    }
    hipLaunchKernelGGL(k_decima_policy<true>, dim3(L.num_envs), dim3(64), 0, (hipStream_t)stream, dparams(h), h->obs,
                       node_feats, commit_cap, edge_mask, depth, wpk, node_cap, seed, counter, env_mask, o, overflow,
                       h->policy_plan, stride);
    return hip_check(hipGetLastError(), "k_decima_policy(global plan) launch");
  }
  {
    const int rc = lds_opt_in((const void*)k_decima_policy<false>, lds);
    if (rc != SSIM_OK) return rc;
  }
  hipLaunchKernelGGL(k_decima_policy<false>, dim3(L.num_envs), dim3(64), (size_t)lds, (hipStream_t)stream,
                     dparams(h), h->obs, node_feats, commit_cap, edge_mask, depth, wpk, node_cap, seed, counter,
                     env_mask, o, overflow, (uint8_t*)nullptr, (int64_t)0);
  return hip_check(hipGetLastError(), "k_decima_policy launch");
}

// The persistent Decima rollout's LDS plan (decima_rollout.h): the policy's per-node rows for observations of up to
// `cap` nodes in the wave's LDS, after the engine's own LDS (`off` relative to the scratch block), within the env's
// share of its CU (StateOffsets::lds_share: the share compute_layout's residency decision assumed, so the plan never
// lowers the workgroups per CU the layout counted on).
struct DecimaLdsPlan {
  int32_t cap, off;
  int64_t lds;       // dynamic LDS of the launch
  int32_t help_off;  // the exec-score helpers' mailbox (units with helper waves), after the rest
  int threads;       // block size: 64 per wave of the unit
};
static DecimaLdsPlan decima_lds_plan(const Params& P, int waves) {
  const StateOffsets& O = P.O;
  const ssim_layout& L = P.L;
  DecimaLdsPlan pl{0, 0, O.lds_bytes, 0, 64 * waves};
  const int64_t help = waves > 1 ? dp_help_bytes(L.num_executors) : 0;
  const int64_t eng = O.lds_resident ? O.hot_bytes + O.scratch_bytes : O.scratch_hbm_bytes;  // (HBM: row map cold)
  // Engines without the duration-descriptor cache hold only per-operation temporaries in their LDS scratch (set
  // tables, key lists, the commitment plan, observe()'s stage -> row map), none live across a decision: the plan
  // overlays them. (Round 6: LDS-resident engines too — the PPO collect's J = 200 / N = 50 envs keep a 146 KB hot block
  // in a CU's 160 KB, and overlaying their 10.8 KB scratch takes the plan from ~8 to ~60 nodes, so nearly every
  // decision's policy runs from LDS instead of the global plan.)
#ifdef SSIM_PROFILE
  const bool overlay = false;  // (the profile sums live in the scratch)
#else
  const bool overlay = L.num_executors > kDurCacheMaxExecs;
#endif
  // (past the LDS copy of the executor records, sc_execs, when the HBM-resident engine keeps one for the launch)
  const int64_t off = overlay ? (!O.lds_resident && SSIM_DR_EX_LDS ? O.sc_keys_a : 0)
                              : align16(O.lds_resident ? O.scratch_bytes : O.scratch_hbm_bytes);
  const int64_t base = O.lds_resident ? O.hot_bytes : 0;  // (the plan offset is relative to the scratch block)
  const int64_t room = O.lds_share - base - off - help;
  int cap = 0;
  while (cap < L.stage_cap && decima_policy_lds_bytes(cap + 1, kDpLdsDags) <= room &&
         decima_scratch_bytes(cap + 1) <= room)
    ++cap;
  // The one-wave exec-score loop keeps escore[k], k < N, in the plan's agg rows (cap x 16 floats, decima_policy.h), the
  // reason ssim_decima_policy raises its node_cap to ceil(N / 16). A smaller LDS plan cannot hold them (a stage cap
  // below ceil(N / 16), or the little room an -DSSIM_PROFILE / SSIM_DR_EX_LDS build leaves next to many executors'
  // scratch): every decision then takes the global plan, which ssim_decima_rollout checks the same way.
  if (cap < (L.num_executors + kDpEmb - 1) / kDpEmb) cap = 0;
  pl.cap = cap;
  pl.off = (int32_t)off;
  if (cap > 0) {
    const int64_t need = base + off + decima_policy_lds_bytes(cap, kDpLdsDags);
    pl.lds = need > align16(eng) ? need : align16(eng);
  }
  if (help > 0) {
    pl.help_off = (int32_t)align16(pl.lds);
    pl.lds = pl.help_off + help;
  }
  return pl;
}

// The launch shape of kernel `fn` of the unit row `k`, so that kernel, plan and block size are all of one row: the
// row's LDS plan, into `a` too when given, and the opt-in for its dynamic LDS (a null `fn` only computes: no device call).
static int decima_launch_plan(const ssim_handle* h, const DecimaUnitRow& k, const void* fn, DecimaRolloutArgs* a,
                              DecimaLdsPlan* pl) {
  *pl = decima_lds_plan(h->params, k.waves);
  if (a != nullptr) a->plan_cap = pl->cap, a->plan_off = pl->off, a->help_off = pl->help_off;
  return fn != nullptr ? lds_opt_in(fn, pl->lds) : SSIM_OK;
}

extern "C" int64_t ssim_decima_rollout_lds_bytes(const ssim_handle* h) {
  if (h == nullptr) return set_err(SSIM_E_ARG, "ssim_decima_rollout_lds_bytes: null handle");
  DecimaLdsPlan pl;
  (void)decima_launch_plan(h, pick_decima(h->params), nullptr, nullptr, &pl);
  return pl.lds;
}

// Test hook (host only, no launch): the node cap of the LDS plan and the waves per workgroup of the unit that
// ssim_decima_rollout runs for this handle, so a test can say which plan a recorded decision took.
extern "C" int ssim_debug_decima_plan(const ssim_handle* h, int32_t* cap, int32_t* waves) {
  if (h == nullptr || cap == nullptr || waves == nullptr)
    return set_err(SSIM_E_ARG, "ssim_debug_decima_plan: null argument");
  DecimaLdsPlan pl;
  (void)decima_launch_plan(h, pick_decima(h->params), nullptr, nullptr, &pl);
  *cap = pl.cap;
  *waves = pl.threads / 64;
  return SSIM_OK;
}

extern "C" int64_t ssim_decima_workspace_bytes(const ssim_handle* h) {
  if (h == nullptr) return set_err(SSIM_E_ARG, "ssim_decima_workspace_bytes: null handle");
  return decima_work(h->params.L).total;
}

// Argument checks the Decima and teacher rollout entries share (`who` names the entry in messages).
static int check_sample_arena(const char* who, const ssim_decima_samples& sm) {
  if (sm.cursor == nullptr || sm.rec == nullptr || sm.nodes == nullptr || sm.edges == nullptr || sm.dags == nullptr ||
      sm.cap_samples <= 0 || sm.cap_nodes < 0 || sm.cap_edges < 0 || sm.cap_dags < 0)
    return set_err(SSIM_E_ARG, "%s: incomplete sample arena", who);
  return SSIM_OK;
}
static int check_decima_workspace(const char* who, const DecimaWork& wl, int64_t workspace_bytes) {
  if (workspace_bytes < wl.total)
    return set_err(SSIM_E_ARG, "%s: workspace of %lld B, needs %lld (ssim_decima_workspace_bytes)", who,
                   (long long)workspace_bytes, (long long)wl.total);
  return SSIM_OK;
}
static int check_edge_mask_depth(const char* who, const ssim_handle* h) {
  if (h->params.C.max_stages > kDecimaMaxDepth)
    return set_err(SSIM_E_ARG, "%s: max_stages %d > %d (edge-mask word)", who, h->params.C.max_stages,
                   kDecimaMaxDepth);
  return SSIM_OK;
}

// The checks and launch arguments ssim_decima_rollout and ssim_decima_rollout_timed share (`who` names the entry in
// messages): the policy weights packed on `stream`, the workspace layout, the sample arena.
static int decima_rollout_args(const char* who, ssim_handle* h, const float* params, int32_t num_params,
                               float num_tasks_scale, float work_scale, uint64_t seed, uint64_t counter,
                               void* workspace, int64_t workspace_bytes, const ssim_decima_samples* samples,
                               void* stream, DecimaRolloutArgs* out) {
  if (num_params != kDecimaParams)
    return set_err(SSIM_E_ARG, "%s: %d parameters, the fused kernel implements the "
                   "decima_tpch.yaml architecture (%d)", who, num_params, kDecimaParams);
  const ssim_layout& L = h->params.L;
  if (const int rc = check_edge_mask_depth(who, h); rc != SSIM_OK) return rc;
  if (L.num_executors > 64 * kDpExecChunks)
    return set_err(SSIM_E_ARG, "%s: more than %d executors", who, 64 * kDpExecChunks);
  // (the global plan's agg rows, stage_cap x 16 floats, hold the N exec scores too: decima_lds_plan)
  if (L.stage_cap < (L.num_executors + kDpEmb - 1) / kDpEmb)
    return set_err(SSIM_E_ARG, "%s: stage cap %d below ceil(%d executors / %d): the policy plan "
                   "cannot hold the exec scores", who, L.stage_cap, L.num_executors, kDpEmb);
  const DecimaWork wl = decima_work(L);
  if (const int rc = check_decima_workspace(who, wl, workspace_bytes); rc != SSIM_OK) return rc;
  DecimaRolloutArgs a{};
  if (samples != nullptr) {
    if (const int rc = check_sample_arena(who, *samples); rc != SSIM_OK) return rc;
    a.smp = *samples;
  }
  a.weights = reinterpret_cast<const dp_f32x4*>(static_cast<uint8_t*>(workspace) + wl.packed);
  a.work = static_cast<uint8_t*>(workspace);
  {
    const int rc = decima_pack(params, static_cast<uint8_t*>(workspace) + wl.packed, stream);
    if (rc != SSIM_OK) return rc;
  }
  a.wl = wl;
  a.num_tasks_scale = num_tasks_scale;
  a.work_scale = work_scale;
  a.seed = seed;
  a.counter = counter;
  *out = a;
  return SSIM_OK;
}

extern "C" int ssim_decima_rollout(ssim_handle* h, const float* params, int32_t num_params, float num_tasks_scale,
                                   float work_scale, uint64_t seed, uint64_t counter, int32_t max_steps,
                                   int64_t total_decisions, int32_t flags, const double* time_limits, void* workspace,
                                   int64_t workspace_bytes, const ssim_decima_samples* samples, int32_t* action_log,
                                   void* stream) {
  if (h == nullptr || params == nullptr || workspace == nullptr || max_steps < 0 || total_decisions < 0)
    return set_err(SSIM_E_ARG, "ssim_decima_rollout: bad argument");
  const bool greedy = (flags & SSIM_ROLLOUT_GREEDY) != 0;
  if (greedy &&
      (flags & (SSIM_ROLLOUT_AUTORESET | SSIM_ROLLOUT_PREEMPT | SSIM_ROLLOUT_WARMUP | SSIM_ROLLOUT_TEST_REJECT)) != 0)
    return set_err(SSIM_E_ARG, "ssim_decima_rollout: SSIM_ROLLOUT_GREEDY does not combine with SSIM_ROLLOUT_AUTORESET / "
                   "PREEMPT / WARMUP / TEST_REJECT (flags 0x%x)", flags);
  const int rc0 = check_rollout_flags("ssim_decima_rollout", h, flags,
                                      SSIM_ROLLOUT_AUTORESET | SSIM_ROLLOUT_PREEMPT | SSIM_ROLLOUT_WARMUP |
                                          SSIM_ROLLOUT_TEST_REJECT | SSIM_ROLLOUT_GREEDY,
                                      total_decisions);
  if (rc0 != SSIM_OK) return rc0;
  DecimaRolloutArgs a{};
  {
    const int rc = decima_rollout_args("ssim_decima_rollout", h, params, num_params, num_tasks_scale, work_scale, seed,
                                       counter, workspace, workspace_bytes, samples, stream, &a);
    if (rc != SSIM_OK) return rc;
  }
  const ssim_layout& L = h->params.L;
  const DecimaUnitRow& ks = pick_decima(h->params);
  const DecimaRolloutFn fn = greedy ? ks.greedy : (flags & SSIM_ROLLOUT_WARMUP) ? ks.rollout_warmup : ks.rollout;
  flags &= ~SSIM_ROLLOUT_GREEDY;  // (the kernel never sees the flag's bit)
  DecimaLdsPlan ln;
  const int rc = decima_launch_plan(h, ks, (const void*)fn, &a, &ln);
  if (rc != SSIM_OK) return rc;
  if (total_decisions > 0 && h->ticket_slot) flags |= kFlagTicketSlot;
  hipLaunchKernelGGL(fn, dim3(L.num_envs), dim3(ln.threads), (size_t)ln.lds, (hipStream_t)stream, dparams(h),
                     h->state, h->obs, a, max_steps, flags, time_limits, h->reset, action_log, total_decisions,
                     h->prof_next);
  h->prof_next = nullptr;
  const int rc2 = hip_check(hipGetLastError(), "k_decima_rollout launch");
  if (rc2 == SSIM_OK && total_decisions > 0) h->ticket_slot ^= 1;
  return rc2;
}

extern "C" int ssim_decima_rollout_timed(ssim_handle* h, const float* params, int32_t num_params,
                                         float num_tasks_scale, float work_scale, uint64_t seed, uint64_t counter,
                                         int32_t max_steps, int64_t total_decisions, int32_t flags,
                                         const double* time_limits, void* workspace, int64_t workspace_bytes,
                                         const ssim_decima_samples* samples, const ssim_decima_timed* timed,
                                         int32_t* action_log, void* stream) {
  if (h == nullptr || params == nullptr || workspace == nullptr || max_steps < 0)
    return set_err(SSIM_E_ARG, "ssim_decima_rollout_timed: bad argument");
  if (flags & SSIM_ROLLOUT_GREEDY)
    return set_err(SSIM_E_ARG, "ssim_decima_rollout_timed: SSIM_ROLLOUT_GREEDY is a flag of ssim_decima_rollout only "
                   "(fixed-duration collection samples; flags 0x%x)", flags);
  if ((flags & (SSIM_ROLLOUT_AUTORESET | SSIM_ROLLOUT_PREEMPT | SSIM_ROLLOUT_WARMUP)) != 0 || total_decisions != 0 ||
      time_limits != nullptr)
    return set_err(SSIM_E_ARG, "ssim_decima_rollout_timed: does not combine with SSIM_ROLLOUT_AUTORESET / PREEMPT / "
                   "WARMUP, a decision budget or time_limits (flags 0x%x)", flags);
  if ((flags & ~SSIM_ROLLOUT_TEST_REJECT) != 0)
    return set_err(SSIM_E_ARG, "ssim_decima_rollout_timed: unknown flags 0x%x", flags);
  if (samples == nullptr) return set_err(SSIM_E_ARG, "ssim_decima_rollout_timed: needs a sample arena");
  if (timed == nullptr) return set_err(SSIM_E_ARG, "ssim_decima_rollout_timed: null timed argument");
  const ssim_decima_timed& t = *timed;
  if (t.cap_resets <= 0) return set_err(SSIM_E_ARG, "ssim_decima_rollout_timed: cap_resets %d <= 0", t.cap_resets);
  if (t.clock == nullptr || t.seeds == nullptr || t.limits == nullptr || t.sched == nullptr ||
      t.reset_steps == nullptr || t.ep_arrival == nullptr || t.ep_completed == nullptr || t.ep_state == nullptr)
    return set_err(SSIM_E_ARG, "ssim_decima_rollout_timed: incomplete timed argument (null array)");
  if (!(t.duration >= 0.0)) return set_err(SSIM_E_ARG, "ssim_decima_rollout_timed: duration must be >= 0");
  if (!(h->params.C.job_arrival_gap > 0.0))
    return set_err(SSIM_E_ARG, "ssim_decima_rollout_timed: in-place resets need job_arrival_gap in the config");
  DecimaRolloutArgs a{};
  {
    const int rc = decima_rollout_args("ssim_decima_rollout_timed", h, params, num_params, num_tasks_scale, work_scale,
                                       seed, counter, workspace, workspace_bytes, samples, stream, &a);
    if (rc != SSIM_OK) return rc;
  }
  const DecimaUnitRow& ks = pick_decima(h->params);
  const DecimaTimedFn fn = ks.timed;
  DecimaLdsPlan ln;
  const int rc = decima_launch_plan(h, ks, (const void*)fn, &a, &ln);
  if (rc != SSIM_OK) return rc;
  hipLaunchKernelGGL(fn, dim3(h->params.L.num_envs), dim3(ln.threads), (size_t)ln.lds, (hipStream_t)stream,
                     dparams(h), h->state, h->obs, a, t, max_steps, flags, h->reset, action_log, h->prof_next);
  h->prof_next = nullptr;
  return hip_check(hipGetLastError(), "k_decima_rollout_timed launch");
}

// The teacher rollout's LDS plan (teacher_rollout.h): the Decima rollout's plan of a one-wave unit (decima_lds_plan: the
// same engine configuration, so what the plan overlays or follows is the same, and the same share of the CU), of which
// the teacher uses the features' scratch only. A decision takes the LDS under the rule of decima_rollout.h
// DecimaPolicy::act (at most `cap` nodes and kDpLdsDags DAGs), so a teacher collection runs the features where a Decima
// collection of the same observations runs them, and both placements occur at small shapes.
static DecimaLdsPlan teacher_lds_plan(const Params& P) { return decima_lds_plan(P, 1); }
static TeacherRolloutFn pick_teacher(const Params& p) {
  return unit_of(p, teacher_unit) == kTrLds ? teacher_rollout_lds() : teacher_rollout_hbm();
}

extern "C" int ssim_debug_teacher_plan(const ssim_handle* h, int32_t* cap, int32_t* dags) {
  if (h == nullptr || cap == nullptr || dags == nullptr)
    return set_err(SSIM_E_ARG, "ssim_debug_teacher_plan: null argument");
  *cap = teacher_lds_plan(h->params).cap;
  *dags = kDpLdsDags;
  return SSIM_OK;
}

extern "C" int ssim_teacher_rollout(ssim_handle* h, int32_t kind, uint64_t seed, float num_tasks_scale,
                                    float work_scale, int32_t max_steps, int32_t flags, void* workspace,
                                    int64_t workspace_bytes, const ssim_decima_samples* samples, int32_t* action_log,
                                    void* stream) {
  if (h == nullptr || workspace == nullptr || max_steps < 0)
    return set_err(SSIM_E_ARG, "ssim_teacher_rollout: bad argument");
  if (!known_kind(kind)) return unknown_kind("ssim_rollout", kind);
  if (kind == SSIM_POLICY_SJF_CP && h->params.C.max_stages > kPrioMaxStages)
    return set_err(SSIM_E_ARG, "ssim_teacher_rollout: SSIM_POLICY_SJF_CP supports at most %d stages per job "
                   "(max_stages %d)", kPrioMaxStages, h->params.C.max_stages);
  if (flags != 0)
    return set_err(SSIM_E_ARG, "ssim_teacher_rollout: collection mode only, flags must be 0 (no SSIM_ROLLOUT_AUTORESET / "
                   "PREEMPT / WARMUP / GREEDY; flags 0x%x)", flags);
  if (const int rc = check_edge_mask_depth("ssim_teacher_rollout", h); rc != SSIM_OK) return rc;
  if (samples == nullptr) return set_err(SSIM_E_ARG, "ssim_teacher_rollout: needs a sample arena");
  if (const int rc = check_sample_arena("ssim_teacher_rollout", *samples); rc != SSIM_OK) return rc;
  const ssim_layout& L = h->params.L;
  const DecimaWork wl = decima_work(L);
  if (const int rc = check_decima_workspace("ssim_teacher_rollout", wl, workspace_bytes); rc != SSIM_OK) return rc;
  uint8_t* const work = static_cast<uint8_t*>(workspace);
  const DecimaLdsPlan pl = teacher_lds_plan(h->params);
  TeacherArgs a{};
  a.work = work + wl.feat_scratch;
  a.stride = wl.stride;
  static_cast<DecimaFeatArrays&>(a) = wl.arrays(work);
  a.num_tasks_scale = num_tasks_scale;
  a.work_scale = work_scale;
  a.kind = kind;
  a.seed = seed;
  a.plan_cap = pl.cap;
  a.plan_off = pl.off;
  a.plan_dags = kDpLdsDags;
  a.smp = *samples;
  const TeacherRolloutFn fn = pick_teacher(h->params);
  const int rc = lds_opt_in((const void*)fn, pl.lds);
  if (rc != SSIM_OK) return rc;
  hipLaunchKernelGGL(fn, dim3(L.num_envs), dim3(64), (size_t)pl.lds, (hipStream_t)stream, dparams(h), h->state, h->obs,
                     a, max_steps, h->reset, action_log);
  return hip_check(hipGetLastError(), "k_teacher_rollout launch");
}

extern "C" const char* ssim_last_error(void) { return g_err; }

#ifndef SSIM_BUILD_ID
#define SSIM_BUILD_ID "unversioned"
#endif
extern "C" const char* ssim_build_id(void) { return SSIM_BUILD_ID; }
