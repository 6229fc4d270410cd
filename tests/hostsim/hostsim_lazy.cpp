// hostsim_lazy.cpp — TEST-ONLY host build of the fused rollouts' decision loop (rollout.h rollout_loop) on the lazy
// engine (engine.h Sim kLazyObs): the loop and the observation split the device's k_rollout / k_rollout_prio run,
// with a one-lane wave and no budget. hostsim.cpp's own rollout steps an eager engine and checks the obs-arena
// policy view before every step, which a lazy engine's arena cannot serve between two decisions of a launch.
// Shares hostsim.cpp's handle and wave type (one shared object: lazy_driver.py).
#include "hostsim.cpp"

extern "C" {

// ssim_rollout_steps of a heuristic or priority kind as kernels.h rollout_body runs it without a budget: env e takes
// min(env_steps[e], num_steps) decisions (all num_steps when env_steps is null).
int hs_rollout_lazy(hs_handle* h, int kind, uint64_t seed, const int32_t* env_steps, int num_steps, int flags,
                    const double* limits, int32_t* action_log) {
  using SimT = Sim<WaveSerial, 0, 0, 0, true>;
  const Params* P = h->params;
  const int B = P->L.num_envs;
  const bool autoreset = (flags & SSIM_ROLLOUT_AUTORESET) != 0;
  for (int e = 0; e < B; ++e) {
    int steps = num_steps;
    if (env_steps != nullptr) {
      steps = env_steps[e] < num_steps ? env_steps[e] : num_steps;
      if (steps <= 0) continue;
    }
    if (!autoreset && action_log == nullptr) {  // (rollout_body's env_idle)
      const EnvHeader* gh = reinterpret_cast<const EnvHeader*>(h->state + kParamsReserve +
                                                               (int64_t)e * P->L.env_bytes + P->O.hdr);
      if (gh->terminated || (gh->err & SSIM_ERR_STICKY) || gh->num_jobs == 0) continue;
    }
    SimT s(P, h->state, h->resident ? resident_lds(h) : h->scratch, h->obs, e, h->resident != 0, false,
           /*ex_lds=*/h->resident == 0);
    const double limit = limits != nullptr ? limits[e] : __builtin_inf();
    uint8_t* rec = h->reset + (int64_t)e * P->L.reset_stride;
    const auto reset_in_place = [&](SimT& x) { x.reset_sampled(SSIM_RESET_CONTINUE, 0ull, limit, rec); };
    RolloutCursor c{0, 0, 0};
    const NoBudget stop;
    s.load_hot();
    if (policy_is_prio(kind))
      rollout_loop(s, PrioPolicy{kind}, stop, c, B, e, steps, autoreset, action_log, reset_in_place);
    else
      rollout_loop(s, HeuristicPolicy{kind, seed}, stop, c, B, e, steps, autoreset, action_log, reset_in_place);
    s.save_hot();
  }
  return 0;
}

}  // extern "C"
