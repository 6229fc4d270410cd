// units.h — which kernel unit (k_*.hip) a launch on a layout runs, and the units' names. Host code without HIP: the
// C ABI (sparksched.hip) indexes its kernel tables by these enums, and the host test build (tests/hostsim) checks the
// rule's truth table without a device.
#pragma once
#include "sparksched.h"

namespace ssim {

enum EngineUnit : int { kEngBench900, kEngBench, kEngLds, kEngHbm, kEngHbmN100, kEngHbmN50, kEngHbmN10, kNumEngineUnits };
enum DecimaUnit : int { kDrHbm, kDrHbm50, kDrLds, kDrLds50, kNumDecimaUnits };  // k_dr_* with their k_drt_* / k_drg_*
enum PrioUnit : int { kPrioLds, kPrioHbm, kNumPrioUnits };
enum WfairUnit : int { kWfairLds, kWfairHbm, kNumWfairUnits };
enum TeacherUnit : int { kTrLds, kTrHbm, kNumTeacherUnits };  // k_tr_*: the teacher rollout (teacher_rollout.h)

// The shapes with kernels of their own: BASELINE configs[1] (10 executors, 50 jobs), decima_tpch.yaml (50, 200), the
// configs[3] shard (100, 200).
inline bool shape_n10(const ssim_layout& L) { return L.num_executors == 10 && L.job_cap == 50; }
inline bool shape_n50(const ssim_layout& L) { return L.num_executors == 50 && L.job_cap == 200; }
inline bool shape_n100(const ssim_layout& L) { return L.num_executors == 100 && L.job_cap == 200; }

// THE RULE. `generic` is the diagnostic switch SSIM_GENERIC=1 (read by sparksched.hip). It sends every HBM-resident
// layout, engine and Decima, to the run-time-shape units, and an LDS-resident Decima layout from dr_lds50 to dr_lds;
// the LDS-resident engine units ignore it (their shape units stay).
// Engine: LDS-resident layouts specialise on the benchmark shape, fully (stage cap too) when the packed dataset's cap
// is the synthetic set's 50 x 18 = 900, else on (executors, jobs) with the stage cap read at run time (any other
// TPC-H-format dataset); HBM-resident ones on (executors, jobs).
inline EngineUnit engine_unit(const ssim_layout& L, bool lds_resident, bool generic) {
  if (lds_resident) return !shape_n10(L) ? kEngLds : L.stage_cap == 900 ? kEngBench900 : kEngBench;
  if (generic) return kEngHbm;
  return shape_n100(L) ? kEngHbmN100 : shape_n50(L) ? kEngHbmN50 : shape_n10(L) ? kEngHbmN10 : kEngHbm;
}
inline DecimaUnit decima_unit(const ssim_layout& L, bool lds_resident, bool generic) {
  const bool n50 = shape_n50(L) && !generic;
  return lds_resident ? (n50 ? kDrLds50 : kDrLds) : (n50 ? kDrHbm50 : kDrHbm);
}
// The priority kinds (SJF / SJF-CP) have run-time-shape kernels only, one per residency.
inline PrioUnit prio_unit(const ssim_layout&, bool lds_resident, bool) { return lds_resident ? kPrioLds : kPrioHbm; }
// The weighted-fair kinds likewise, in units of their own (k_wfair_*.hip).
inline WfairUnit wfair_unit(const ssim_layout&, bool lds_resident, bool) { return lds_resident ? kWfairLds : kWfairHbm; }
// The teacher rollout (every policy kind in one kernel) likewise (k_tr_*.hip).
inline TeacherUnit teacher_unit(const ssim_layout&, bool lds_resident, bool) { return lds_resident ? kTrLds : kTrHbm; }

// Waves per env's workgroup of a Decima unit: dr_lds50 has the exec-score helper waves (decima_policy.h kDpHelpWaves,
// which sparksched.hip asserts equal to this).
constexpr int kDecimaHelpWaves = 4;
inline int decima_unit_waves(DecimaUnit u) { return u == kDrLds50 ? kDecimaHelpWaves : 1; }

// Unit names (ssim_debug_kernel_name): the translation unit without its "k_" and ".hip".
inline const char* engine_unit_name(EngineUnit u) {
  static const char* const names[kNumEngineUnits] = {"bench900", "bench", "lds", "hbm", "hbm_n100", "hbm_n50", "hbm_n10"};
  return names[u];
}
inline const char* decima_unit_name(DecimaUnit u, bool greedy = false) {
  static const char* const names[2][kNumDecimaUnits] = {{"dr_hbm", "dr_hbm50", "dr_lds", "dr_lds50"},
                                                        {"drg_hbm", "drg_hbm50", "drg_lds", "drg_lds50"}};
  return names[greedy ? 1 : 0][u];
}
inline const char* prio_unit_name(PrioUnit u) { return u == kPrioLds ? "prio_lds" : "prio_hbm"; }
inline const char* wfair_unit_name(WfairUnit u) { return u == kWfairLds ? "wfair_lds" : "wfair_hbm"; }
inline const char* teacher_unit_name(TeacherUnit u) { return u == kTrLds ? "tr_lds" : "tr_hbm"; }
constexpr const char* kKatBadName = "kat_bad_page";  // the test-only known-bad page assembly (k_hbm_n100.hip)

}  // namespace ssim
