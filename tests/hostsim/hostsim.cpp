// hostsim.cpp — TEST-ONLY host build of the device engine (gym-sparksched_amd/csrc/engine.h, policy.h).
//
// Not part of the product: the product is the gfx950 library (sparksched.hip) and nothing in the
// product loads this file's output. It instantiates the same Sim<W>/PolicyView<W> templates with a
// one-lane wave (W::kWidth = 1) so the simulation logic can be checked against the CPU oracle, with host
// sanitizers, in a container that has no GPU. Device parity is checked separately by the `-m gpu` tests.
#define __device__
#define __host__
#define __forceinline__ inline
#define __constant__
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <stdint.h>

// Diagnostic variant (-DSSIM_POOL_STATS, scripts/pool_stats.py): per CPython-set operation kind (add, remove,
// idle order) a histogram over table sizes (log2) and the sum of the keys held.
#ifdef SSIM_POOL_STATS
static int64_t g_pool_ops[3][16], g_pool_keys[3][16];
static inline void pool_stat(int op, int size, int used) {
  int b = 0;
  while ((1 << (b + 1)) <= size && b < 15) ++b;
  g_pool_ops[op][b]++;
  g_pool_keys[op][b] += used;
}
#define SSIM_POOL_STAT(op, size, used) pool_stat(op, size, used)
#endif
// Diagnostic variant (-DSSIM_FIELD_STATS, scripts/field_stats.py): wave-uniform hot-block reads by section (engine.h
// SSIM_FIELD_STAT).
#ifdef SSIM_FIELD_STATS
static int64_t g_field[16];
#define SSIM_FIELD_STAT(sec) \
  do {                       \
    if ((sec) >= 0) g_field[(sec)]++; \
  } while (0)
#endif

#include "decima.h"
#include "engine.h"
#include "policy.h"
#include "rollout.h"
#include "units.h"

using namespace ssim;

struct WaveSerial {
  static constexpr int kWidth = 1;
  static int lane() { return 0; }
  static uint64_t ballot(bool p) { return p ? 1u : 0u; }
  static int ffs(uint64_t m) { return m ? __builtin_ctzll(m) : -1; }
  static int popc(uint64_t m) { return __builtin_popcountll(m); }
  static int rank(uint64_t) { return 0; }
  template <class T>
  static T uni(T v) {
    return v;
  }
  static int bcast_i(int v, int) { return v; }
  static int writelane(int v, int, int) { return v; }
  static int compact(uint64_t, int v) { return v; }
  static void sync() {}
  static void drain() {}
  static void gsync() {}
  static uint64_t clock() { return 0; }
  static uint64_t realtime() { return 0; }
  static void lds_add_u64(uint64_t* p, uint64_t v) { *p += v; }
  static int excl_scan(int x, int* total) {
    *total = x;
    return 0;
  }
  static double sum_d(double x) { return x; }
  static float fdiv(float a, float b) { return a / b; }
  static float fmul(float a, float b) { return a * b; }
  static int lds_load(const int* p) { return *p; }
  static void amax(int* p, int v) { *p = v > *p ? v : *p; }
  static void amin(int* p, int v) { *p = v < *p ? v : *p; }
  static void aor(uint32_t* p, uint32_t v) { *p |= v; }
  static int max_i(int x) { return x; }
  static int min_i(int x) { return x; }
  static void min_pair(int&, int&) {}
  template <int kSpan>
  static int argmin_event(double t, int, bool valid, double* tmin) {
    *tmin = valid ? t : __builtin_inf();
    return valid ? 0 : -1;
  }
};

struct hs_handle {
  Params* params;
  uint8_t* state;
  uint8_t* obs;
  uint8_t* reset;
  uint8_t* scratch;
  uint8_t* lds;   // emulated LDS residency: [hot copy | scratch] (hs_set_resident)
  int resident;
};

// LDS-residency emulation (hs_set_resident): step and rollout calls run on a working copy of the hot block made by
// the engine's own load_hot / save_hot, with the copy pre-filled with a poison byte, so a read of a record outside
// the live range the copy covers (or a write the save drops) shows up as a parity failure on the CPU.
static constexpr uint8_t kPoison = 0xA5;
static uint8_t* resident_lds(hs_handle* h) {
  const Params* P = h->params;
  const int64_t n = P->O.hot_bytes + P->L.scratch_bytes;
  if (h->lds == nullptr) h->lds = (uint8_t*)malloc((size_t)n);
  memset(h->lds, kPoison, (size_t)n);
  return h->lds;
}

extern "C" {

int hs_create(const ssim_config* cfg, const ssim_dataset* ds, hs_handle** out, ssim_layout* layout_out) {
  hs_handle* h = (hs_handle*)calloc(1, sizeof(hs_handle));
  Params p;
  memset(&p, 0, sizeof(p));
  if (!compute_layout(*cfg, &p.L, &p.O)) {
    free(h);
    return -1;
  }
  p.D = *ds;
  p.C = *cfg;
  fill_hot_params(&p);
  if (!fill_interval_table(&p, ds->intervals, cfg->num_executors)) {
    free(h);
    return -2;
  }
  h->state = (uint8_t*)calloc(1, (size_t)p.L.state_bytes);
  h->obs = (uint8_t*)calloc(1, (size_t)p.L.obs_bytes);
  h->reset = (uint8_t*)calloc(1, (size_t)p.L.reset_bytes);
  h->scratch = (uint8_t*)calloc(1, (size_t)p.L.scratch_bytes);
  memcpy(h->state, &p, sizeof(Params));
  h->params = (Params*)h->state;
  *layout_out = p.L;
  *out = h;
  return 0;
}

void hs_destroy(hs_handle* h) {
  free(h->state);
  free(h->obs);
  free(h->reset);
  free(h->scratch);
  free(h->lds);
  free(h);
}

void hs_set_resident(hs_handle* h, int on) { h->resident = on; }

uint8_t* hs_obs(hs_handle* h) { return h->obs; }
uint8_t* hs_reset_arena(hs_handle* h) { return h->reset; }
uint8_t* hs_state(hs_handle* h) { return h->state; }

int hs_reset(hs_handle* h) {
  const Params* P = h->params;
  for (int e = 0; e < P->L.num_envs; ++e) {
    Sim<WaveSerial> s(P, h->state, h->scratch, h->obs, e, false);
    s.reset(h->reset + (int64_t)e * P->L.reset_stride);
  }
  return 0;
}

int hs_step(hs_handle* h, const int32_t* stage_idx, const int32_t* num_exec) {
  const Params* P = h->params;
  for (int e = 0; e < P->L.num_envs; ++e) {
    Sim<WaveSerial> s(P, h->state, h->resident ? resident_lds(h) : h->scratch, h->obs, e, h->resident != 0, false,
                      /*ex_lds=*/h->resident == 0);  // (the device's HBM-resident launches: executor records in LDS)
    StepIn a;
    a.stage_idx = stage_idx[e];
    a.num_exec = num_exec[e];
    s.load_hot();  // (k_step's sequence; no-ops without residency)
    s.step(a);
    s.save_hot();
  }
  return 0;
}

int hs_policy(hs_handle* h, int kind, uint64_t seed, uint64_t counter, int32_t* stage_idx, int32_t* num_exec) {
  const Params* P = h->params;
  for (int e = 0; e < P->L.num_envs; ++e) {
    PolicyView<WaveSerial> v{P->L, h->obs, e};
    const StepIn a = v.act(kind, seed, counter);
    stage_idx[e] = a.stage_idx;
    num_exec[e] = a.num_exec;
  }
  return 0;
}

int hs_reset_sampled(hs_handle* h, const uint8_t* mode, const uint64_t* seeds, const double* limits) {
  const Params* P = h->params;
  for (int e = 0; e < P->L.num_envs; ++e) {
    if (mode[e] == SSIM_RESET_SKIP) continue;
    Sim<WaveSerial> s(P, h->state, h->scratch, h->obs, e, false);
    s.load_header();
    s.reset_sampled(mode[e], seeds ? seeds[e] : 0ull, limits ? limits[e] : __builtin_inf(),
                    h->reset + (int64_t)e * P->L.reset_stride);
  }
  return 0;
}

int hs_rollout_ex(hs_handle* h, int kind, uint64_t seed, int num_steps, int flags, const double* limits,
                  int32_t* action_log);
int hs_rollout(hs_handle* h, int kind, uint64_t seed, int num_steps, int32_t* action_log) {
  return hs_rollout_ex(h, kind, seed, num_steps, 0, nullptr, action_log);
}

int hs_rollout_steps(hs_handle* h, int kind, uint64_t seed, const int32_t* env_steps, int num_steps, int flags,
                     const double* limits, int32_t* action_log);
int hs_rollout_ex(hs_handle* h, int kind, uint64_t seed, int num_steps, int flags, const double* limits,
                  int32_t* action_log) {
  return hs_rollout_steps(h, kind, seed, nullptr, num_steps, flags, limits, action_log);
}

// ssim_rollout_steps: env e takes min(env_steps[e], num_steps) decisions (all num_steps when env_steps is null)
int hs_rollout_steps(hs_handle* h, int kind, uint64_t seed, const int32_t* env_steps, int num_steps, int flags,
                     const double* limits, int32_t* action_log) {
  const Params* P = h->params;
  const int B = P->L.num_envs;
  for (int e = 0; e < B; ++e) {
    Sim<WaveSerial> s(P, h->state, h->resident ? resident_lds(h) : h->scratch, h->obs, e, h->resident != 0, false,
                      /*ex_lds=*/h->resident == 0);  // (the device's HBM-resident launches: executor records in LDS)
    PolicyView<WaveSerial> v{P->L, h->obs, e};
    const int steps = env_steps != nullptr && env_steps[e] < num_steps ? env_steps[e] : num_steps;
    s.load_hot();
    for (int k = 0; k < steps; ++k) {
      // the device rollout's policy (picks from the hot block) must equal the obs-arena view's (k_policy)
      s.load_header();
      const StepIn a = sim_policy(s, kind, seed);
      const StepIn b = v.act(kind, seed, (uint64_t)s.h.decisions + ((uint64_t)s.h.episode << 32));
      if (!s.idle() && (a.stage_idx != b.stage_idx || a.num_exec != b.num_exec)) return -5;
      if (action_log) {
        action_log[((int64_t)k * B + e) * 2 + 0] = a.stage_idx;
        action_log[((int64_t)k * B + e) * 2 + 1] = a.num_exec;
      }
      s.step_loaded(a);
      if ((flags & SSIM_ROLLOUT_AUTORESET) && s.h.num_jobs > 0 && !s.frozen() &&
          (s.h.terminated || s.h.wall >= s.h.time_limit))
        s.reset_sampled(SSIM_RESET_CONTINUE, 0ull, limits ? limits[e] : __builtin_inf(),
                        h->reset + (int64_t)e * P->L.reset_stride);
    }
    s.save_hot();
  }
  return 0;
}

void hs_job_times(hs_handle* h, double* ta, double* tc, int32_t* st) {
  const Params* P = h->params;
  const int J = P->L.job_cap;
  for (int e = 0; e < P->L.num_envs; ++e) {
    const uint8_t* hot = h->state + kParamsReserve + (int64_t)e * P->L.env_bytes;
    const JobRec* jr = reinterpret_cast<const JobRec*>(hot + P->O.jobs);
    const JobTimes* jt = reinterpret_cast<const JobTimes*>(hot + P->O.jtimes);
    for (int j = 0; j < J; ++j) {
      ta[(int64_t)e * J + j] = jt[j].tarr;
      tc[(int64_t)e * J + j] = jt[j].tdone;
      st[(int64_t)e * J + j] = jr[j].state;
    }
  }
}

// Decima featurisation of the current obs (decima.h), all envs; outputs as ssim_decima_features.
int hs_decima(hs_handle* h, float nts, float ws, float* feats, int32_t* ccap, uint32_t* emask, int32_t* depth) {
  const Params* P = h->params;
  uint8_t* scratch = (uint8_t*)calloc(1, (size_t)decima_scratch_bytes(P->L.stage_cap));
  for (int e = 0; e < P->L.num_envs; ++e) {
    DecimaView<WaveSerial> v{P->L, h->obs, e};
    v.run(nts, ws, scratch, feats, ccap, emask, depth);
  }
  free(scratch);
  return 0;
}

// Per env: live stage window (live_hi - scan_live_lo), active stages, active jobs, arrived jobs.
void hs_live_stats(hs_handle* h, int32_t* out) {
  const Params* P = h->params;
  for (int e = 0; e < P->L.num_envs; ++e) {
    Sim<WaveSerial> s(P, h->state, h->scratch, h->obs, e, false);
    s.load_header();
    out[4 * e + 0] = s.live_hi() - s.scan_live_lo();
    out[4 * e + 1] = s.h.n_active_stages;
    out[4 * e + 2] = s.h.n_active_jobs;
    out[4 * e + 3] = s.h.arrivals;
  }
}

#ifdef SSIM_POOL_STATS
void hs_pool_stats(int64_t* out) {  // [3][16] op counts then [3][16] key sums; resets the counters
  memcpy(out, g_pool_ops, sizeof(g_pool_ops));
  memcpy(out + 48, g_pool_keys, sizeof(g_pool_keys));
  memset(g_pool_ops, 0, sizeof(g_pool_ops));
  memset(g_pool_keys, 0, sizeof(g_pool_keys));
}
#endif

#ifdef SSIM_FIELD_STATS
void hs_field_stats(int64_t* out) {  // [16] read counts by section; resets the counters
  memcpy(out, g_field, sizeof(g_field));
  memset(g_field, 0, sizeof(g_field));
}
#endif

// PCG64 / CPython-set models exposed for the known-answer tests.
void hs_pcg_run(uint64_t* words, const int32_t* ops, int n_ops, double* out) {
  Pcg64 r;
  r.s_hi = words[0];
  r.s_lo = words[1];
  r.i_hi = words[2];
  r.i_lo = words[3];
  r.has32 = (uint32_t)words[4];
  r.u32 = (uint32_t)words[5];
  for (int k = 0; k < n_ops; ++k) {
    const int op = ops[k];
    out[k] = op == 0 ? r.random() : (double)r.bounded((uint32_t)op);
  }
  words[0] = r.s_hi;
  words[1] = r.s_lo;
  words[2] = r.i_hi;
  words[3] = r.i_lo;
  words[4] = r.has32;
  words[5] = r.u32;
}

// Seeded PCG64 (SeedSequence) words, then `n` standard exponentials; log1p on given inputs.
void hs_seed_words(uint64_t seed, uint64_t* words) {
  const Pcg64 r = Pcg64::from_seed(seed);
  words[0] = r.s_hi;
  words[1] = r.s_lo;
  words[2] = r.i_hi;
  words[3] = r.i_lo;
}
void hs_std_exponential(uint64_t* words, int n, double* out) {
  Pcg64 r;
  r.s_hi = words[0];
  r.s_lo = words[1];
  r.i_hi = words[2];
  r.i_lo = words[3];
  r.has32 = (uint32_t)words[4];
  r.u32 = (uint32_t)words[5];
  for (int k = 0; k < n; ++k) out[k] = r.std_exponential();
  words[0] = r.s_hi;
  words[1] = r.s_lo;
  words[4] = r.has32;
  words[5] = r.u32;
}
void hs_log1p(const double* x, int n, double* out) {
  for (int k = 0; k < n; ++k) out[k] = fd_log1p(x[k]);
}

// Runs a trace of set operations; after each op writes the iteration order into `orders`
// (row of `width` int32, -1 padded). ops: (code, key) pairs; code 0 add, 1 remove, 2 copy,
// 3 "set(filtered)" with keys whose bit in `key` (bitmask over key%31) is set, 4 pop.
int hs_pyset_trace(const int32_t* ops, int n_ops, int width, int32_t* orders) {
  PySetMeta m;
  uint8_t* tab = (uint8_t*)malloc(4096);
  uint8_t* tab2 = (uint8_t*)malloc(4096);
  int32_t keys[1024], tmp[1024];
  ps_init(&m, tab);
  uint32_t finger = 0;
  for (int k = 0; k < n_ops; ++k) {
    const int code = ops[2 * k], key = ops[2 * k + 1];
    if (code == 0) {
      ps_add<WaveSerial>(&m, tab, (uint32_t)key, tmp);
    } else if (code == 1) {
      if (!ps_remove<WaveSerial>(&m, tab, (uint32_t)key)) return -1;
    } else if (code == 2) {  // s = s.copy()
      int n = ps_keys<WaveSerial>(&m, tab, keys);
      memcpy(tab2, tab, (size_t)m.mask + 1);
      PySetMeta src = m;
      ps_copy_order<WaveSerial>(&src, keys, n, tab2);
      // materialise the copy as the current set (ps_copy_order left the copy's table in tab2 unless
      // it was a slot-for-slot copy of the source table)
      uint32_t size = 8;
      if (n * 5 >= 21)
        while ((int)size <= n * 2) size <<= 1;
      if (n > 0 && !((size - 1) == src.mask && src.fill == src.used)) {
        memcpy(tab, tab2, size);
        m.mask = (uint16_t)(size - 1);
      } else if (n == 0) {
        ps_init(&m, tab);
      }
      m.fill = m.used = (uint16_t)n;
      finger = 0;
    } else if (code == 3) {  // s = set(x for x in s if mask bit)
      int n = ps_keys<WaveSerial>(&m, tab, keys);
      int c = 0;
      for (int i = 0; i < n; ++i)
        if ((key >> (keys[i] % 31)) & 1) keys[c++] = keys[i];
      ps_init(&m, tab);
      for (int i = 0; i < c; ++i) ps_add<WaveSerial>(&m, tab, (uint32_t)keys[i], tmp);
      finger = 0;
    } else if (code == 4) {  // pop
      if (m.used == 0) return -2;
      uint32_t i = finger & m.mask;
      while (tab[i] >= kSlotDummy) i = (i + 1) & m.mask;
      tab[i] = kSlotDummy;
      m.used--;
      finger = i + 1;
    }
    int n = ps_keys<WaveSerial>(&m, tab, keys);
    if (n > width) return -3;
    for (int i = 0; i < width; ++i) orders[(int64_t)k * width + i] = i < n ? keys[i] : -1;
  }
  free(tab);
  free(tab2);
  return 0;
}

// The C ABI's kernel-unit rule (units.h): the unit names and the Decima unit's waves per workgroup for a layout.
void hs_unit_names(const ssim_layout* L, int lds_resident, int generic, const char** engine, const char** decima,
                   const char** greedy, const char** prio, int* waves) {
  const bool res = lds_resident != 0, gen = generic != 0;
  const DecimaUnit d = decima_unit(*L, res, gen);
  *engine = engine_unit_name(engine_unit(*L, res, gen));
  *decima = decima_unit_name(d);
  *greedy = decima_unit_name(d, true);
  *prio = prio_unit_name(prio_unit(*L, res, gen));
  *waves = decima_unit_waves(d);
}

}  // extern "C"
