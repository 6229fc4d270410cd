// policy.h — on-device action drivers that read the observation arena, one wavefront per env.
//
//   FAIR / FIFO : RoundRobinScheduler.schedule (schedulers/heuristics/round_robin.py:14-49) with
//                 find_stage / preprocess_obs (schedulers/heuristics/utils.py:5-37): prefer the source
//                 job with all committable executors, else the first job (arrival order) under the cap.
//   RANDOM      : uniform choice among jobs that have a schedulable stage (the distribution produced by
//                 random_scheduler.py:16-32's rejection loop), find_stage, num_exec ~ U{1..committable};
//                 the stream is a counter-based splitmix64 of (seed, env, counter), so a run is exactly
//                 reproducible; parity tests record these actions and replay them on the CPU oracle.
//   SJF / SJF-CP: shortest job first (prio_job): the job with a schedulable stage and the least remaining work
//                 W(k) = sum over its rows of float64(remaining tasks) * float64(most recent duration), added in row
//                 order; ties to the earlier job. SJF takes that job's find_stage and all committable executors;
//                 SJF-CP takes its schedulable row with the longest critical path cp(r) = w(r) + max(0, max cp(child))
//                 (prio_cp_stage; ties to the lowest row). Their own driver (prio_act / sim_policy_prio) and their own
//                 rollout kernel (kernels.h k_rollout_prio): policy_act is inlined into every tuned k_rollout
//                 instantiation and stays as it is. DESIGN.md "Priority schedulers".
//   WFair(alpha): weighted fair (wfair_act), kinds SSIM_POLICY_WFAIR_BASE + (2 alpha + 4): fair's rule with a per-job
//                 cap min(N, ceil(N * W(k)^alpha / sum of W^alpha)), alpha a half-integer in [-2, 2]. Its own
//                 driver and rollout kernel (rollout.h WfairPolicy, kernels.h k_rollout_wfair), so k_rollout_prio is
//                 compiled from the code it had without these kinds. DESIGN.md "Weighted-fair schedulers".
#pragma once
#include <stdint.h>

#include "engine.h"

namespace ssim {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ULL;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
  return x ^ (x >> 31);
}

// uniform integer in [0, n) from 32 random bits (n >= 1)
__device__ __forceinline__ int uniform_below(uint64_t bits, int n) {
  return (int)(((bits & 0xFFFFFFFFULL) * (uint64_t)n) >> 32);
}

// The decision rule of the device policies over a per-active-job view (nj active jobs, index k in arrival
// order): pick(k) = find_stage of job k (-1 = none), supply(k) = its exec supply; comm = committable
// executors, src = source_job_idx. Shared by the obs-arena view (k_policy) and the fused rollout, which
// passes the picks its observation pass computed (Sim::observe) so both give the same action.
template <class W, class Pick, class Supply>
__device__ __forceinline__ StepIn policy_act(int kind, uint64_t seed, uint64_t counter, int eid, int N, int nj,
                                             int comm, int src, Pick pick, Supply supply) {
  StepIn a;
  a.stage_idx = -1;
  a.num_exec = comm > 0 ? comm : 1;
  if (kind == SSIM_POLICY_FAIR || kind == SSIM_POLICY_FIFO) {
    const int cap = kind == SSIM_POLICY_FAIR ? (N + (nj > 1 ? nj : 1) - 1) / (nj > 1 ? nj : 1) : N;
    if (src < nj) {
      const int s = W::uni(pick(src));
      if (s >= 0) {
        a.stage_idx = s;
        return a;
      }
    }
    for (int k0 = 0; k0 < nj; k0 += W::kWidth) {
      const int k = k0 + W::lane();
      const bool ok = k < nj && k != src && supply(k) < cap;
      const int s = ok ? pick(k) : -1;
      const uint64_t m = W::ballot(s >= 0);
      if (m) {
        const int l = W::ffs(m);
        a.stage_idx = W::bcast_i(s, l);
        const int room = cap - W::bcast_i(ok ? supply(k) : 0, l);
        a.num_exec = comm < room ? comm : room;
        return a;
      }
    }
    return a;
  }
  // RANDOM
  const uint64_t key = splitmix64(seed ^ splitmix64((uint64_t)eid * 0xD1B54A32D192ED03ULL + counter));
  if (nj <= W::kWidth) {  // one chunk: each lane keeps its job's pick
    const int k = W::lane();
    const int s = k < nj ? pick(k) : -1;
    const uint64_t m = W::ballot(s >= 0);
    const int valid = W::popc(m);
    if (valid > 0) {
      const int r = uniform_below(splitmix64(key ^ 0x1ULL), valid);
      const int l = W::ffs(W::ballot(s >= 0 && W::rank(m) == r));
      a.stage_idx = W::bcast_i(s, l);
    }
  } else {
    int valid = 0;
    for (int k0 = 0; k0 < nj; k0 += W::kWidth) {
      const int k = k0 + W::lane();
      valid += W::popc(W::ballot(k < nj && pick(k) >= 0));
    }
    if (valid > 0) {
      int r = uniform_below(splitmix64(key ^ 0x1ULL), valid);
      for (int k0 = 0; k0 < nj; k0 += W::kWidth) {
        const int k = k0 + W::lane();
        const int s = k < nj ? pick(k) : -1;
        const uint64_t m = W::ballot(s >= 0);
        const int cnt = W::popc(m);
        if (r < cnt) {
          const int l = W::ffs(W::ballot(s >= 0 && W::rank(m) == r));
          a.stage_idx = W::bcast_i(s, l);
          break;
        }
        r -= cnt;
      }
    }
  }
  a.num_exec = comm > 0 ? 1 + uniform_below(splitmix64(key ^ 0x2ULL), comm) : 1;
  return a;
}

// ---------------------------------------------------------------------------------- SJF / SJF-CP (priority kinds)
// The kinds that are not policy_act's: SJF / SJF-CP and weighted fair (prio_act takes all of them; on the device the
// rollouts of weighted fair have their own driver, in the one-lane host build PrioPolicy drives them too).
__device__ __forceinline__ bool policy_is_prio(int kind) {
  return kind == SSIM_POLICY_SJF || kind == SSIM_POLICY_SJF_CP ||
         (kind >= SSIM_POLICY_WFAIR_BASE && kind <= SSIM_POLICY_WFAIR_LAST);
}
constexpr int kPrioMaxStages = 64;  // SJF-CP: one lane (one bit of a child set) per row of the chosen job

// k* of the priority kinds: the active job with a pick (pick(k) >= 0) and the smallest (work(k), k); -1 if no job
// has a pick. One lane per job, 64 jobs per round; work(k) >= 0 (a sum of products of non-negative floats), which
// is what the bit-pattern minimum of WaveHip::min_d needs. Wave-uniform result.
template <class W, class Work, class Pick>
__device__ __forceinline__ int prio_job(int nj, Work work, Pick pick) {
  double bw = __builtin_inf();
  int bk = -1;
  for (int k0 = 0; k0 < nj; k0 += W::kWidth) {
    const int k = k0 + W::lane();
    const bool c = k < nj && pick(k) >= 0;
    const double w = c ? work(k) : __builtin_inf();
    if constexpr (W::kWidth == 64) {
      const double m = W::template min_d<64>(w);
      const uint64_t eq = W::ballot(c && w == m);
      if (eq != 0 && (bk < 0 || m < bw)) {  // (strict: a tie stays with the earlier round's job)
        bw = m;
        bk = k0 + W::ffs(eq);
      }
    } else {
      if (c && (bk < 0 || w < bw)) {
        bw = w;
        bk = k;
      }
    }
  }
  return bk;
}

// The SJF-CP stage of the chosen job: its n <= 64 rows one per lane; row(l, &w, &kids, &rank) gives row l's work,
// the set of its children's row numbers (bit c = an edge l -> c) and its rank among the env's schedulable rows
// (-1: not schedulable; a lane that stands for no row of the observation reports w = 0, no children, rank -1 and is
// in no other row's child set). cp(l) = w(l) + max(0, max over children cp(c)): rounds of relaxation from cp = w
// until no lane changes (at most the DAG's depth + 1; capped at n + 1 so a corrupt edge list cannot spin). Returns the
// rank of the schedulable row with the largest cp (lowest row on ties), -1 if none. Wave-uniform control flow.
template <class W, class Row>
__device__ __forceinline__ int prio_cp_stage(int n, Row row) {
  if constexpr (W::kWidth == 64) {
    const int l = W::lane();
    double w = 0.0;
    uint64_t kids = 0;
    int rank = -1;
    if (l < n) row(l, &w, &kids, &rank);
    uint64_t all = 0;  // every row that is some row's child
    for (uint64_t m = W::ballot(kids != 0); m != 0; m &= m - 1) {
      const int b = W::ffs(m);
      all |= (uint64_t)(uint32_t)W::bcast_i((int)(uint32_t)kids, b) |
             ((uint64_t)(uint32_t)W::bcast_i((int)(uint32_t)(kids >> 32), b) << 32);
    }
    double cp = w;
    for (int round = 0; round <= n; ++round) {
      double best = 0.0;
      for (uint64_t m = all; m != 0; m &= m - 1) {
        const int b = W::ffs(m);
        const double v = W::bcast_d(cp, b);
        if (((kids >> b) & 1ull) != 0 && v > best) best = v;
      }
      const double next = w + best;
      const bool moved = next != cp;
      cp = next;
      if (W::ballot(moved) == 0) break;
    }
    uint64_t m = W::ballot(rank >= 0);
    if (m == 0) return -1;
    int at = W::ffs(m);
    double top = W::bcast_d(cp, at);
    for (m &= m - 1; m != 0; m &= m - 1) {
      const int b = W::ffs(m);
      const double v = W::bcast_d(cp, b);
      if (v > top) {
        top = v;
        at = b;
      }
    }
    return W::bcast_i(rank, at);
  } else {
    double w[kPrioMaxStages], cp[kPrioMaxStages];
    uint64_t kids[kPrioMaxStages];
    int rank[kPrioMaxStages];
    for (int l = 0; l < n; ++l) {
      w[l] = 0.0;
      kids[l] = 0;
      rank[l] = -1;
      row(l, &w[l], &kids[l], &rank[l]);
      cp[l] = w[l];
    }
    for (int round = 0; round <= n; ++round) {
      bool moved = false;
      for (int l = 0; l < n; ++l) {
        double best = 0.0;
        for (uint64_t m = kids[l]; m != 0; m &= m - 1) {
          const double v = cp[__builtin_ctzll(m)];
          if (v > best) best = v;
        }
        const double next = w[l] + best;
        moved = moved || next != cp[l];
        cp[l] = next;
      }
      if (!moved) break;
    }
    int at = -1;
    for (int l = 0; l < n; ++l)
      if (rank[l] >= 0 && (at < 0 || cp[l] > cp[at])) at = l;
    return at < 0 ? -1 : rank[at];
  }
}

// ------------------------------------------------------------------------------------- weighted fair (WFair(alpha))
// The kinds SSIM_POLICY_WFAIR_BASE + (alpha2 + 4), alpha2 = 2 * alpha in -4..4 (include/sparksched.h has the rule; the
// host scheduler WeightedFairScheduler is its specification). Every written operation below is one correctly rounded
// float64 operation and none may be fused with a neighbour (a * b + c contracted to an fma rounds once, not twice), so
// the functions that hold them switch contraction off.
#if defined(__clang__)
#define SSIM_FP_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SSIM_FP_NO_CONTRACT  // (the host build compiles with -ffp-contract=off)
#endif
__device__ __forceinline__ bool policy_is_wfair(int kind) {
  return kind >= SSIM_POLICY_WFAIR_BASE && kind <= SSIM_POLICY_WFAIR_LAST;
}
__device__ __forceinline__ int wfair_alpha2(int kind) { return kind - SSIM_POLICY_WFAIR_BASE - 4; }
constexpr int kWfairKeep = 4;  // blocks of 64 jobs whose weights stay in registers between the two passes

// p = W^(alpha2 / 2) from multiplies, one square root and one divide; a job without work weighs 1 under alpha2 = 0
// (every job does), else 0. alpha2 is wave-uniform.
__device__ __forceinline__ double wfair_weight(double w, int alpha2) {
  SSIM_FP_NO_CONTRACT
  if (!(w > 0.0)) return alpha2 == 0 ? 1.0 : 0.0;
  const int a = alpha2 < 0 ? -alpha2 : alpha2;
  double h = 1.0;
  if (a == 1)
    h = __builtin_sqrt(w);
  else if (a == 2)
    h = w;
  else if (a == 3)
    h = w * __builtin_sqrt(w);
  else if (a == 4)
    h = w * w;
  return alpha2 < 0 ? 1.0 / h : h;
}

// The sum of one block of 64 weights, folding halves: x[:32] + x[32:], then 16, 8, 4, 2, 1. On a wave that is the
// xor-32 .. xor-1 butterfly (WaveHip::sum_d's association); the one-lane build folds a local array.
template <class W>
__device__ __forceinline__ double wfair_block_sum(double x) {
  SSIM_FP_NO_CONTRACT
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = x + W::shfl_xor_d(x, off);
  return W::uni(x);
}
__device__ __forceinline__ double wfair_fold64(double* x) {
  SSIM_FP_NO_CONTRACT
  for (int half = 32; half > 0; half >>= 1)
    for (int i = 0; i < half; ++i) x[i] = x[i] + x[i + half];
  return x[0];
}

// P: the block sums of weight(k), k < nj, added left to right from 0.0. keep[b] receives this lane's weight of block
// b < kWfairKeep (0.0 past nj) for the second pass.
template <class W, class Weight>
__device__ __forceinline__ double wfair_total(int nj, Weight weight, double (&keep)[kWfairKeep]) {
  SSIM_FP_NO_CONTRACT
  double P = 0.0;
  if constexpr (W::kWidth == 64) {
    const int l = W::lane();
#pragma unroll
    for (int b = 0; b < kWfairKeep; ++b) {
      keep[b] = 0.0;
      if (b * 64 < nj) {
        if (b * 64 + l < nj) keep[b] = weight(b * 64 + l);
        P = P + wfair_block_sum<W>(keep[b]);
      }
    }
    for (int k0 = kWfairKeep * 64; k0 < nj; k0 += 64) {
      double x = 0.0;
      if (k0 + l < nj) x = weight(k0 + l);
      P = P + wfair_block_sum<W>(x);
    }
  } else {
    for (int b = 0; b < kWfairKeep; ++b) keep[b] = 0.0;
    for (int k0 = 0; k0 < nj; k0 += 64) {
      double x[64];
      for (int i = 0; i < 64; ++i) x[i] = k0 + i < nj ? weight(k0 + i) : 0.0;
      P = P + wfair_fold64(x);
    }
  }
  return P;
}

// cap = min(N, ceil((N * p) / P)), P > 0
__device__ __forceinline__ int wfair_cap(int N, double p, double P) {
  SSIM_FP_NO_CONTRACT
  const double c = __builtin_ceil(((double)N * p) / P);
  return c < (double)N ? (int)c : N;
}

// The rule over a per-active-job view (policy_act's, plus work(k) = W(k), prio_job's): the source job keeps every
// committable executor if it has a pick; else one lane per job, 64 jobs per round, each lane forms its job's weight, a
// butterfly per block gives P, and a second pass over the blocks finds the first job other than the source under its
// cap with a pick (ballot, ffs) and broadcasts its pick and room. Wave-uniform control flow around every cross-lane
// operation; the weights of the first kWfairKeep blocks are not computed twice.
template <class W, class Work, class Pick, class Supply>
__device__ __forceinline__ StepIn wfair_act(int alpha2, int N, int nj, int comm, int src, Work work, Pick pick,
                                            Supply supply) {
  StepIn a;
  a.stage_idx = -1;
  a.num_exec = comm > 0 ? comm : 1;
  if (src < nj) {
    const int s = W::uni(pick(src));
    if (s >= 0) {
      a.stage_idx = s;
      return a;
    }
  }
  const auto weight = [&](int k) { return wfair_weight(work(k), alpha2); };
  double keep[kWfairKeep];
  const double P = wfair_total<W>(nj, weight, keep);
  if (!(P > 0.0)) return a;
  if constexpr (W::kWidth == 64) {
    const int l = W::lane();
    const auto block = [&](int k0, double p) {
      const int k = k0 + l;
      int cap = 0, sup = 0, s = -1;
      if (k < nj && k != src) {
        cap = wfair_cap(N, p, P);
        sup = supply(k);
        if (sup < cap) s = pick(k);
      }
      const uint64_t m = W::ballot(s >= 0);
      if (m == 0) return false;
      const int at = W::ffs(m);
      a.stage_idx = W::bcast_i(s, at);
      const int room = W::bcast_i(cap - sup, at);
      a.num_exec = comm < room ? comm : room;
      return true;
    };
#pragma unroll
    for (int b = 0; b < kWfairKeep; ++b) {
      if (b * 64 >= nj) return a;
      if (block(b * 64, keep[b])) return a;
    }
    for (int k0 = kWfairKeep * 64; k0 < nj; k0 += 64) {
      double p = 0.0;
      if (k0 + l < nj) p = weight(k0 + l);
      if (block(k0, p)) return a;
    }
  } else {
    for (int k = 0; k < nj; ++k) {
      if (k == src) continue;
      const int cap = wfair_cap(N, weight(k), P), sup = supply(k);
      if (sup >= cap) continue;
      const int s = pick(k);
      if (s >= 0) {
        a.stage_idx = s;
        a.num_exec = comm < cap - sup ? comm : cap - sup;
        return a;
      }
    }
  }
  return a;
}

template <class W>
struct PolicyView {
  const ssim_layout& L;
  const uint8_t* obs;
  int eid;

  __device__ __forceinline__ const int32_t* counts() const {
    return reinterpret_cast<const int32_t*>(obs + L.ob_counts) + (int64_t)eid * SSIM_NUM_COUNTS;
  }
  __device__ __forceinline__ const int32_t* ptr() const {
    return reinterpret_cast<const int32_t*>(obs + L.ob_dag_ptr) + (int64_t)eid * (L.job_cap + 1);
  }
  __device__ __forceinline__ const int32_t* sup() const {
    return reinterpret_cast<const int32_t*>(obs + L.ob_supplies) + (int64_t)eid * L.job_cap;
  }
  __device__ __forceinline__ const int32_t* srank() const {
    return reinterpret_cast<const int32_t*>(obs + L.ob_sched_rank) + (int64_t)eid * L.stage_cap;
  }
  __device__ __forceinline__ const uint8_t* front() const { return obs + L.ob_frontier + (int64_t)eid * L.stage_cap; }

  // find_stage (utils.py:17-37) for active job index k; -1 if none
  __device__ __forceinline__ int find_stage(int k) const {
    const int32_t* p = ptr();
    const int32_t* r = srank();
    const uint8_t* f = front();
    int fallback = -1;
    for (int node = p[k]; node < p[k + 1]; ++node) {
      const int i = r[node];
      if (i < 0) continue;
      if (f[node]) return i;
      if (fallback < 0) fallback = i;
    }
    return fallback;
  }

  __device__ __forceinline__ const float* nodes() const {
    return reinterpret_cast<const float*>(obs + L.ob_nodes) + (int64_t)eid * L.stage_cap * 3;
  }
  __device__ __forceinline__ const int64_t* links() const {
    return reinterpret_cast<const int64_t*>(obs + L.ob_edge_links) + (int64_t)eid * L.edge_cap * 2;
  }

  // Weighted fair on the observation: W(k) over the job's rows in row order, find_stage, ob_supplies
  __device__ __forceinline__ StepIn wfair(int kind) const {
    const int32_t* c = counts();
    const int32_t* p = ptr();
    const int32_t* su = sup();
    const float* nd = nodes();
    return wfair_act<W>(
        wfair_alpha2(kind), L.num_executors, W::uni(c[SSIM_OC_NUM_JOBS]), W::uni(c[SSIM_OC_COMMITTABLE]),
        W::uni(c[SSIM_OC_SOURCE_JOB_IDX]),
        [&](int k) {
          double sum = 0.0;
          for (int r = p[k]; r < p[k + 1]; ++r) sum += (double)nd[3 * r] * (double)nd[3 * r + 1];
          return sum;
        },
        [&](int k) { return find_stage(k); }, [&](int k) { return su[k]; });
  }

  // SJF / SJF-CP on the observation (the rule at the top of this file, the specification's own arrays); the
  // weighted-fair kinds share the entry
  __device__ __forceinline__ StepIn prio_act(int kind) const {
    if (policy_is_wfair(kind)) return wfair(kind);
    const int32_t* c = counts();
    const int32_t* p = ptr();
    const float* nd = nodes();
    const int nj = W::uni(c[SSIM_OC_NUM_JOBS]), comm = W::uni(c[SSIM_OC_COMMITTABLE]);
    StepIn a;
    a.stage_idx = -1;
    a.num_exec = comm > 0 ? comm : 1;
    const int ks = prio_job<W>(
        nj,
        [&](int k) {
          double sum = 0.0;
          for (int r = p[k]; r < p[k + 1]; ++r) sum += (double)nd[3 * r] * (double)nd[3 * r + 1];
          return sum;
        },
        [&](int k) { return find_stage(k); });
    if (ks < 0) return a;
    a.num_exec = comm;
    if (kind == SSIM_POLICY_SJF) {
      a.stage_idx = W::uni(find_stage(ks));
      return a;
    }
    const int lo = W::uni(p[ks]), hi = W::uni(p[ks + 1]);
    if (hi - lo > kPrioMaxStages) return a;  // (ssim_policy refuses the config: max_stages > 64)
    // the job's edges: the list is in node order, so they are the entries [e0, e1) with e0 = #(u < lo), e1 = #(u < hi)
    const int64_t* ln = links();
    int ne = W::uni(c[SSIM_OC_NUM_EDGES]);
    ne = ne < L.edge_cap ? ne : L.edge_cap;
    int e0 = 0, e1 = 0;
    for (int i0 = 0; i0 < ne; i0 += W::kWidth) {
      const int i = i0 + W::lane();
      const int64_t u = i < ne ? ln[2 * i] : (int64_t)hi;
      e0 += W::popc(W::ballot(u < lo));
      e1 += W::popc(W::ballot(u < hi));
    }
    const int32_t* sr = srank();
    a.stage_idx = prio_cp_stage<W>(hi - lo, [&](int l, double* w, uint64_t* kids, int* rank) {
      const int r = lo + l;
      *w = (double)nd[3 * r] * (double)nd[3 * r + 1];
      *rank = sr[r];
      uint64_t m = 0;
      for (int e = e0; e < e1; ++e) {
        const int64_t v = ln[2 * e + 1] - lo;
        if (ln[2 * e] == r && v >= 0 && v < hi - lo) m |= 1ull << v;
      }
      *kids = m;
    });
    return a;
  }

  __device__ __forceinline__ StepIn act(int kind, uint64_t seed, uint64_t counter) const {
    if (policy_is_prio(kind)) return prio_act(kind);
    const int32_t* c = counts();
    const int32_t* su = sup();
    return policy_act<W>(kind, seed, counter, eid, L.num_executors, c[SSIM_OC_NUM_JOBS], c[SSIM_OC_COMMITTABLE],
                         c[SSIM_OC_SOURCE_JOB_IDX], [&](int k) { return find_stage(k); },
                         [&](int k) { return su[k]; });
  }
};

// The fused rollout's policy input: the header (loaded) and the picks of the env's last observation
// (Sim::observe), read from the hot block instead of the obs arena the same wave just wrote. Fair / FIFO / random only
// (HeuristicPolicy, the tuned k_rollout instantiations).
template <class SimT>
__device__ __forceinline__ StepIn sim_policy_legacy(SimT& s, int kind, uint64_t seed) {
  using W = typename SimT::WT;
  const int16_t* aj = s.template H<int16_t>(s.O.active_jobs);
  const uint64_t counter = (uint64_t)s.h.decisions + ((uint64_t)s.h.episode << 32);
  return policy_act<W>(
      kind, seed, counter, s.eid, s.NE, s.h.n_active_jobs, s.committable(), s.h.src_idx,
      [&](int k) {
        const int key = s.job(aj[k]).pick;
        return key == 0x7FFFFFFF ? -1 : (key & 0xFFFF);
      },
      [&](int k) { return (int)s.job(aj[k]).supply; });
}

// SJF / SJF-CP from the hot block: PolicyView::prio_act's rule on the stage records. A job's rows are its stages
// that are not completed, in stage order (the active-stage list keeps node order), so its work is summed over all its
// stage records (a completed stage has no remaining task: it adds +0.0, which changes no sum) and the CP lanes are its
// local stage ids, a completed stage standing for no row. Children come from the dataset's topology (the bit sets of
// templates of <= 32 stages, else the child lists) with observe()'s liveness test; the schedulable rows and their ranks
// from the schedulable list observe() wrote (ascending stage index: one job's entries are contiguous).
// Weighted fair from the hot block: PolicyView::wfair's rule on the stage records (W(k) as sim_policy_prio's, over all
// of the job's stage records), the picks and supplies of the job records, the header's source job.
template <class SimT>
__device__ __forceinline__ StepIn sim_policy_wfair(SimT& s, int kind) {
  using W = typename SimT::WT;
  const int16_t* aj = s.template H<int16_t>(s.O.active_jobs);
  const double* recent = s.recent();
  return wfair_act<W>(
      wfair_alpha2(kind), s.NE, s.h.n_active_jobs, s.committable(), s.h.src_idx,
      [&](int k) {
        const JobRec jr = s.job(aj[k]);
        double sum = 0.0;
        for (int g = jr.base; g < jr.base + jr.nst; ++g) {
          const StageRec sr = s.stage(g);
          sum += (double)(float)sr.rem * (double)(float)recent[g];
        }
        return sum;
      },
      [&](int k) {
        const int key = s.job(aj[k]).pick;
        return key == 0x7FFFFFFF ? -1 : (key & 0xFFFF);
      },
      [&](int k) { return (int)s.job(aj[k]).supply; });
}

template <class SimT>
__device__ __forceinline__ StepIn sim_policy_prio(SimT& s, int kind) {
  using W = typename SimT::WT;
  const int16_t* aj = s.template H<int16_t>(s.O.active_jobs);
  const double* recent = s.recent();
  const int comm = s.committable();
  StepIn a;
  a.stage_idx = -1;
  a.num_exec = comm > 0 ? comm : 1;
  const auto pick = [&](int k) {
    const int key = s.job(aj[k]).pick;
    return key == 0x7FFFFFFF ? -1 : (key & 0xFFFF);
  };
  const auto work = [&](int g) {
    const StageRec sr = s.stage(g);
    return (double)(float)sr.rem * (double)(float)recent[g];
  };
  const int ks = prio_job<W>(
      s.h.n_active_jobs,
      [&](int k) {
        const JobRec jr = s.job(aj[k]);
        double sum = 0.0;
        for (int g = jr.base; g < jr.base + jr.nst; ++g) sum += work(g);
        return sum;
      },
      pick);
  if (ks < 0) return a;
  a.num_exec = comm;
  if (kind == SSIM_POLICY_SJF) {
    a.stage_idx = W::uni(pick(ks));
    return a;
  }
  const int j = W::uni(aj[ks]);
  const int base = s.job_base(j), nst = s.job_nst(j);
  if (nst > kPrioMaxStages) return a;  // (the rollout entry points refuse the config: max_stages > 64)
  const typename SimT::TopoView tv = s.topo_view();
  // the job's schedulable stages as a set of local ids, and the rank of the first of them
  const int16_t* sched = s.template H<int16_t>(s.O.sched_list);
  const int nsched = s.h.n_sched;
  uint64_t smask = 0;
  int first = -1;
  for (int r0 = 0; r0 < nsched; r0 += W::kWidth) {
    const int r = r0 + W::lane();
    const int g = r < nsched ? (int)sched[r] : -1;
    uint64_t m = W::ballot(g >= base && g < base + nst);
    if (m != 0 && first < 0) first = r0 + W::ffs(m);
    for (; m != 0; m &= m - 1) smask |= 1ull << (W::bcast_i(g, W::ffs(m)) - base);
  }
  a.stage_idx = prio_cp_stage<W>(nst, [&](int l, double* w, uint64_t* kids, int* rank) {
    const StageRec sr = s.stage(base + l);
    if (sr.rem == 0 && sr.exe == 0) return;  // completed: not a row of the observation
    *w = (double)(float)sr.rem * (double)(float)recent[base + l];
    if ((smask >> l) & 1ull) *rank = first + __builtin_popcountll(smask & ((1ull << l) - 1ull));
    uint64_t m = 0;
    const auto add_child = [&](int b) {
      if (b < 0 || b >= nst) return;
      const StageRec c = s.stage(base + b);
      if (!(c.rem == 0 && c.exe == 0)) m |= 1ull << b;
    };
    if (tv.bits) {
      for (uint32_t cm = (uint32_t)(ldg(tv.ts_topo, sr.ts) >> 32); cm != 0; cm &= cm - 1) add_child(__builtin_ctz(cm));
    } else {
      for (int k = ldg(tv.child_base, sr.ts); k < ldg(tv.child_base, sr.ts + 1); ++k) add_child(ldg(tv.children, k));
    }
    *kids = m;
  });
  return a;
}

// Any kind, from the hot block (the host build's rollout loop; the device kernels call the driver of their family).
template <class SimT>
__device__ __forceinline__ StepIn sim_policy(SimT& s, int kind, uint64_t seed) {
  if (policy_is_wfair(kind)) return sim_policy_wfair(s, kind);
  return policy_is_prio(kind) ? sim_policy_prio(s, kind) : sim_policy_legacy(s, kind, seed);
}

}  // namespace ssim
