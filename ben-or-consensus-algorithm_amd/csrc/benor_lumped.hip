// benor_lumped.hip -- the adversarial scheduler at the level of classes (bo_lumped_*,
// include/benor.h).
//
// One trial loop, a template over the rule (lumped::RuleRef, lumped::RuleB, and
// lumped::RuleT, the threshold rule of three runtime words behind bo_lumped_*_rule,
// DESIGN §4.3.13) and over the coin a P-phase takes (CoinLocal, CoinShared): six entries.  The chain itself -- the
// scheduler's closed forms, the rules on scalars, a round, the outcome bins, the
// Binomial(n, 1/2) draw -- is benor_lumped.h, shared with the host; this file supplies
// the words: Philox stream 12 for a round's common coin, stream 13 for the Binomial draws.
//
// One lane = one trial.  A lane's state is (H0, H1), (a_0, a_1), the two decided flags and
// the round, all in registers; there is no per-node plane and no per-wave LDS.  A lane that
// ends a trial records it and starts its next trial id in the same loop iteration, so a wave
// keeps stepping rounds with every lane busy until the launch runs out of trials.  Every
// random word is keyed by the trial id: results do not depend on the lane, the grid or the
// launch split.  A round with no local coin is a few dozen integer instructions whatever N
// is; a local coin costs one Philox block per two set bits of h_pi and, for a set bit k >= 7,
// a search of at most 17 steps in that k's thresholds (k = 24 holds about 37 000, searched
// from 2^16), read where they lie in global memory (all tables together are about 1 MB and
// stay in L2; the small ones are not staged in LDS).
// The workgroup's histogram is in LDS (flush_hist's scheme).  No floating point runs on the
// device; scalar memory traffic is loads only.
#include "benor_device.h"

namespace benor {

namespace {

using lumped::Shape;
using lumped::State;

struct CoinLocal {
  static constexpr bool kShared = false;
};
struct CoinShared {
  static constexpr bool kShared = true;
};

// The j-th 64-bit word of a draw: block j >> 1 of {trial_lo, trial_hi, c2 + (j >> 1), c3}, its low pair for an
// even j and its high pair for an odd one.  Words are asked for in order, so a block serves two.
struct Words {
  uint32_t k0, k1, tlo, thi, c2, c3;
  uint4 blk;
  __device__ __forceinline__ uint64_t operator()(uint32_t j) {
    if (!(j & 1u)) {
      blk = philox4x32_10(k0, k1, make_uint4(tlo, thi, c2 + (j >> 1), c3));
      return (uint64_t)blk.y << 32 | blk.x;
    }
    return (uint64_t)blk.w << 32 | blk.z;
  }
};

// What lumped::round asks of a trial: the round's coin state and a parity's Binomial draw.
template <class Coin>
struct Source {
  const lumped::TableDir &tables;
  uint32_t k0, k1, coin_common;
  uint32_t tlo, thi;                               // the lane's trial id
  __device__ __forceinline__ uint32_t common(uint32_t r) const {
    if constexpr (!Coin::kShared) {
      return 1u;
    } else {
      const uint4 b = philox4x32_10<false>(k0, k1, make_uint4(tlo, thi, 0u, (r - 1u) | (kStreamCommonCoin << 24)));
      return (coin_common == 0xFFFFFFFFu || b.x < coin_common) ? 2u | (b.y & 1u) : 1u;
    }
  }
  __device__ __forceinline__ uint32_t binom(uint32_t n, uint32_t pi, uint32_t r) const {
    Words w{k0, k1, tlo, thi, 16u * pi, r | (lumped::kStreamBinom << 24), make_uint4(0u, 0u, 0u, 0u)};
    return lumped::binom_half(n, w, tables);
  }
};

// Launch bounds: 256 lanes, no occupancy asked for -- the report in DESIGN §4.3.12 gives each entry's VGPRs
// (no spill, no scratch); LDS is the histogram alone (at most 12.3 KB at k_max = 1024).
template <class Rule, class Coin>
__global__ void __launch_bounds__(kLumpedBlock) benor_lumped_kernel(LumpedParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);
  for (uint32_t i = threadIdx.x; i < p.hist_len; i += blockDim.x) lhist[i] = 0u;
  __syncthreads();

  const Shape s = p.s;
  Rule rule{};                                     // (empty for the compile-time rules)
  if constexpr (Rule::kRule == lumped::RuleT::kRule) rule.t = p.thresholds;
  Source<Coin> src{p.tables, (uint32_t)p.seed, (uint32_t)(p.seed >> 32), p.coin_common, 0u, 0u};
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;

  State st;
  uint32_t r = 0u;
  // A trial's start: its id into the word source, and the class sizes round 1 reads.
  auto start = [&]() {
    const uint64_t trial = p.trial_begin + t;
    src.tlo = (uint32_t)trial, src.thi = (uint32_t)(trial >> 32);
    st.a[0] = st.a[1] = 0u, st.dec = 0u, r = 0u;
    if (p.init_mode == BO_INIT_RANDOM) {
      st.H1 = src.binom(s.hh, 0u, 0u);
      st.H0 = s.hh - st.H1;
    } else {
      st.H0 = p.init0, st.H1 = p.init1;
    }
  };

  bool live = t < p.trial_count;
  if (live) start();
  while (live) {
    ++r;
    const bool all_dec = lumped::round(rule, s, r, st, src);
    if (all_dec || r == p.k_max) {
      bool violation;
      const uint32_t bin = lumped::outcome_bin(st.a[0] + st.a[1], s.hh, all_dec, r, violation);
      atomicAdd(&lhist[bin], 1u);
      if (violation) atomicAdd(&lhist[p.hist_len - 1u], 1u);
      if (p.state_out) {                           // a one-trial launch
        bo_lumped_state o;
        o.a[0] = st.a[0], o.a[1] = st.a[1];
        o.dec[0] = (uint8_t)(st.dec & 1u), o.dec[1] = (uint8_t)((st.dec >> 1) & 1u);
        o.pad[0] = o.pad[1] = 0;
        o.rounds = all_dec ? r : 0u;
        *p.state_out = o;
      }
      t += stride;                                 // the lane's next trial, in the same iteration
      live = t < p.trial_count;
      if (live) start();
    }
  }

  __syncthreads();
  for (uint32_t i = threadIdx.x; i < p.hist_len; i += blockDim.x) {
    const uint32_t c = lhist[i];
    if (c) atomicAdd(&p.hist[i], (unsigned long long)c);
  }
}

using LumpedKernel = void (*)(LumpedParams);
LumpedKernel lumped_entry(const LumpedParams &p) {
  const bool shared = p.coin_common != 0u;
  if (p.rule == lumped::RuleT::kRule)
    return shared ? benor_lumped_kernel<lumped::RuleT, CoinShared> : benor_lumped_kernel<lumped::RuleT, CoinLocal>;
  if (p.rule == lumped::RuleB::kRule)
    return shared ? benor_lumped_kernel<lumped::RuleB, CoinShared> : benor_lumped_kernel<lumped::RuleB, CoinLocal>;
  return shared ? benor_lumped_kernel<lumped::RuleRef, CoinShared> : benor_lumped_kernel<lumped::RuleRef, CoinLocal>;
}

}  // namespace

int lumped_blocks_per_cu(const LumpedParams &p) {
  int n = 0;
  const hipError_t e =
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, lumped_entry(p), kLumpedBlock, p.hist_len * sizeof(uint32_t));
  return e == hipSuccess ? n : 0;
}

hipError_t launch_lumped(const LumpedParams &p, int grid, hipStream_t s) {
  if (p.rule > lumped::RuleT::kRule || (p.rule == lumped::RuleT::kRule && rule::check(p.thresholds, nullptr) != BO_OK) ||
      p.s.hh == 0u || p.s.q == 0u || p.s.hh < p.s.q || p.s.N > lumped::kMaxN || p.k_max == 0u ||
      p.hist_len != (p.k_max + 1u) * 3u + 1u || !p.hist || !p.tables.thr || !p.tables.off || !p.tables.lo ||
      (p.state_out && p.trial_count != 1u) || grid < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(lumped_entry(p), dim3(grid), dim3(kLumpedBlock), p.hist_len * sizeof(uint32_t), s, p);
  return hipGetLastError();
}

}  // namespace benor
