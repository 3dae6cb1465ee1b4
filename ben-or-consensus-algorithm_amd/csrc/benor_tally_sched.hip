// benor_tally_sched.hip -- count-level delivery under an adversarial scheduler
// (BO_MODE_SCHED_TALLY, BO_MODE_SCHED_RULE_B).
//
// One trial loop, a template over the rule applied to a receiver's counts (RuleRef,
// RuleB, RuleT) and over the coin a P-phase takes (CoinLocal, CoinShared; all five in
// benor_tally_common.h): variant 18 runs <RuleRef, CoinLocal>, variant 19 <RuleB,
// CoinLocal>, and variants 20 and 21 the same two rules with <CoinShared>.  A plan of
// variant 19 or 21 whose rule is replaced by a threshold rule (bo_plan_create_rule,
// KParams::rule_on) runs <RuleT, CoinLocal> or <RuleT, CoinShared>.
//
// The model is benor_tally_byz.hip's -- b of the m live nodes Byzantine, the h = m - b
// honest ones run the rule and alone receive -- except for who is heard: the adversary,
// not a draw, picks the q senders of every honest receiver c at every step, and what each
// Byzantine sender among them says.  With (H0, H1, Hq) the step's class sizes over the
// honest senders (h >= q, since f + b <= F) the receiver's counts are a closed form:
//   push(v):  c_v = min(q, H_v + b), rest = q - c_v, c_{1-v} = rest - min(rest, Hq)
//             (the most v any inbox allows, then the least 1 - v)
//   even():   hq = min(q, Hq), r = q - hq, lo = r - min(r, H1 + b), hi = min(r, H0 + b),
//             c0 = clamp((r + (c & 1)) >> 1, lo, hi), c1 = r - c0
//             ("?" first, then the two tallies as level as the senders allow)
// BO_BYZ_SPLIT is push(c & 1) in both phases, BO_BYZ_BALANCE even() in both.  Either way
// a step's (c0, c1) takes two values, one per parity of c, and the lane's parity is its
// receiver's in every group (c = 64 j + lane): both are computed wave-uniformly from the
// popcounted class sizes and each lane selects its own.  No table, no threshold search, no
// selection-sampling walk: no word of streams 5, 6, 10 or 11 is drawn.  What a node-round
// costs is the rule's ballots and, for the lanes that take a coin, coin_ballot's Philox
// block (the coin stream of every batch mode; a common round of CoinShared runs none).
//
// One wave = one trial, lane l of receiver group j = compact index 64 j + l over the m
// live nodes, on the helpers of benor_tally_common.h.  Per-wave LDS is byz_layout(W, 0,
// states): the planes HP (honest, constant per plan), X1, P1, P0 of W words (X0, read
// only by round 1's class sizes, lies in P0's words) and a decided plane in a
// per-node-state launch; no row region, nothing behind the waves' regions.  An R-phase
// writes all W proposal words at once -- the ballots of the two parities, ANDed with
// each group's honest lanes, lane w writing word w -- so a group without an honest lane
// proposes nothing and a Byzantine lane never sets a bit; the P-phase walks the groups
// that have an honest lane, as benor_tally_heard_kernel does.  Histogram and the state
// launch are that kernel's.  No floating point runs on the device, and no launch leaves
// overflow or deferral state.
#include "benor_tally_common.h"

namespace benor {

namespace {

// A receiver's counts under the two strategies; every argument may be wave-uniform.
__device__ __forceinline__ void sched_push(uint32_t v, uint32_t q, uint32_t H0, uint32_t H1, uint32_t Hq, uint32_t nb,
                                           uint32_t &c0, uint32_t &c1) {
  const uint32_t Hv = v ? H1 : H0;
  const uint32_t cv = Hv + nb < q ? Hv + nb : q;
  const uint32_t rest = q - cv;
  const uint32_t co = rest - (rest < Hq ? rest : Hq);
  c0 = v ? co : cv;
  c1 = v ? cv : co;
}

__device__ __forceinline__ void sched_even(uint32_t odd, uint32_t q, uint32_t H0, uint32_t H1, uint32_t Hq, uint32_t nb,
                                           uint32_t &c0, uint32_t &c1) {
  const uint32_t hq = q < Hq ? q : Hq;
  const uint32_t r = q - hq;
  const uint32_t lo = r - (r < H1 + nb ? r : H1 + nb);
  const uint32_t hi = r < H0 + nb ? r : H0 + nb;   // lo <= hi: r <= H0 + H1 + 2 nb
  uint32_t c = (r + odd) >> 1;
  c = c < lo ? lo : c;
  c = c > hi ? hi : c;
  c0 = c;
  c1 = r - c;
}

// The lane's (c0, c1) of a step with honest class sizes (H0, H1, Hq): the two parities' counts,
// wave-uniform, and the lane's pick.
__device__ __forceinline__ void sched_counts(uint32_t strategy, uint32_t q, uint32_t H0, uint32_t H1, uint32_t Hq,
                                             uint32_t nb, uint32_t lane, uint32_t &c0, uint32_t &c1) {
  uint32_t e0, e1, o0, o1;
  if (strategy == BO_BYZ_SPLIT) {
    sched_push(0u, q, H0, H1, Hq, nb, e0, e1);
    sched_push(1u, q, H0, H1, Hq, nb, o0, o1);
  } else {
    sched_even(0u, q, H0, H1, Hq, nb, e0, e1);
    sched_even(1u, q, H0, H1, Hq, nb, o0, o1);
  }
  const bool odd = lane & 1u;
  c0 = odd ? o0 : e0;
  c1 = odd ? o1 : e1;
}

// Launch bounds: the six entries compile to 47 or 48 VGPRs with no VGPR spill under a bound of
// eight waves per SIMD -- all a SIMD holds, a workgroup being one wave per SIMD -- so that bound is
// asked for (SGPR spills, 34 to 80 words, go to VGPR lanes within those 48); LDS allows more than
// eight workgroups at every W (at W = 64: 8 KiB of planes and the histogram per workgroup).
template <class Rule, class Coin>
__global__ void __launch_bounds__(256, 8) benor_tally_sched_kernel(KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t N = p.N, F = p.F, W = p.W, q = p.q, nb = p.byz_n, strategy = p.byz_strategy;

  uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);
  const bool states = p.node_out != nullptr;       // a state launch: a DEC plane of its own
  const Planes S(smem + p.hist_bytes + wv * p.wave_bytes, byz_layout(W, 0u, states));
  uint64_t *const HP = S.AL, *const X1 = S.X1, *const P1 = S.P1, *const P0 = S.P0, *const X0 = S.X0;

  for (uint32_t i = threadIdx.x; i < p.hist_len; i += blockDim.x) lhist[i] = 0u;
  for (uint32_t w = lane; w < W; w += 64u) HP[w] = p.byz_plane[w];
  __syncthreads();

  uint32_t h = 0u;                                 // honest nodes
  for (uint32_t j = 0; j < W; ++j) h += (uint32_t)__builtin_popcountll(HP[j]);
  h = uni(h);

  const uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32);
  const uint64_t waves_total = (uint64_t)gridDim.x * kWavesPerBlock;
  Coin coin = make_coin<Coin>(p);
  const Rule rl = make_rule<Rule>(p);             // (empty for the compile-time rules)

  for (uint64_t t = (uint64_t)blockIdx.x * kWavesPerBlock + wv; t < p.trial_count; t += waves_total) {
    const uint64_t trial = p.trial_begin + t;
    const uint32_t tlo = uni((uint32_t)trial), thi = uni((uint32_t)(trial >> 32));
    __builtin_amdgcn_wave_barrier();               // the previous trial's state reads are done
    trial_start<true>(X1, X0, p, k0, k1, trial, tlo, thi, lane);
    __builtin_amdgcn_wave_barrier();

    uint64_t dec = 0ull;                           // bit j: node 64 j + lane has decided (sticky)
    uint32_t R = 0;
    bool all_dec = false;
    for (uint32_t r = 1; r <= p.k_max; ++r) {
      coin.round_start();
      // ---- R-phase ("proposal phase", node.ts:46-82)
      uint32_t H0 = 0, H1 = 0;
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t hp = HP[j];
        if (r == 1u) H0 += (uint32_t)__builtin_popcountll(X0[j] & hp);
        H1 += (uint32_t)__builtin_popcountll(X1[j] & hp);
      }
      H1 = uni(H1);
      H0 = r == 1u ? uni(H0) : h - H1;             // after a P-phase every honest x is binary
      uint32_t c0, c1;
      sched_counts(strategy, q, H0, H1, h - H0 - H1, nb, lane, c0, c1);   // ("?" starts: round 1 only)
      {
        uint64_t a0, a1;                           // the proposals of a group whose 64 lanes are all honest
        rl.r(c0, c1, N, F, ~0ull, a0, a1);
        __builtin_amdgcn_wave_barrier();           // the class sizes are read before P0 takes X0's words
        for (uint32_t w = lane; w < W; w += 64u) {
          const uint64_t hp = HP[w];
          P0[w] = a0 & hp, P1[w] = a1 & hp;
        }
      }
      // ---- P-phase ("voting phase", node.ts:83-158)
      __builtin_amdgcn_wave_barrier();
      H0 = 0, H1 = 0;
      for (uint32_t j = 0; j < W; ++j) {
        H0 += (uint32_t)__builtin_popcountll(P0[j]);   // proposals are honest nodes' only
        H1 += (uint32_t)__builtin_popcountll(P1[j]);
      }
      H0 = uni(H0), H1 = uni(H1);
      sched_counts(strategy, q, H0, H1, h - H0 - H1, nb, lane, c0, c1);
      bool undecided = false;
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t hp = uni64(HP[j]);
        if (!hp) continue;                         // a group without an honest lane takes no coin
        const bool mine = (hp >> lane) & 1ull;     // this lane's node is honest
        bool decided;
        const uint64_t x1 = rl.p(c0, c1, N, F, hp, k0, k1, tlo, thi, j, r, decided, coin);
        if (mine && decided) dec |= 1ull << j;     // sticky
        undecided = undecided || (mine && !((dec >> j) & 1ull));
        if (lane == 0) X1[j] = (X1[j] & ~hp) | x1;                       // a Byzantine node's bit is never written
      }
      R = r;
      all_dec = !__any(undecided);                 // over the honest nodes
      if (all_dec) break;
    }
    __builtin_amdgcn_wave_barrier();
    uint32_t K = 0;                                // the honest nodes with x = 1
    for (uint32_t j = 0; j < W; ++j) K += (uint32_t)__builtin_popcountll(X1[j] & HP[j]);
    K = uni(K);
    trial_end(lhist, p, K, h, false, all_dec, R, lane);
    if (states) write_states<false>(p, HP, X1, X0, S.DEC, nullptr, 0u, dec, R, lane);
  }

  __syncthreads();
  flush_hist(lhist, p);
}

}  // namespace

// The entry of a plan: its rule and coin by the variant; a plan whose rule is replaced (rule_on, a Protocol B
// plan: the launch checks) takes the threshold rule's entry of its coin.
using SchedKernel = void (*)(KParams);
static SchedKernel sched_entry(const KParams &p) {
  if (p.rule_on)
    return variant_shared_coin(p.variant) ? benor_tally_sched_kernel<RuleT, CoinShared> : benor_tally_sched_kernel<RuleT, CoinLocal>;
  switch (p.variant) {
    case sched_variant(BO_MODE_SCHED_TALLY, false): return benor_tally_sched_kernel<RuleRef, CoinLocal>;
    case sched_variant(BO_MODE_SCHED_RULE_B, false): return benor_tally_sched_kernel<RuleB, CoinLocal>;
    case sched_variant(BO_MODE_SCHED_TALLY, true): return benor_tally_sched_kernel<RuleRef, CoinShared>;
    case sched_variant(BO_MODE_SCHED_RULE_B, true): return benor_tally_sched_kernel<RuleB, CoinShared>;
    default: return nullptr;
  }
}

// Workgroups of the kernel that one CU holds at once (registers and LDS; 0 = unknown).
int sched_blocks_per_cu(const KParams &p) { return variant_sched(p.variant) ? blocks_per_cu(sched_entry(p), p) : 0; }

// The scheduler's variants.  All run without a Byzantine node too (byz_n = 0: crash-only adversarial scheduling);
// the shared-coin ones need coin_common != 0, the others have every coin local.
hipError_t launch_tally_sched(const KParams &plan, int grid, hipStream_t s) {
  const KParams p = state_launch(plan, byz_state_bytes(plan.W));
  const bool shared = variant_shared_coin(p.variant);
  if (!variant_sched(p.variant) || !p.byz_plane || p.W == 0u || p.W > kMaxW || p.q > p.m ||
      (p.byz_strategy != BO_BYZ_BALANCE && p.byz_strategy != BO_BYZ_SPLIT) || shared != (p.coin_common != 0u) ||
      (p.rule_on && (!variant_rule_b(p.variant) || rule::check(p.rule, nullptr) != BO_OK)) || p.byz_n > p.m - p.q || plan.wave_bytes < byz_wave_bytes(p.W, 0u) ||
      plan.lds_bytes < p.hist_bytes + kWavesPerBlock * plan.wave_bytes)
    return hipErrorInvalidValue;
  return launch_lds(sched_entry(p), p, grid, s);
}

}  // namespace benor
