// benor_tally_byz.hip -- three-valued count-level random delivery with Byzantine
// senders (BO_MODE_BYZ_TALLY with b > 0 Byzantine nodes), and the same
// under Ben-Or's Byzantine-tolerant rule (BO_MODE_BYZ_RULE_B, b >= 0).
//
// Two trial loops, each a template over the rule applied to a receiver's counts
// (RuleRef, RuleB) and over the coin a P-phase takes (CoinLocal, CoinShared; all four
// in benor_tally_common.h): variant 14 runs <RuleRef, CoinLocal>, variant 15 <RuleB,
// CoinLocal>, and variants 16 and 17 the same two rules with <CoinShared>, the shared
// coin of BO_MODE_BYZ_COIN and BO_MODE_BYZ_RULE_B_COIN.  A plan of
// variant 15 or 17 whose rule is replaced by a threshold rule (bo_plan_create_rule,
// KParams::rule_on) runs the same two loops with <RuleT, CoinLocal> or
// <RuleT, CoinShared>.  Everything else in this comment holds for all of them.
//
// The model is benor_tally3.hip's with b of the m live nodes Byzantine: they send
// at every step and lie, they never receive.  The h = m - b honest nodes run the
// rule; honest receiver c draws q messages from all m senders.  With (H0, H1, Hq)
// the class sizes over the honest senders and B1 of the b Byzantine messages that
// could reach c carrying a 1, its (c0, c1) is draw3 among m senders with the class
// sizes (H0 + b - B1, H1 + B1, Hq).  B1 is
//   BO_BYZ_RANDOM: Binomial(b, byz_one / 2^32) per (receiver, round, phase):
//     #{ j : thr[j] <= u }, thr the plan's b thresholds (bo_byz_cdf), u from the
//     Philox block {trial_lo, trial_hi, c, (r - 1) | 10 << 24} (stream 10; R-phase
//     out[1] << 32 | out[0], P-phase out[3] << 32 | out[2]); 0 at byz_one = 0 and b
//     at UINT32_MAX without a draw;
//   BO_BYZ_OPPOSE: 0 if H1 > H0, b if H0 > H1, for every receiver; BO_BYZ_RANDOM's
//     step on H0 == H1.
// BO_BYZ_BALANCE and BO_BYZ_SPLIT, whose liars see the receiver's inbox, run a second
// loop of this file, benor_tally_heard_kernel (further down).
//
// One wave = one trial, lane l of receiver group j = compact index 64 j + l over
// the m live nodes, as in benor_tally_crash.hip, on the same helpers
// (benor_tally_common.h).  Its alive plane is here the honest plane HP,
// constant per plan: class sizes are popcounts of the x and proposal planes ANDed
// with it, a group without an honest lane draws nothing, and a Byzantine lane
// never writes a plane bit.  A step is one of two kinds, wave-uniformly:
//   * every receiver hears the same Byzantine messages (OPPOSE off a tie, byz_one 0
//     or UINT32_MAX): the phase is set up once with its row staged in LDS and the
//     honest lanes draw from it (phase_setup and draw3, mode 4's step with shifted
//     class sizes);
//   * each receiver has a B1 of its own: one stream-10 block per lane next to the
//     stream-5 block, a binary search of the Binomial thresholds, and one per-lane
//     draw from the lane's own row of the (m, q) table in global memory
//     (draw3_lane, as benor_tally_subset.hip, with one table and no directory).
//     Neighbouring lanes' B1 differ by O(sqrt b), so the rows they touch lie close.
// The thresholds, 8 b <= 32 KiB shared by every trial, are copied into LDS once
// per workgroup, behind the four waves' regions, when that costs no resident
// workgroup (byz_thr_in_lds); otherwise they are searched in global memory.
//
// Per-wave LDS: the planes HP, X1, P1, P0 of W words (X0, read only by round 1's
// class sizes, lies in P0's words), a decided plane in a per-node-state launch,
// and the row region.  Histogram and the state launch are benor_tally_crash.hip's
// with the honest nodes in the place of the alive ones; a Byzantine node's state is
// not written (the host reports it).  No floating point runs on the device, and no
// launch leaves overflow or deferral state.
#include "benor_tally_common.h"

namespace benor {

namespace {

constexpr uint32_t kByzCertain = 0xFFFFFFFFu;      // KParams::byz_one: every Byzantine message carries 1
constexpr uint32_t kByzWgPerCu = 6u;               // resident workgroups the registers allow (__launch_bounds__ below)

// (RuleRef, RuleB and make_coin: benor_tally_common.h, shared with benor_tally_sched.hip)

// The oblivious strategies (BO_BYZ_RANDOM, BO_BYZ_OPPOSE), for either rule: benor_tally_byz_kernel<RuleRef> is
// variant 14's entry, <RuleB> variant 15's.  The entries themselves are the templates: a rule-templated
// device function called from two plain entries compiles variant 14 with six more SGPR spills.
// (six waves per SIMD: one more than benor_tally_crash.hip, there is no schedule and no alive plane to maintain)
template <class Rule, class Coin>
__global__ void __launch_bounds__(256, 6) benor_tally_byz_kernel(KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t N = p.N, m = p.m, F = p.F, W = p.W, q = p.q, nb = p.byz_n;

  uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);
  const bool states = p.node_out != nullptr;       // a state launch: a DEC plane of its own
  const Planes S(smem + p.hist_bytes + wv * p.wave_bytes, byz_layout(W, p.tally_cap, states));
  uint64_t *const HP = S.AL, *const X1 = S.X1, *const P1 = S.P1, *const P0 = S.P0, *const X0 = S.X0, *const row = S.row;
  uint64_t *BT = reinterpret_cast<uint64_t *>(smem + p.hist_bytes + kWavesPerBlock * p.wave_bytes);   // [b] (byz_lds)
  const bool in_lds = p.byz_lds != 0u;
  const uint32_t bsteps = search_steps(nb);

  for (uint32_t i = threadIdx.x; i < p.hist_len; i += blockDim.x) lhist[i] = 0u;
  if (in_lds)
    for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) BT[i] = p.byz_thr[i];
  for (uint32_t w = lane; w < W; w += 64u) HP[w] = p.byz_plane[w];
  __syncthreads();

  uint32_t h = 0u;                                 // honest nodes
  for (uint32_t j = 0; j < W; ++j) h += (uint32_t)__builtin_popcountll(HP[j]);
  h = uni(h);

  const Table tb{m, p.tally_off, p.tally_thr};     // the plan's one table

  const uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32);
  const uint64_t waves_total = (uint64_t)gridDim.x * kWavesPerBlock;
  Coin coin = make_coin<Coin>(p);
  const Rule rl = make_rule<Rule>(p);             // (empty for the compile-time rules)

  // What the Byzantine senders say at a step with honest class sizes (H0, H1): true if every
  // receiver has a B1 of its own, else B1u for all of them.
  uint32_t B1u = 0u;
  const auto per_lane_step = [&](uint32_t H0, uint32_t H1) {
    if (p.byz_strategy == BO_BYZ_OPPOSE && H0 != H1) {
      B1u = H0 > H1 ? nb : 0u;
      return false;
    }
    B1u = p.byz_one == kByzCertain ? nb : 0u;
    if constexpr (Rule::kNoLiar || Coin::kShared)
      if (nb == 0u) return false;                  // no Byzantine node: byz_thr is not there to search
    return p.byz_one != 0u && p.byz_one != kByzCertain;
  };
  // A lane with a B1 of its own searches its row of the one table where it lies in global memory.
  const auto one_table = [&](uint32_t) { return tb; };
  // Receiver c's B1 from its stream-10 uniform.
  const auto lies = [&](uint64_t u) {
    return in_lds ? count_le(BT, nb, bsteps, u) : count_le<false>(p.byz_thr, nb, bsteps, u);
  };

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
      bool own = per_lane_step(H0, H1);
      PhaseC ph = phase_none();
      if (!own) ph = phase_setup(row, p, tb, H0 + nb - B1u, H1 + B1u, h - H0 - H1, lane);
      else __builtin_amdgcn_wave_barrier();        // the class sizes are read before P0 takes X0's words
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t hp = uni64(HP[j]);
        uint64_t p0 = 0ull, p1 = 0ull;
        if (hp) {                                  // a group without an honest lane draws nothing
          const uint32_t c = j * 64u + lane;
          // the round's block of receiver c: u_R = out[1] << 32 | out[0], u_P = out[3] << 32 | out[2]
          const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
          const uint64_t u = (uint64_t)b.y << 32 | b.x;
          uint32_t c0, c1;
          if (!own) {
            draw3(row, ph, m, q, k0, k1, tlo, thi, c, r, 0u, u, c0, c1);
          } else {
            const uint4 l = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamLie << 24)));
            const uint32_t B1 = lies((uint64_t)l.y << 32 | l.x);
            draw3_lane(one_table, p.tally_cap, 0u, m, q, H0 + nb - B1, H1 + B1, k0, k1, tlo, thi, c, r, 0u, u,
                       (hp >> lane) & 1ull, c0, c1);
          }
          rl.r(c0, c1, N, F, hp, p0, p1);
        }
        if (lane == 0) P0[j] = p0, P1[j] = p1;
      }
      // ---- P-phase ("voting phase", node.ts:83-158)
      __builtin_amdgcn_wave_barrier();
      H0 = 0, H1 = 0;
      for (uint32_t j = 0; j < W; ++j) {
        H0 += (uint32_t)__builtin_popcountll(P0[j]);   // proposals are honest nodes' only
        H1 += (uint32_t)__builtin_popcountll(P1[j]);
      }
      H0 = uni(H0), H1 = uni(H1);
      own = per_lane_step(H0, H1);
      if (!own) ph = phase_setup(row, p, tb, H0 + nb - B1u, H1 + B1u, h - H0 - H1, lane);
      bool undecided = false;
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t hp = uni64(HP[j]);
        if (!hp) continue;
        const uint32_t c = j * 64u + lane;
        const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
        const uint64_t u = (uint64_t)b.w << 32 | b.z;
        const bool mine = (hp >> lane) & 1ull;     // this lane's node is honest
        uint32_t c0, c1;
        if (!own) {
          draw3(row, ph, m, q, k0, k1, tlo, thi, c, r, 1u, u, c0, c1);
        } else {
          const uint4 l = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamLie << 24)));
          const uint32_t B1 = lies((uint64_t)l.w << 32 | l.z);
          draw3_lane(one_table, p.tally_cap, 0u, m, q, H0 + nb - B1, H1 + B1, k0, k1, tlo, thi, c, r, 1u, u, mine, c0,
                     c1);
        }
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

// ---- BO_BYZ_BALANCE, BO_BYZ_SPLIT: Byzantine senders that see the receiver's inbox
//
// The Byzantine messages are a class of their own inside the draw.  Stage 1 is mode 4's
// draw among m senders with the class sizes (H0, H1, Hq + b): wave-uniform, so every step
// is phase_setup + draw3 from the LDS row, and (h0, h1) are the honest 0s and 1s heard.
// Stage 2 splits the rest = q - h0 - h1 messages of the merged class into honest "?" and
// Byzantine ones, nB ~ Hypergeometric(Hq + b, b, rest): nothing is drawn at Hq = 0 (nB =
// rest; every step but a round-1 R-phase with "?" starts), else draw3's selection sampling
// over the smaller of the two sub-classes (the Byzantine one on a tie) from stream 11.
// The nB liars then say l1 ones and nB - l1 zeros, having seen (h0, h1).

// Stage 2: how many of receiver c's `rest` messages from the merged class of Hq honest "?"
// and nb Byzantine senders are Byzantine.  Hq and nb are wave-uniform, Hq != 0; a lane
// with rest = 0 draws nothing, and a lane whose count is settled stops taking words.
__device__ __forceinline__ uint32_t heard_byz(uint32_t Hq, uint32_t nb, uint32_t rest, uint32_t k0, uint32_t k1,
                                              uint32_t tlo, uint32_t thi, uint32_t c, uint32_t r, uint32_t phase) {
  const bool walk_byz = nb <= Hq;                  // the smaller sub-class is walked
  const uint32_t KW = walk_byz ? nb : Hq;
  const uint32_t dtop = Hq + nb;                   // >= rest, >= KW
  const uint32_t c3 = (r - 1u) | (phase << 16) | (kStreamHeard << 24);
  uint32_t i = 0, cS = 0;
  for (uint32_t blk = 0; __any(i < KW && cS < rest); ++blk) {
    const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c | (blk << 12), c3));
    walk_word(b.x, KW, dtop, rest, i, cS), walk_word(b.y, KW, dtop, rest, i, cS);
    walk_word(b.z, KW, dtop, rest, i, cS), walk_word(b.w, KW, dtop, rest, i, cS);
  }
  return walk_byz ? cS : rest - cS;
}

// Of the nB Byzantine messages in receiver c's inbox, how many say 1, given the honest
// (h0, h1) next to them.
__device__ __forceinline__ uint32_t heard_lies(uint32_t strategy, uint32_t c, uint32_t h0, uint32_t h1, uint32_t nB) {
  if (strategy == BO_BYZ_SPLIT) return (c & 1u) ? nB : 0u;
  const int32_t d = (int32_t)(h0 + nB) - (int32_t)h1;   // BO_BYZ_BALANCE: the tallies as equal as nB lies allow
  if (d <= 0) return 0u;
  const uint32_t half = (uint32_t)d >> 1;
  return half < nB ? half : nB;
}

// benor_tally_byz_kernel's trial loop with every step of the first kind: no Binomial
// thresholds (byz_thr and byz_lds are not read), no per-lane row.  byz_n > 0 (launch_tally_byz).
template <class Rule, class Coin>
__global__ void __launch_bounds__(256, 6) benor_tally_heard_kernel(KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t N = p.N, m = p.m, F = p.F, W = p.W, q = p.q, nb = p.byz_n, strategy = p.byz_strategy;

  uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);
  const bool states = p.node_out != nullptr;       // a state launch: a DEC plane of its own
  const Planes S(smem + p.hist_bytes + wv * p.wave_bytes, byz_layout(W, p.tally_cap, states));
  uint64_t *const HP = S.AL, *const X1 = S.X1, *const P1 = S.P1, *const P0 = S.P0, *const X0 = S.X0, *const row = S.row;

  for (uint32_t i = threadIdx.x; i < p.hist_len; i += blockDim.x) lhist[i] = 0u;
  for (uint32_t w = lane; w < W; w += 64u) HP[w] = p.byz_plane[w];
  __syncthreads();

  uint32_t h = 0u;                                 // honest nodes
  for (uint32_t j = 0; j < W; ++j) h += (uint32_t)__builtin_popcountll(HP[j]);
  h = uni(h);

  const Table tb{m, p.tally_off, p.tally_thr};     // the plan's one table

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
      uint32_t Hq = h - H0 - H1;                   // "?" starts: round 1 only
      PhaseC ph = phase_setup(row, p, tb, H0, H1, Hq + nb, lane);   // (reads the class sizes before P0 takes X0's words)
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t hp = uni64(HP[j]);
        uint64_t p0 = 0ull, p1 = 0ull;
        if (hp) {                                  // a group without an honest lane draws nothing
          const uint32_t c = j * 64u + lane;
          // the round's block of receiver c: u_R = out[1] << 32 | out[0], u_P = out[3] << 32 | out[2]
          const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
          uint32_t h0, h1;
          draw3(row, ph, m, q, k0, k1, tlo, thi, c, r, 0u, (uint64_t)b.y << 32 | b.x, h0, h1);
          const uint32_t rest = ((hp >> lane) & 1ull) ? q - h0 - h1 : 0u;   // (a Byzantine lane hears nothing)
          const uint32_t nB = Hq != 0u ? heard_byz(Hq, nb, rest, k0, k1, tlo, thi, c, r, 0u) : rest;
          const uint32_t l1 = heard_lies(strategy, c, h0, h1, nB);
          const uint32_t c0 = h0 + nB - l1, c1 = h1 + l1;
          rl.r(c0, c1, N, F, hp, p0, p1);
        }
        if (lane == 0) P0[j] = p0, P1[j] = p1;
      }
      // ---- P-phase ("voting phase", node.ts:83-158)
      __builtin_amdgcn_wave_barrier();
      H0 = 0, H1 = 0;
      for (uint32_t j = 0; j < W; ++j) {
        H0 += (uint32_t)__builtin_popcountll(P0[j]);   // proposals are honest nodes' only
        H1 += (uint32_t)__builtin_popcountll(P1[j]);
      }
      H0 = uni(H0), H1 = uni(H1);
      Hq = h - H0 - H1;
      ph = phase_setup(row, p, tb, H0, H1, Hq + nb, lane);
      bool undecided = false;
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t hp = uni64(HP[j]);
        if (!hp) continue;
        const uint32_t c = j * 64u + lane;
        const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
        const bool mine = (hp >> lane) & 1ull;     // this lane's node is honest
        uint32_t h0, h1;
        draw3(row, ph, m, q, k0, k1, tlo, thi, c, r, 1u, (uint64_t)b.w << 32 | b.z, h0, h1);
        const uint32_t rest = mine ? q - h0 - h1 : 0u;
        const uint32_t nB = Hq != 0u ? heard_byz(Hq, nb, rest, k0, k1, tlo, thi, c, r, 1u) : rest;
        const uint32_t l1 = heard_lies(strategy, c, h0, h1, nB);
        const uint32_t c0 = h0 + nB - l1, c1 = h1 + l1;
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

// The strategies whose liars see the receiver's inbox run the heard entry of the plan's rule; a
// BO_MODE_BYZ_RULE_B plan without a Byzantine node has no inbox to read and runs the other one.
bool byz_heard(const KParams &p) {
  return p.byz_n != 0u && (p.byz_strategy == BO_BYZ_BALANCE || p.byz_strategy == BO_BYZ_SPLIT);
}

// The b Binomial thresholds go into LDS, once per workgroup, when a CU then holds as many
// workgroups as without them: the fewer of what `lds_bytes` (histogram and the four waves'
// regions) allows and the six that the registers allow.
bool byz_thr_in_lds(uint32_t lds_bytes, uint32_t b) {
  const uint32_t without = lds_groups_per_cu(lds_bytes) < kByzWgPerCu ? lds_groups_per_cu(lds_bytes) : kByzWgPerCu;
  return lds_groups_per_cu(lds_bytes + 8u * b) >= without;
}

// The entry of a plan: its rule and coin by the variant, its loop by the strategy; a plan whose rule is replaced
// (rule_on, a Protocol B plan: the launch checks) takes the threshold rule's entry of its coin and loop.
using ByzKernel = void (*)(KParams);
static ByzKernel byz_entry(const KParams &p) {
  const bool heard = byz_heard(p);
  if (p.rule_on) {
    if (variant_shared_coin(p.variant))
      return heard ? benor_tally_heard_kernel<RuleT, CoinShared> : benor_tally_byz_kernel<RuleT, CoinShared>;
    return heard ? benor_tally_heard_kernel<RuleT, CoinLocal> : benor_tally_byz_kernel<RuleT, CoinLocal>;
  }
  switch (p.variant) {
    case byz_variant(BO_MODE_BYZ_TALLY): return heard ? benor_tally_heard_kernel<RuleRef, CoinLocal> : benor_tally_byz_kernel<RuleRef, CoinLocal>;
    case byz_variant(BO_MODE_BYZ_RULE_B): return heard ? benor_tally_heard_kernel<RuleB, CoinLocal> : benor_tally_byz_kernel<RuleB, CoinLocal>;
    case byz_variant(BO_MODE_BYZ_COIN): return heard ? benor_tally_heard_kernel<RuleRef, CoinShared> : benor_tally_byz_kernel<RuleRef, CoinShared>;
    case byz_variant(BO_MODE_BYZ_RULE_B_COIN): return heard ? benor_tally_heard_kernel<RuleB, CoinShared> : benor_tally_byz_kernel<RuleB, CoinShared>;
    default: return nullptr;
  }
}

// Workgroups of the kernel that one CU holds at once (registers and LDS; 0 = unknown).
int byz_blocks_per_cu(const KParams &p) { return variant_byz(p.variant) ? blocks_per_cu(byz_entry(p), p) : 0; }

// The Byzantine variants.  BO_MODE_BYZ_TALLY's alone needs a Byzantine node; the others run without one too (byz_n = 0:
// no thresholds, none in LDS).  The shared-coin ones need coin_common != 0 (0 is the parent mode's plan).
hipError_t launch_tally_byz(const KParams &plan, int grid, hipStream_t s) {
  const KParams p = state_launch(plan, byz_state_bytes(plan.W));
  const bool shared = variant_shared_coin(p.variant);
  const bool heard = byz_heard(p);                 // BO_BYZ_BALANCE, BO_BYZ_SPLIT: no thresholds, none in LDS
  const bool no_thr = heard || p.byz_n == 0u;
  if (!variant_byz(p.variant) || !p.tally_off || !p.tally_thr || !p.byz_plane || (no_thr ? p.byz_lds != 0u : !p.byz_thr) ||
      p.W > kMaxW || (p.byz_n == 0u && p.variant == byz_variant(BO_MODE_BYZ_TALLY)) || (shared && p.coin_common == 0u) ||
      (p.rule_on && (!variant_rule_b(p.variant) || rule::check(p.rule, nullptr) != BO_OK)) || p.byz_n > p.m - p.q || plan.wave_bytes < byz_wave_bytes(p.W, p.tally_cap) ||
      plan.lds_bytes < p.hist_bytes + kWavesPerBlock * plan.wave_bytes + (p.byz_lds ? 8u * p.byz_n : 0u))
    return hipErrorInvalidValue;
  return launch_lds(byz_entry(p), p, grid, s);
}

}  // namespace benor
