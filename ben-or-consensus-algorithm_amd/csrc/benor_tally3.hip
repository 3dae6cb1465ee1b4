// benor_tally3.hip -- three-valued count-level random delivery
// (BO_MODE_RANDOM_TALLY3 outside BO_MODE_RANDOM_TALLY's scope).
//
// The model is benor_tally.hip's: a receiver's inbox is a uniform q-subset of
// the m live senders, independent per (receiver, round, phase), and its rule
// reads only the counts.  Here a phase's votes fall into three classes -- K0
// zeros, K1 ones, Kq "?" -- so (c0, c1, c?) is multivariate hypergeometric over
// (K0, K1, Kq) with q draws.  It is drawn as one marginal and one conditional:
//
//   classes  S = the smallest class (ties: "?", then 0, then 1); A = the ones,
//            or the zeros when S is the ones; T = the third.
//   cA       = lo + #{ j : T[j] <= u } from row K_A of the HG(m, ., q) table,
//            u the phase's 64-bit uniform of the receiver-round's stream-5 block
//            -- benor_tally.hip's draw (with Kq = 0 it IS that draw).
//   cS       given cA the other q - cA slots are a uniform subset of the
//            m - K_A senders outside A: member i = 0..Ks-1 of S is in it with
//            probability (q - cA - taken) / (m - K_A - i) (selection sampling).
//            Ks and the denominators are wave-uniform, `taken` is per lane.
//            Each step draws an exact uniform integer below its denominator
//            (multiply-shift with rejection, as DStream::uniform) from the
//            receiver's word stream of Philox stream 6, words in order:
//              ctr = {trial_lo, trial_hi, c | block << 12,
//                     (r - 1) | phase << 16 | 6 << 24}.
//            Ks = 0 consumes none of it; m = q takes every member without a draw.
//   cT       = q - cA - cS.
//
// Only the class sizes of a phase enter the next one, so the trial's state is
// the x = 1 ballots and the sticky decided bits: after any P-phase x is binary,
// and the "?" of round 1 is the plan constant init_q (live "?" initial values).
// R-phase: c0 > c1 -> 0, c1 > c0 -> 1, else "?".  P-phase: c0 > F -> 0 decided,
// else c1 > F -> 1 decided, else the strict majority, else the node's coin
// (coin_ballot, compact index and round: the coin stream of every batch mode).
//
// One wave = one trial, lane l of receiver group j = live node 64 j + l.  The
// stream-5 block is regenerated in the P-phase instead of held per group, so
// the group loop is a runtime loop and the kernel has one form for every W.
// No floating point runs on the device.
#include "benor_tally_common.h"

namespace benor {

namespace {

__global__ void __launch_bounds__(256) benor_tally3_kernel(KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t m = p.m, F = p.F, W = p.W, q = p.q;

  uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);
  uint64_t *X1 = reinterpret_cast<uint64_t *>(smem + p.hist_bytes + wv * p.wave_bytes);   // [W] x = 1 ballots
  uint64_t *row = X1 + ((W + 1u) & ~1u);                                                  // [tally_cap] thresholds

  for (uint32_t i = threadIdx.x; i < p.hist_len; i += blockDim.x) lhist[i] = 0u;
  __syncthreads();

  uint64_t expect = 0ull;                          // groups holding a live receiver for this lane
  for (uint32_t j = 0; j < W; ++j)
    if (j * 64u + lane < m) expect |= 1ull << j;

  const uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32);
  const uint64_t waves_total = (uint64_t)gridDim.x * kWavesPerBlock;
  const Table tb{m, p.tally_off, p.tally_thr};     // the plan's one table

  for (uint64_t t = (uint64_t)blockIdx.x * kWavesPerBlock + wv; t < p.trial_count; t += waves_total) {
    const uint64_t trial = p.trial_begin + t;
    const uint32_t tlo = uni((uint32_t)trial), thi = uni((uint32_t)(trial >> 32));
    __builtin_amdgcn_wave_barrier();               // the previous trial's state reads are done
    trial_start<false>(X1, nullptr, p, k0, k1, trial, tlo, thi, lane);
    __builtin_amdgcn_wave_barrier();
    uint32_t K = 0;                                // live nodes with x = 1
    for (uint32_t j = 0; j < W; ++j) K += (uint32_t)__builtin_popcountll(X1[j]);
    K = uni(K);
    uint32_t Kq = p.init_mode == BO_INIT_FIXED ? p.init_q : 0u;   // live nodes with x = "?": round 1 only
    uint64_t dec = 0ull;
    uint32_t R = 0;
    bool all_dec = false;
    for (uint32_t r = 1; r <= p.k_max; ++r) {
      // ---- R-phase ("proposal phase", node.ts:46-82): only the proposals' class sizes go on
      PhaseC ph = phase_setup(row, p, tb, m - K - Kq, K, Kq, lane);
      uint32_t P0 = 0, P1 = 0;
      for (uint32_t j = 0; j < W; ++j) {
        const uint32_t c = j * 64u + lane;
        // the round's block of receiver c: u_R = out[1] << 32 | out[0], u_P = out[3] << 32 | out[2]
        const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
        uint32_t c0, c1;
        draw3(row, ph, m, q, k0, k1, tlo, thi, c, r, 0u, (uint64_t)b.y << 32 | b.x, c0, c1);
        P0 += (uint32_t)__builtin_popcountll(ballot(c < m && c0 > c1));
        P1 += (uint32_t)__builtin_popcountll(ballot(c < m && c1 > c0));
      }
      P0 = uni(P0), P1 = uni(P1);
      // ---- P-phase ("voting phase", node.ts:83-158)
      ph = phase_setup(row, p, tb, P0, P1, m - P0 - P1, lane);
      uint32_t Kn = 0;
      for (uint32_t j = 0; j < W; ++j) {
        const uint32_t c = j * 64u + lane;
        const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
        uint32_t c0, c1;
        draw3(row, ph, m, q, k0, k1, tlo, thi, c, r, 1u, (uint64_t)b.w << 32 | b.z, c0, c1);
        bool decided;
        const uint64_t x1 = p_rule(c0, c1, F, group_mask(j, m), k0, k1, tlo, thi, j, r, decided);
        if (lane == 0) X1[j] = x1;
        Kn += (uint32_t)__builtin_popcountll(x1);
        if (decided) dec |= 1ull << j;             // sticky
      }
      K = uni(Kn);
      Kq = 0u;
      R = r;
      all_dec = __all((dec & expect) == expect);
      if (all_dec) break;
    }
    __builtin_amdgcn_wave_barrier();
    trial_end(lhist, p, K, m, false, all_dec, R, lane);
    if (p.node_out) {
      for (uint32_t c = lane; c < m; c += 64u) {
        const uint32_t j = c >> 6;
        bo_node_state ns;
        ns.killed = 0;
        ns.x = (int8_t)((X1[j] >> lane) & 1ull);
        ns.decided = (int8_t)((dec >> j) & 1ull);
        ns.pad = 0;
        ns.k = (int32_t)R + 1;
        p.node_out[p.live_ids[c]] = ns;
      }
    }
  }

  __syncthreads();
  flush_hist(lhist, p);
}

}  // namespace

// Workgroups of the kernel that one CU holds at once (registers and LDS; 0 = unknown).
int tally3_blocks_per_cu(const KParams &p) { return blocks_per_cu(benor_tally3_kernel, p); }

hipError_t launch_tally3(const KParams &p, int grid, hipStream_t s) {
  if (!p.tally_off || !p.tally_thr || p.W > kMaxW || p.wave_bytes < tally_wave_bytes(p.W, p.tally_cap))
    return hipErrorInvalidValue;
  return launch_lds(benor_tally3_kernel, p, grid, s);
}

}  // namespace benor
