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
#include "benor_device.h"

namespace benor {

namespace {

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The wave-uniform part of a phase's draw.
struct Phase3 {
  uint32_t sel;      // 0: S = "?", A = 1, T = 0;  1: S = 0, A = 1, T = "?";  2: S = 1, A = 0, T = "?"
  uint32_t KA, KS;   // class sizes
  uint32_t lo;       // max(0, q - (m - KA)): row KA's least count
  uint32_t n, steps; // row KA staged in LDS: its width, and ceil(log2(n + 1))
};

__device__ __forceinline__ Phase3 phase_setup(uint64_t *__restrict__ row, const KParams &p, uint32_t K0, uint32_t K1,
                                              uint32_t Kq, uint32_t lane) {
  Phase3 ph;
  if (Kq <= K0 && Kq <= K1) ph.sel = 0u, ph.KS = Kq, ph.KA = K1;
  else if (K0 <= K1) ph.sel = 1u, ph.KS = K0, ph.KA = K1;
  else ph.sel = 2u, ph.KS = K1, ph.KA = K0;
  const uint32_t m = p.m, q = p.q, K = ph.KA;
  ph.lo = K + q > m ? K + q - m : 0u;
  ph.n = 0u, ph.steps = 0u;
  if (K != 0u && K != m && m != q) {               // else the row is a point
    __builtin_amdgcn_wave_barrier();               // the previous phase's searches are done with the region
    const uint32_t o = uni(p.tally_off[K]);
    uint32_t n = uni(p.tally_off[K + 1u]) - o;
    if (n > p.tally_cap) n = p.tally_cap;          // the region's size (the host table never exceeds it)
    const unsigned long long *src = p.tally_thr + o;
    for (uint32_t i = lane; i < n; i += 64u) row[i] = src[i];
    __builtin_amdgcn_wave_barrier();               // a wave's LDS operations retire in order
    ph.n = n;
    ph.steps = 32u - (uint32_t)__builtin_clz(n | 1u);
  }
  return ph;
}

// #{ j < n : T[j] <= u }: `steps` wave-uniform steps (benor_tally.hip row_count).
__device__ __forceinline__ uint32_t row_count(const uint64_t *__restrict__ row, uint32_t n, uint32_t steps,
                                              uint64_t u) {
  uint32_t pos = 0;
  for (uint32_t st = 1u << (steps - 1u); st != 0u; st >>= 1) {
    const uint32_t i = pos + st - 1u;
    const uint64_t t = row[i < n ? i : n - 1u];
    if (i < n && t <= u) pos += st;
  }
  return pos;
}

// Receiver c's counts (c0, c1) of the phase: u = its 64-bit uniform.
__device__ __forceinline__ void draw3(const uint64_t *__restrict__ row, const Phase3 &ph, uint32_t m, uint32_t q,
                                      uint32_t k0, uint32_t k1, uint32_t tlo, uint32_t thi, uint32_t c, uint32_t r,
                                      uint32_t phase, uint64_t u, uint32_t &c0, uint32_t &c1) {
  uint32_t cA = ph.lo;
  if (ph.n != 0u) cA += row_count(row, ph.n, ph.steps, u);
  uint32_t cS = 0u;
  if (ph.KS != 0u) {
    if (m == q) {
      cS = ph.KS;                                  // every live sender is in the inbox
    } else {
      const uint32_t slots = q - cA;               // inbox slots left to the senders outside A
      const uint32_t dtop = m - ph.KA;             // ... of which there are this many (>= slots, >= KS)
      const uint32_t c3 = (r - 1u) | (phase << 16) | (kStreamWalk << 24);
      // The wave steps through the word stream together, block by block; a
      // lane's member index i moves on with every word it accepts, so a lane
      // that rejects a word (probability < d / 2^32) falls one word behind
      // the others and the loop runs until the last lane is through.
      uint32_t i = 0;
      const auto word = [&](uint32_t w) {
        if (i < ph.KS) {
          const uint32_t d = dtop - i;             // member i's denominator, >= 1
          const uint64_t mm = (uint64_t)w * d;     // multiply-shift: the draw is the high word ...
          const uint32_t l = (uint32_t)mm;
          bool ok = true;
          if (l < d) ok = l >= (0u - d) % d;       // ... unless the low word falls in the biased remainder
          if (ok) {
            if ((uint32_t)(mm >> 32) < slots - cS) ++cS;
            ++i;
          }
        }
      };
      for (uint32_t blk = 0; __any(i < ph.KS); ++blk) {
        const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c | (blk << 12), c3));
        word(b.x), word(b.y), word(b.z), word(b.w);
      }
    }
  }
  const uint32_t cT = q - cA - cS;
  c1 = ph.sel == 2u ? cS : cA;
  c0 = ph.sel == 0u ? cT : (ph.sel == 1u ? cS : cA);
}

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

  for (uint64_t t = (uint64_t)blockIdx.x * kWavesPerBlock + wv; t < p.trial_count; t += waves_total) {
    const uint64_t trial = p.trial_begin + t;
    const uint32_t tlo = uni((uint32_t)trial), thi = uni((uint32_t)(trial >> 32));
    __builtin_amdgcn_wave_barrier();               // the previous trial's state reads are done
    if (p.init_mode == BO_INIT_RANDOM) {           // /start (node.ts:167-188): stream 1, as every batch mode
      const uint32_t nph = (W + 1u) >> 1;
      if (lane < nph) {
        uint4 r;
        if (m <= 32u) r = make_uint4(init_word_small(k0, k1, trial), 0u, 0u, 0u);   // shared block (m <= 32)
        else r = philox4x32_10(k0, k1, make_uint4(tlo, thi, lane, kStreamInit << 24));
        const uint32_t w0 = 2u * lane, w1 = w0 + 1u;
        X1[w0] = ((uint64_t)r.y << 32 | r.x) & group_mask(w0, m);
        if (w1 < W) X1[w1] = ((uint64_t)r.w << 32 | r.z) & group_mask(w1, m);
      }
    } else {
      for (uint32_t w = lane; w < W; w += 64u) {
        const uint4 rc = p.init_plane[w];
        X1[w] = (uint64_t)rc.w << 32 | rc.z;
      }
    }
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
      Phase3 ph = phase_setup(row, p, m - K - Kq, K, Kq, lane);
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
      ph = phase_setup(row, p, P0, P1, m - P0 - P1, lane);
      uint32_t Kn = 0;
      for (uint32_t j = 0; j < W; ++j) {
        const uint32_t c = j * 64u + lane;
        const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
        uint32_t c0, c1;
        draw3(row, ph, m, q, k0, k1, tlo, thi, c, r, 1u, (uint64_t)b.w << 32 | b.z, c0, c1);
        const uint64_t vm = group_mask(j, m);
        const bool d0l = c0 > F, d1l = !d0l && c1 > F;
        const uint64_t d0 = ballot(d0l) & vm;
        const uint64_t d1 = ballot(d1l) & vm;
        const uint64_t rest = vm & ~(d0 | d1);
        uint64_t x1 = d1;
        if (rest) {
          x1 |= ballot(c1 > c0) & rest;
          const uint64_t tie = ballot(c1 == c0) & rest;              // an empty tally included
          if (tie) x1 |= coin_ballot(k0, k1, tlo, thi, j, r, tie);
        }
        if (lane == 0) X1[j] = x1;
        Kn += (uint32_t)__builtin_popcountll(x1);
        if (d0l || d1l) dec |= 1ull << j;          // sticky
      }
      K = uni(Kn);
      Kq = 0u;
      R = r;
      all_dec = __all((dec & expect) == expect);
      if (all_dec) break;
    }
    __builtin_amdgcn_wave_barrier();
    const uint32_t v = (K != 0u && K != m) ? 2u : (K != 0u ? 1u : 0u);
    if (lane == 0) {
      atomicAdd(&lhist[all_dec ? (R * 3u + v) : v], 1u);
      if (all_dec && v == 2u) atomicAdd(&lhist[p.hist_len - 1u], 1u);
      if (p.rounds_out) *p.rounds_out = all_dec ? R : 0u;
    }
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
int tally3_blocks_per_cu(const KParams &p) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, benor_tally3_kernel, 64 * kWavesPerBlock,
                                                                    p.lds_bytes);
  return e == hipSuccess ? n : 0;
}

hipError_t launch_tally3(const KParams &p, int grid, hipStream_t s) {
  if (!p.tally_off || !p.tally_thr || p.W > kMaxW || p.wave_bytes < tally_wave_bytes(p.W, p.tally_cap))
    return hipErrorInvalidValue;
  if (p.lds_bytes > 64u * 1024u) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&benor_tally3_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(benor_tally3_kernel, dim3(grid), dim3(64 * kWavesPerBlock), p.lds_bytes, s, p);
  return hipGetLastError();
}

}  // namespace benor
