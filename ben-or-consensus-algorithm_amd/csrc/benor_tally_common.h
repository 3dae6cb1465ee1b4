// benor_tally_common.h -- what the count-level kernels share:
// benor_tally.hip, benor_tally3.hip, benor_tally_crash.hip, benor_tally_partial.hip,
// benor_tally_subset.hip, benor_tally_byz.hip (two kernels) and benor_tally_sched.hip.  Each piece stands
// here once: the per-wave LDS layouts, the threshold search, the three-class draw
// in its wave-uniform and its per-lane form, the stream-6 walk whose word order is
// the bit-exact contract with the oracle, a trial's start and end, the P-phase
// rule (and both phases of Ben-Or's Byzantine-tolerant rule, and the threshold rule
// of three runtime words over benor_rule.h), the per-node-state write-out, the random schedule, and the host's occupancy query and launch.
//
// The first part, the layouts, is plain C++ that also compiles on the host without
// HIP (tests/tally_layout_check.cpp sweeps it); the rest is device code.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BENOR_TALLY_HD __host__ __device__ inline
#else
#define BENOR_TALLY_HD inline
#endif

namespace benor {

constexpr uint32_t kSchedWords = 256u;             // stream-7 words drawn per pass (64 lanes, one block each)

// The per-wave LDS of the kernels that keep ballot planes: byte offsets from the
// wave's base, which is 16-byte aligned (KParams::hist_bytes and wave_bytes are
// multiples of 16).  The kernels take their pointers from it and the host its
// sizes, so the two cannot disagree.
//   AL   [W] u64   alive (crash family) or honest (Byzantine kernels: HP) nodes
//   X1   [W] u64   x = 1
//   P1   [W] u64   proposals 1; the schedule draw's chosen set
//   P0   [W] u64   proposals 0
//   X0   [W] u64   x = 0, read by round 1's class sizes only (after a P-phase every
//                  x is binary): P0's words, unless the launch keeps the plane for
//                  the crashed nodes' reports (own_x0: the crash family's state launch)
//   DEC  [W] u64   decided, a state launch only
//   row  [cap] u64 the staged row of thresholds
//   WB   [256] u32 a pass of stream-7 words, a random schedule only; written as
//                  uint4, so 16-byte aligned.  Inside `row` when that region holds
//                  them (2 capE >= 256: no row is staged while a schedule is drawn)
//   SC   [ncr] u32 the schedule
//   CL   [ncr] u32 the step's crasher list (partial, subset)
// W and cap are rounded up to even (WP, capE) and ncr to a multiple of 4, so every
// region starts on 8 bytes and row, WB, SC and CL on 16.
struct PlaneLayout {
  uint32_t AL, X1, P1, P0, X0, DEC, row, WB, SC, CL;
  uint32_t end;                                    // the wave's bytes
};

BENOR_TALLY_HD PlaneLayout plane_layout(uint32_t W, uint32_t cap, uint32_t ncr, bool random, bool states, bool own_x0,
                                        bool cl) {
  const uint32_t WP = ((W + 1u) & ~1u) * 8u, capE = ((cap + 1u) & ~1u) * 8u, list = ((ncr + 3u) & ~3u) * 4u;
  const bool wb_in_row = capE >= kSchedWords * 4u;
  PlaneLayout L;
  L.AL = 0u;
  L.X1 = L.AL + WP;
  L.P1 = L.X1 + WP;
  L.P0 = L.P1 + WP;
  L.X0 = own_x0 ? L.P0 + WP : L.P0;
  L.DEC = L.X0 + WP;
  L.row = states ? L.DEC + WP : L.P0 + WP;
  L.WB = wb_in_row ? L.row : L.row + capE;
  L.SC = L.row + capE + (random && !wb_in_row ? kSchedWords * 4u : 0u);
  L.CL = L.SC + list;
  L.end = cl ? L.CL + list : L.CL;
  return L;
}

// The crash family (benor_tally_crash.hip; with the crasher list benor_tally_partial.hip
// and benor_tally_subset.hip).  A batch launch holds four planes, which at N = 4096 keeps
// three workgroups on a CU as benor_tally3.hip has; a state launch adds X0 and DEC.
BENOR_TALLY_HD PlaneLayout crash_layout(uint32_t W, uint32_t cap, uint32_t ncr, bool random, bool states, bool cl) {
  return plane_layout(W, cap, ncr, random, states, states, cl);
}
// The Byzantine kernels (benor_tally_byz.hip): no schedule, and a Byzantine node's
// state is the host's to report, so a state launch adds DEC alone.
BENOR_TALLY_HD PlaneLayout byz_layout(uint32_t W, uint32_t cap, bool states) {
  return plane_layout(W, cap, 0u, false, states, false, false);
}

// A batch launch's per-wave bytes, and what a per-node-state launch (one trial) adds.
BENOR_TALLY_HD uint32_t crash_wave_bytes(uint32_t W, uint32_t cap, uint32_t ncr, bool random, bool cl) {
  return crash_layout(W, cap, ncr, random, false, cl).end;
}
BENOR_TALLY_HD uint32_t crash_state_bytes(uint32_t W) {
  return crash_layout(W, 0u, 0u, false, true, false).end - crash_layout(W, 0u, 0u, false, false, false).end;
}
BENOR_TALLY_HD uint32_t byz_wave_bytes(uint32_t W, uint32_t cap) { return byz_layout(W, cap, false).end; }
BENOR_TALLY_HD uint32_t byz_state_bytes(uint32_t W) { return byz_layout(W, 0u, true).end - byz_layout(W, 0u, false).end; }
// benor_tally.hip and benor_tally3.hip: the x = 1 plane and the row.
BENOR_TALLY_HD uint32_t tally_wave_bytes(uint32_t W, uint32_t cap) { return (((W + 1u) & ~1u) + cap) * 8u; }

}  // namespace benor

#if defined(__HIPCC__) || defined(__CUDACC__)

#include <type_traits>

#include "benor_device.h"
#include "benor_rule.h"

namespace benor {

namespace {

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return (uint64_t)uni((uint32_t)(v >> 32)) << 32 | uni((uint32_t)v); }

constexpr uint32_t kStepClamp = 0xFFFFFu;          // schedule entries: step in 20 bits, compact index in 12

// ---- the threshold search
// #{ j < n : T[j] <= u } for ascending T[0..n), n >= 1, in LDS or in global memory:
// `steps` halving steps from 2^(steps - 1), no divergent loop.  Any steps >=
// search_steps(n) gives the same count, since a probe at or beyond n fails: a call
// site may derive it from n or from any bound on n, such as the plan's tally_cap;
// both are the same function of (T, n, u).  What a failing probe reads is the one
// choice left to the call site.  In LDS it reads T[n - 1] (CLAMP): one ds_read_b64
// per step and no branch.  In global memory it reads nothing: the lanes of a group
// search rows of their own, far apart when their pools differ (mode 7), and a read
// of the row's end would cost each a cache line it does not need.
__device__ __forceinline__ uint32_t search_steps(uint32_t n) { return 32u - (uint32_t)__builtin_clz(n | 1u); }

template <bool CLAMP = true, class T>
__device__ __forceinline__ uint32_t count_le(const T *__restrict__ row, uint32_t n, uint32_t steps, uint64_t u) {
  uint32_t pos = 0;
  for (uint32_t st = 1u << (steps - 1u); st != 0u; st >>= 1) {
    const uint32_t i = pos + st - 1u;
    if constexpr (CLAMP) {
      const uint64_t t = row[i < n ? i : n - 1u];
      if (i < n && t <= u) pos += st;
    } else {
      if (i < n && row[i] <= u) pos += st;
    }
  }
  return pos;
}

// ---- the class choice
// A phase's votes fall into three classes, K0 zeros, K1 ones, Kq "?".  S = the
// smallest class (ties: "?", then 0, then 1), walked from stream 6; A = the ones, or
// the zeros when S is the ones, counted from row KA of the table; T = the third.
struct Classes {
  uint32_t sel;      // 0: S = "?", A = 1, T = 0;  1: S = 0, A = 1, T = "?";  2: S = 1, A = 0, T = "?"
  uint32_t KA, KS;   // class sizes
};

__device__ __forceinline__ Classes choose_classes(uint32_t K0, uint32_t K1, uint32_t Kq) {
  Classes cl;
  if (Kq <= K0 && Kq <= K1) cl.sel = 0u, cl.KS = Kq, cl.KA = K1;
  else if (K0 <= K1) cl.sel = 1u, cl.KS = K0, cl.KA = K1;
  else cl.sel = 2u, cl.KS = K1, cl.KA = K0;
  return cl;
}

// (c0, c1) from the counts of A and S among the q messages.
__device__ __forceinline__ void class_counts(uint32_t sel, uint32_t q, uint32_t cA, uint32_t cS, uint32_t &c0,
                                             uint32_t &c1) {
  const uint32_t cT = q - cA - cS;
  c1 = sel == 2u ? cS : cA;
  c0 = sel == 0u ? cT : (sel == 1u ? cS : cA);
}

// ---- the selection-sampling walk
// One word of a walk: member i of the walked class is in the inbox with probability
// (slots - taken) / (dtop - i).  The word gives an exact uniform integer below the
// denominator (multiply-shift with rejection, as DStream::uniform); a rejected word
// leaves i where it is, so the next word serves the same member.
__device__ __forceinline__ void walk_word(uint32_t w, uint32_t KS, uint32_t dtop, uint32_t slots, uint32_t &i,
                                          uint32_t &cS) {
  if (i < KS) {
    const uint32_t d = dtop - i;                   // member i's denominator, >= 1
    const uint64_t mm = (uint64_t)w * d;           // multiply-shift: the draw is the high word ...
    const uint32_t l = (uint32_t)mm;
    bool ok = true;
    // ... unless the low word falls in the biased remainder (probability < d / 2^32: marked unlikely, which
    // keeps the division out of the walk's loop body)
    if (__builtin_expect(l < d, 0)) ok = l >= (0u - d) % d;
    if (ok) {
      if ((uint32_t)(mm >> 32) < slots - cS) ++cS;
      ++i;
    }
  }
}

// cS: how many of the KS members of S are among receiver c's q messages from m
// senders, given cA of class A's KA.  The other q - cA slots are a uniform subset of
// the m - KA senders outside A, walked from the receiver's word stream of Philox
// stream 6, blocks {trial_lo, trial_hi, c | blk << 12, (r - 1) | phase << 16 | 6 << 24},
// blk = 0, 1, .., words x, y, z, w in order.  KS = 0 consumes none of it; m = q takes
// every member without a draw.  Every quantity may be wave-uniform or the lane's own.
__device__ __forceinline__ uint32_t walk6(uint32_t m, uint32_t q, uint32_t KA, uint32_t KS, uint32_t cA, uint32_t k0,
                                          uint32_t k1, uint32_t tlo, uint32_t thi, uint32_t c, uint32_t r,
                                          uint32_t phase) {
  uint32_t cS = 0u;
  if (m == q) {
    cS = KS;                                       // every sender is in the inbox
  } else {
    const uint32_t slots = q - cA;                 // inbox slots left to the senders outside A
    const uint32_t dtop = m - KA;                  // ... of which there are this many (>= slots, >= KS)
    const uint32_t c3 = (r - 1u) | (phase << 16) | (kStreamWalk << 24);
    // The wave steps through the word stream together, block by block; a
    // lane's member index i moves on with every word it accepts, so a lane
    // that rejects a word (probability < d / 2^32) falls one word behind
    // the others and the loop runs until the last lane is through.
    uint32_t i = 0;
    for (uint32_t blk = 0; __any(i < KS); ++blk) {
      const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c | (blk << 12), c3));
      walk_word(b.x, KS, dtop, slots, i, cS), walk_word(b.y, KS, dtop, slots, i, cS);
      walk_word(b.z, KS, dtop, slots, i, cS), walk_word(b.w, KS, dtop, slots, i, cS);
    }
  }
  return cS;
}

// ---- the three-class draw, wave-uniform form
// The table HG(m, ., q) of a pool of m senders: row K is thr[off[K] .. off[K + 1]).
struct Table {
  uint32_t m;
  const uint32_t *off;                             // [m + 2] row offsets
  const unsigned long long *thr;
};

// Entry m0 - m of the crash family's directory: the table of a pool of m <= m0 nodes.
__device__ __forceinline__ Table dir_table(const KParams &p, uint32_t m) {
  const CrashDir de = p.cr_dir[p.m - m];           // p.m - m <= cr_n crashes so far
  Table tb;
  tb.m = m;
  tb.off = p.tally_off + uni(de.off_base);
  tb.thr = p.tally_thr + uni64(de.thr_base);
  return tb;
}

// The wave-uniform part of a phase's draw.
struct PhaseC {
  uint32_t sel, KA, KS;   // the class choice
  uint32_t lo;            // max(0, q - (m - KA)): row KA's least count
  uint32_t n, steps;      // row KA staged in LDS: its width (0: a point), and search_steps(n)
};

__device__ __forceinline__ PhaseC phase_none() {
  PhaseC ph;
  ph.sel = 0u, ph.KA = 0u, ph.KS = 0u, ph.lo = 0u, ph.n = 0u, ph.steps = 0u;
  return ph;
}

// Row K of the table into the wave's LDS region; returns its width (<= cap).
__device__ __forceinline__ uint32_t stage_row(uint64_t *__restrict__ row, const uint32_t *off,
                                              const unsigned long long *thr, uint32_t cap, uint32_t K, uint32_t lane) {
  const uint32_t o = uni(off[K]);
  uint32_t n = uni(off[K + 1u]) - o;
  if (n > cap) n = cap;                            // the region's size (no row of any table exceeds it)
  const unsigned long long *src = thr + o;
  for (uint32_t i = lane; i < n; i += 64u) row[i] = src[i];
  __builtin_amdgcn_wave_barrier();                 // a wave's LDS operations retire in order
  return n;
}

__device__ __forceinline__ PhaseC phase_setup(uint64_t *__restrict__ row, const KParams &p, const Table &tb, uint32_t K0,
                                              uint32_t K1, uint32_t Kq, uint32_t lane) {
  const Classes cl = choose_classes(K0, K1, Kq);
  PhaseC ph;
  ph.sel = cl.sel, ph.KA = cl.KA, ph.KS = cl.KS;
  const uint32_t m = tb.m, q = p.q, K = ph.KA;
  ph.lo = K + q > m ? K + q - m : 0u;
  ph.n = 0u, ph.steps = 0u;
  if (K != 0u && K != m && m != q) {               // else the row is a point
    __builtin_amdgcn_wave_barrier();               // the previous phase's searches are done with the region
    ph.n = stage_row(row, tb.off, tb.thr, p.tally_cap, K, lane);
    ph.steps = search_steps(ph.n);
  }
  return ph;
}

// Receiver c's counts (c0, c1) of the phase among m senders, u its 64-bit uniform:
// cA = lo + #{ j : T[j] <= u } from the staged row (with Kq = 0 it IS benor_tally.hip's
// draw), cS walked, cT the rest.
__device__ __forceinline__ void draw3(const uint64_t *__restrict__ row, const PhaseC &ph, uint32_t m, uint32_t q,
                                      uint32_t k0, uint32_t k1, uint32_t tlo, uint32_t thi, uint32_t c, uint32_t r,
                                      uint32_t phase, uint64_t u, uint32_t &c0, uint32_t &c1) {
  uint32_t cA = ph.lo;
  if (ph.n != 0u) cA += count_le(row, ph.n, ph.steps, u);
  uint32_t cS = 0u;
  if (ph.KS != 0u) cS = walk6(m, q, ph.KA, ph.KS, cA, k0, k1, tlo, thi, c, r, phase);
  class_counts(ph.sel, q, cA, cS, c0, c1);
}

// ---- the three-class draw, per-lane form
// draw3 for a lane whose pool or class sizes are its own: the same class choice,
// count and walk with every quantity per lane, the row searched where it lies in
// global memory.  m is the lane's pool size, (K0, K1) its class sizes, K0 + K1 <= m;
// table_of(m) gives the lane's table and is called only where a row is searched.
// `steps`: a wave-uniform count of search steps that serves every row (search_steps
// of the plan's cap), or 0 for the lane's own search_steps(width); each kernel keeps
// the form it was measured with.  A lane that is not `active` loads nothing and its
// result is not used.
template <class TableOf>
__device__ __forceinline__ void draw3_lane(const TableOf &table_of, uint32_t cap, uint32_t steps, uint32_t m, uint32_t q,
                                           uint32_t K0, uint32_t K1, uint32_t k0, uint32_t k1, uint32_t tlo,
                                           uint32_t thi, uint32_t c, uint32_t r, uint32_t phase, uint64_t u, bool active,
                                           uint32_t &c0, uint32_t &c1) {
  const Classes cl = choose_classes(K0, K1, m - K0 - K1);
  const uint32_t KA = cl.KA;
  uint32_t cA = KA + q > m ? KA + q - m : 0u;
  if (active && KA != 0u && KA != m && m != q) {   // else the row is a point
    const Table tb = table_of(m);
    const uint32_t o = tb.off[KA];
    uint32_t n = tb.off[KA + 1u] - o;
    if (n > cap) n = cap;
    cA += count_le<false>(tb.thr + o, n, steps ? steps : search_steps(n), u);   // (n = 0: every probe fails)
  }
  const uint32_t cS = walk6(m, q, KA, active ? cl.KS : 0u, cA, k0, k1, tlo, thi, c, r, phase);
  class_counts(cl.sel, q, cA, cS, c0, c1);
}

// ---- a trial's start and end
// /start (node.ts:167-188): the initial values into X1, and into X0 when the caller
// has that plane.  Random ones from stream 1, as every batch mode: lane l draws the
// block of groups 2 l and 2 l + 1 (m <= 32: the shared block); fixed ones from the
// plan's init_plane.
template <bool HAS_X0>
__device__ __forceinline__ void trial_start(uint64_t *__restrict__ X1, uint64_t *__restrict__ X0, const KParams &p,
                                            uint32_t k0, uint32_t k1, uint64_t trial, uint32_t tlo, uint32_t thi,
                                            uint32_t lane) {
  const uint32_t m = p.m, W = p.W;
  if (p.init_mode == BO_INIT_RANDOM) {
    const uint32_t nph = (W + 1u) >> 1;
    if (lane < nph) {
      uint4 r;
      if (m <= 32u) r = make_uint4(init_word_small(k0, k1, trial), 0u, 0u, 0u);   // shared block (m <= 32)
      else r = philox4x32_10(k0, k1, make_uint4(tlo, thi, lane, kStreamInit << 24));
      const uint32_t w0 = 2u * lane, w1 = w0 + 1u;
      const uint64_t g0 = group_mask(w0, m), a0 = ((uint64_t)r.y << 32 | r.x) & g0;
      X1[w0] = a0;
      if constexpr (HAS_X0) X0[w0] = g0 & ~a0;
      if (w1 < W) {
        const uint64_t g1 = group_mask(w1, m), a1 = ((uint64_t)r.w << 32 | r.z) & g1;
        X1[w1] = a1;
        if constexpr (HAS_X0) X0[w1] = g1 & ~a1;
      }
    }
  } else {
    for (uint32_t w = lane; w < W; w += 64u) {
      const uint4 rc = p.init_plane[w];
      if constexpr (HAS_X0) X0[w] = (uint64_t)rc.y << 32 | rc.x;
      X1[w] = (uint64_t)rc.w << 32 | rc.z;
    }
  }
}

// The trial's outcome into the workgroup's histogram: K of the `live` nodes that
// count at the end hold x = 1; v = 0 / 1 if they agree, 2 if not or if `none` is
// left (then bin[2], rounds 0).  Bin R * 3 + v if all decided in round R, else
// bin v; the last bin counts the trials that decided without agreeing.
__device__ __forceinline__ void trial_end(uint32_t *lhist, const KParams &p, uint32_t K, uint32_t live, bool none,
                                          bool all_dec, uint32_t R, uint32_t lane) {
  const uint32_t v = none ? 2u : ((K != 0u && K != live) ? 2u : (K != 0u ? 1u : 0u));
  if (none) all_dec = false;
  if (lane == 0) {
    atomicAdd(&lhist[all_dec ? (R * 3u + v) : v], 1u);
    if (all_dec && v == 2u) atomicAdd(&lhist[p.hist_len - 1u], 1u);
    if (p.rounds_out) *p.rounds_out = all_dec ? R : 0u;
  }
}

// ---- the coin a P-phase rule takes, a compile-time policy of the trial loop
// operator() returns the x = 1 bits of the lanes of `take` (wave-uniform, not empty) in group j.
struct CoinLocal {                                 // every node its own: coin_ballot, the coin stream of every batch mode
  static constexpr bool kShared = false;
  __device__ __forceinline__ void round_start() {}
  __device__ __forceinline__ uint64_t operator()(uint32_t k0, uint32_t k1, uint32_t tlo, uint32_t thi, uint32_t j,
                                                 uint32_t r, uint64_t take) const {
    return coin_ballot(k0, k1, tlo, thi, j, r, take);
  }
};
// A shared coin (BO_MODE_BYZ_COIN, BO_MODE_BYZ_RULE_B_COIN; `common` = KParams::coin_common != 0).  One wave is
// one trial, so the round's stream-12 block is wave-uniform: it is drawn when a group of the round first
// takes a coin and kept as two bits.  A common round runs no per-lane coin block at all.
struct CoinShared {
  static constexpr bool kShared = true;
  uint32_t common;
  uint32_t st;                                     // this round: 0 not drawn yet, 1 each node its own coin, 2 | v common with value v
  __device__ __forceinline__ void round_start() { st = 0u; }
  __device__ __forceinline__ uint64_t operator()(uint32_t k0, uint32_t k1, uint32_t tlo, uint32_t thi, uint32_t j,
                                                 uint32_t r, uint64_t take) {
    if (st == 0u) {
      const uint2 w = common_coin(k0, k1, tlo, thi, r);
      st = (common == 0xFFFFFFFFu || w.x < common) ? 2u | (w.y & 1u) : 1u;
    }
    if (st & 2u) return (st & 1u) ? take : 0ull;
    return coin_ballot(k0, k1, tlo, thi, j, r, take);
  }
};

// ---- the P-phase rule ("voting phase", node.ts:83-158) for receiver group j
// c0 > F -> 0 decided, else c1 > F -> 1 decided, else the strict majority, else the
// node's coin (coin_ballot, compact index and round: the coin stream of every batch
// mode).  `mask` holds the group's lanes that vote; returns their new x = 1 bits,
// and in `decided` whether this lane's counts decide (sticky in the caller, which
// also applies its own mask to it).  `coin` is the trial loop's coin policy; without one, CoinLocal.
template <class Coin>
__device__ __forceinline__ uint64_t p_rule(uint32_t c0, uint32_t c1, uint32_t F, uint64_t mask, uint32_t k0, uint32_t k1,
                                           uint32_t tlo, uint32_t thi, uint32_t j, uint32_t r, bool &decided, Coin &coin) {
  const bool d0l = c0 > F, d1l = !d0l && c1 > F;
  const uint64_t d0 = ballot(d0l) & mask;
  const uint64_t d1 = ballot(d1l) & mask;
  const uint64_t rest = mask & ~(d0 | d1);
  uint64_t x1 = d1;
  if (rest) {
    x1 |= ballot(c1 > c0) & rest;
    const uint64_t tie = ballot(c1 == c0) & rest;  // an empty tally included
    if (tie) x1 |= coin(k0, k1, tlo, thi, j, r, tie);
  }
  decided = d0l || d1l;
  return x1;
}
__device__ __forceinline__ uint64_t p_rule(uint32_t c0, uint32_t c1, uint32_t F, uint64_t mask, uint32_t k0, uint32_t k1,
                                           uint32_t tlo, uint32_t thi, uint32_t j, uint32_t r, bool &decided) {
  CoinLocal coin;
  return p_rule(c0, c1, F, mask, k0, k1, tlo, thi, j, r, decided, coin);
}

// ---- Ben-Or's Byzantine-tolerant rule (Protocol B, N > 5t with t = F; BO_MODE_BYZ_RULE_B)
// The R-phase: propose v iff more than (N + F) / 2 of the messages heard carry v, else
// "?" (neither ballot).  Both cannot hold: c0 + c1 <= N - F.
__device__ __forceinline__ void r_rule_b(uint32_t c0, uint32_t c1, uint32_t N, uint32_t F, uint64_t mask, uint64_t &p0,
                                         uint64_t &p1) {
  p0 = ballot(2u * c0 > N + F) & mask;
  p1 = ballot(2u * c1 > N + F) & mask;
}

// The P-phase, p_rule's interface: v = the value with the strictly larger count (none on
// c0 == c1, an empty tally included); with c_v > F the node adopts v, and decides iff
// 2 c_v > N + F; otherwise x is the node's coin (coin_ballot, the coin stream of every batch
// mode; or the trial loop's coin policy).  Ballots and integer compares only; counts are at most N <= 4096.
template <class Coin>
__device__ __forceinline__ uint64_t p_rule_b(uint32_t c0, uint32_t c1, uint32_t N, uint32_t F, uint64_t mask, uint32_t k0,
                                             uint32_t k1, uint32_t tlo, uint32_t thi, uint32_t j, uint32_t r,
                                             bool &decided, Coin &coin) {
  const uint32_t cv = c1 > c0 ? c1 : c0;
  const bool adopt = c0 != c1 && cv > F;
  const uint64_t take = mask & ~ballot(adopt);
  uint64_t x1 = ballot(adopt && c1 > c0) & mask;
  if (take) x1 |= coin(k0, k1, tlo, thi, j, r, take);
  decided = adopt && 2u * cv > N + F;
  return x1;
}

// ---- the rule as a compile-time policy of the Byzantine and the scheduler trial loops
// (benor_tally_byz.hip, benor_tally_sched.hip)
// The rule a receiver applies to its counts (c0, c1), the one thing in which BO_MODE_BYZ_TALLY and
// BO_MODE_BYZ_RULE_B differ: the R-phase's proposal ballots of a group and the P-phase rule.
// kNoLiar: the mode runs its kernel without a Byzantine node too (byz_n = 0: every step wave-uniform
// with B1 = 0, no threshold read).
struct RuleRef {                                   // the reference's crash-tolerant rule (node.ts:46-158)
  static constexpr bool kNoLiar = false;           // (b = 0 is mode 4's plan; with a shared coin it is not, and runs here)
  static __device__ __forceinline__ void r(uint32_t c0, uint32_t c1, uint32_t, uint32_t, uint64_t hp, uint64_t &p0,
                                           uint64_t &p1) {
    p0 = ballot(c0 > c1) & hp;
    p1 = ballot(c1 > c0) & hp;
  }
  template <class Coin>
  static __device__ __forceinline__ uint64_t p(uint32_t c0, uint32_t c1, uint32_t, uint32_t F, uint64_t hp, uint32_t k0,
                                               uint32_t k1, uint32_t tlo, uint32_t thi, uint32_t j, uint32_t r,
                                               bool &decided, Coin &coin) {
    return p_rule(c0, c1, F, hp, k0, k1, tlo, thi, j, r, decided, coin);
  }
};
struct RuleB {                                     // Ben-Or's Protocol B, t = F
  static constexpr bool kNoLiar = true;
  static __device__ __forceinline__ void r(uint32_t c0, uint32_t c1, uint32_t N, uint32_t F, uint64_t hp, uint64_t &p0,
                                           uint64_t &p1) {
    r_rule_b(c0, c1, N, F, hp, p0, p1);
  }
  template <class Coin>
  static __device__ __forceinline__ uint64_t p(uint32_t c0, uint32_t c1, uint32_t N, uint32_t F, uint64_t hp, uint32_t k0,
                                               uint32_t k1, uint32_t tlo, uint32_t thi, uint32_t j, uint32_t r,
                                               bool &decided, Coin &coin) {
    return p_rule_b(c0, c1, N, F, hp, k0, k1, tlo, thi, j, r, decided, coin);
  }
};

// A threshold rule of three runtime words (bo_rule, benor_rule.h): Protocol A, and Protocol B and
// the reference's rule again at their words.  The words are KParams::rule's, wave-uniform; the rule itself is
// benor_rule.h's scalar R- and P-step, wrapped in ballots.  An interface of its own -- an object with the words,
// made by make_rule -- so that the two compile-time rules above keep theirs and their entries their code.
struct RuleT {
  static constexpr bool kNoLiar = true;            // a Protocol B plan with its rule replaced: b = 0 runs here too
  bo_rule t;
  __device__ __forceinline__ void r(uint32_t c0, uint32_t c1, uint32_t, uint32_t, uint64_t hp, uint64_t &p0,
                                    uint64_t &p1) const {
    const uint32_t prop = rule::r_step(t, c0, c1);
    p0 = ballot(prop == 0u) & hp;
    p1 = ballot(prop == 1u) & hp;
  }
  template <class Coin>
  __device__ __forceinline__ uint64_t p(uint32_t c0, uint32_t c1, uint32_t, uint32_t, uint64_t mask, uint32_t k0,
                                        uint32_t k1, uint32_t tlo, uint32_t thi, uint32_t j, uint32_t r, bool &decided,
                                        Coin &coin) const {
    const uint32_t act = rule::p_step(t, c0, c1, decided);
    const uint64_t take = mask & ballot(act == rule::kNone);
    uint64_t x1 = ballot(act == 1u) & mask;
    if (take) x1 |= coin(k0, k1, tlo, thi, j, r, take);
    return x1;
  }
};

// The rule object of a trial loop: empty for the compile-time rules (their r and p are static), the plan's words for RuleT.
template <class Rule>
__device__ __forceinline__ Rule make_rule(const KParams &p) {
  if constexpr (std::is_same_v<Rule, RuleT>)
    return Rule{bo_rule{uni(p.rule.propose_gt2), uni(p.rule.adopt_gt), uni(p.rule.decide_gt2), 0u}};
  else
    return Rule{};
}

template <class Coin>
__device__ __forceinline__ Coin make_coin(const KParams &p) {
  if constexpr (Coin::kShared) return Coin{p.coin_common, 0u};
  else return Coin{};
}

// ---- the per-node-state write-out of a state launch (one trial)
// The lanes' decided bits (bit j of `dec`: node 64 j + lane) go into the DEC plane;
// then the nodes of the AL plane (alive, or honest) report x, decided and k = R + 1.
// CRASHED: the crashed nodes of the schedule SC[0..ncr) report x and decided as of
// their crash -- a bit of a crashed node is never written again -- and k its round;
// the Byzantine kernels pass their honest plane and skip this (a Byzantine node is
// alive with no protocol state: the host's entry stays).
template <bool CRASHED>
__device__ __forceinline__ void write_states(const KParams &p, const uint64_t *AL, const uint64_t *X1, const uint64_t *X0,
                                             uint64_t *DEC, const uint32_t *SC, uint32_t ncr, uint64_t dec, uint32_t R,
                                             uint32_t lane) {
  for (uint32_t j = 0; j < p.W; ++j) {
    const uint64_t d = ballot((dec >> j) & 1ull);
    if (lane == 0) DEC[j] = d;
  }
  __builtin_amdgcn_wave_barrier();
  for (uint32_t c = lane; c < p.m; c += 64u) {
    const uint32_t j = c >> 6;
    if (!((AL[j] >> lane) & 1ull)) continue;
    bo_node_state ns;
    ns.killed = 0;
    ns.x = (int8_t)((X1[j] >> lane) & 1ull);
    ns.decided = (int8_t)((DEC[j] >> lane) & 1ull);
    ns.pad = 0;
    ns.k = (int32_t)R + 1;
    p.node_out[p.live_ids[c]] = ns;
  }
  if constexpr (CRASHED) {
    for (uint32_t i = lane; i < ncr; i += 64u) {
      const uint32_t e = SC[i], c = e & 0xFFFu, j = c >> 6, b = c & 63u;
      if ((AL[j] >> b) & 1ull) continue;           // its step was never reached
      bo_node_state ns;
      ns.killed = 1;
      ns.x = (int8_t)(((X1[j] >> b) & 1ull) ? 1 : (((X0[j] >> b) & 1ull) ? 0 : 2));
      ns.decided = (int8_t)((DEC[j] >> b) & 1ull);
      ns.pad = 0;
      ns.k = (int32_t)(e >> 13) + 1;
      p.node_out[p.live_ids[c]] = ns;
    }
  }
}

// ---- the crash family's schedule
// The trial's random schedule: Floyd's algorithm over the compact indices, from
// the word stream of Philox stream 7, blocks {trial_lo, trial_hi, b, 7 << 24},
// b = 0, 1, ..  For j = m0 - n .. m0 - 1: t uniform below j + 1, the node is t
// unless already chosen, then j; its step uniform below the window.  The wave
// draws 64 blocks at a time into WB, lane 0 consumes the words in order (a
// rejected word draws the next one for the same denominator); `chosen` is a
// zeroed plane of W words.
__device__ __forceinline__ void draw_schedule(uint32_t *__restrict__ SC, uint32_t *__restrict__ WB,
                                              uint64_t *__restrict__ chosen, const KParams &p, uint32_t k0, uint32_t k1,
                                              uint32_t tlo, uint32_t thi, uint32_t lane) {
  const uint32_t m0 = p.m, window = p.crash_window;
  uint32_t j = m0 - p.cr_n, i = 0u, have = 0u, node = 0u;   // lane 0's walk
  for (uint32_t base = 0u;; base += 64u) {
    const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, base + lane, kStreamSchedule << 24));
    __builtin_amdgcn_wave_barrier();               // the previous pass's words are consumed
    reinterpret_cast<uint4 *>(WB)[lane] = b;
    __builtin_amdgcn_wave_barrier();
    if (lane == 0u) {
      for (uint32_t w = 0u; w < kSchedWords && j < m0; ++w) {
        const uint32_t d = have ? window : j + 1u;
        const uint64_t mm = (uint64_t)WB[w] * d;
        const uint32_t l = (uint32_t)mm;
        if (l < d && l < (0u - d) % d) continue;   // the biased remainder: the next word, same denominator
        uint32_t v = (uint32_t)(mm >> 32);
        if (!have) {
          if ((chosen[v >> 6] >> (v & 63u)) & 1ull) v = j;
          chosen[v >> 6] |= 1ull << (v & 63u);
          node = v;
          have = 1u;
        } else {
          SC[i++] = (v < kStepClamp ? v : kStepClamp) << 12 | node;
          have = 0u;
          ++j;
        }
      }
    }
    if (uni(j) >= m0) break;
  }
  __builtin_amdgcn_wave_barrier();
}

// The planes of a PlaneLayout at a wave's base.
struct Planes {
  uint64_t *AL, *X1, *P1, *P0, *X0, *DEC, *row;
  uint32_t *WB, *SC, *CL;
  __device__ __forceinline__ Planes(unsigned char *base, const PlaneLayout &L)
      : AL(reinterpret_cast<uint64_t *>(base + L.AL)), X1(reinterpret_cast<uint64_t *>(base + L.X1)),
        P1(reinterpret_cast<uint64_t *>(base + L.P1)), P0(reinterpret_cast<uint64_t *>(base + L.P0)),
        X0(reinterpret_cast<uint64_t *>(base + L.X0)), DEC(reinterpret_cast<uint64_t *>(base + L.DEC)),
        row(reinterpret_cast<uint64_t *>(base + L.row)), WB(reinterpret_cast<uint32_t *>(base + L.WB)),
        SC(reinterpret_cast<uint32_t *>(base + L.SC)), CL(reinterpret_cast<uint32_t *>(base + L.CL)) {}
};

// The crash family's trial start: every node alive, the initial values, and a random
// schedule drawn (P1, zeroed, is its chosen set).
__device__ __forceinline__ void crash_trial_start(const Planes &S, const KParams &p, uint32_t k0, uint32_t k1,
                                                  uint64_t trial, uint32_t tlo, uint32_t thi, uint32_t lane) {
  if (lane < p.W) {
    S.AL[lane] = group_mask(lane, p.m);
    S.P1[lane] = 0ull;
  }
  trial_start<true>(S.X1, S.X0, p, k0, k1, trial, tlo, thi, lane);
  __builtin_amdgcn_wave_barrier();
  if (p.cr_random) draw_schedule(S.SC, S.WB, S.P1, p, k0, k1, tlo, thi, lane);
}

// ... and its end: the outcome over the nodes alive at the end (`none`: nobody was
// left at some step), and the states of a state launch.
__device__ __forceinline__ void crash_trial_end(const Planes &S, uint32_t *lhist, const KParams &p, bool none,
                                                bool all_dec, uint32_t R, uint64_t dec, uint32_t lane) {
  __builtin_amdgcn_wave_barrier();
  uint32_t K = 0, ms = 0;                          // the nodes alive at the end, and those with x = 1
  for (uint32_t j = 0; j < p.W; ++j) {
    const uint64_t al = S.AL[j];
    ms += (uint32_t)__builtin_popcountll(al);
    K += (uint32_t)__builtin_popcountll(S.X1[j] & al);
  }
  trial_end(lhist, p, uni(K), uni(ms), none, all_dec, R, lane);
  if (p.node_out) write_states<true>(p, S.AL, S.X1, S.X0, S.DEC, S.SC, p.cr_n, dec, R, lane);
}

// ---- the host side of a kernel with dynamic LDS
// Workgroups of the kernel that one CU holds at once (registers and LDS; 0 = unknown).
template <class Kernel>
int blocks_per_cu(Kernel kernel, const KParams &p) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 64 * kWavesPerBlock, p.lds_bytes);
  return e == hipSuccess ? n : 0;
}

template <class Kernel>
hipError_t launch_lds(Kernel kernel, const KParams &p, int grid, hipStream_t s) {
  if (p.lds_bytes > 64u * 1024u) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * kWavesPerBlock), p.lds_bytes, s, p);
  return hipGetLastError();
}

// The plan sizes a batch launch; a per-node-state launch (node_out set, one trial)
// holds `state_bytes` more per wave.
inline KParams state_launch(const KParams &plan, uint32_t state_bytes) {
  KParams p = plan;
  if (p.node_out) {
    p.wave_bytes += state_bytes;
    p.lds_bytes += kWavesPerBlock * state_bytes;
  }
  return p;
}

}  // namespace

}  // namespace benor

#endif  // device code
