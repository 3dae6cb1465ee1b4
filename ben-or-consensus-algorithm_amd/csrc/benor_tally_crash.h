// benor_tally_crash.h -- device helpers shared by the count-level kernels with
// crashes during the run: benor_tally_crash.hip (BO_MODE_CRASH_TALLY, DESIGN
// §4.3.3) and benor_tally_partial.hip (BO_MODE_CRASH_PARTIAL, §4.3.4).  The table
// of a pool size, a phase's wave-uniform set-up with its row staged in LDS, the
// per-receiver draw (benor_tally3.hip's draw3 with the pool size a parameter) and
// the per-trial random schedule (Philox stream 7).
#pragma once

#include "benor_device.h"

namespace benor {

namespace {

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return (uint64_t)uni((uint32_t)(v >> 32)) << 32 | uni((uint32_t)v); }

constexpr uint32_t kStepClamp = 0xFFFFFu;          // schedule entries: step in 20 bits, compact index in 12
constexpr uint32_t kSchedWords = 256u;             // stream-7 words drawn per pass (64 lanes, one block each)

// The table of the step's live count.
struct Table {
  uint32_t m;                                      // m_s
  const uint32_t *off;                             // [m_s + 2] row offsets
  const unsigned long long *thr;
};

// The wave-uniform part of a phase's draw (benor_tally3.hip Phase3).
struct PhaseC {
  uint32_t sel;      // 0: S = "?", A = 1, T = 0;  1: S = 0, A = 1, T = "?";  2: S = 1, A = 0, T = "?"
  uint32_t KA, KS;   // class sizes
  uint32_t lo;       // max(0, q - (m_s - KA)): row KA's least count
  uint32_t n, steps; // row KA staged in LDS: its width, and ceil(log2(n + 1))
};

__device__ __forceinline__ PhaseC phase_setup(uint64_t *__restrict__ row, const KParams &p, const Table &tb, uint32_t K0,
                                              uint32_t K1, uint32_t Kq, uint32_t lane) {
  PhaseC ph;
  if (Kq <= K0 && Kq <= K1) ph.sel = 0u, ph.KS = Kq, ph.KA = K1;
  else if (K0 <= K1) ph.sel = 1u, ph.KS = K0, ph.KA = K1;
  else ph.sel = 2u, ph.KS = K1, ph.KA = K0;
  const uint32_t m = tb.m, q = p.q, K = ph.KA;
  ph.lo = K + q > m ? K + q - m : 0u;
  ph.n = 0u, ph.steps = 0u;
  if (K != 0u && K != m && m != q) {               // else the row is a point
    __builtin_amdgcn_wave_barrier();               // the previous phase's searches are done with the region
    const uint32_t o = uni(tb.off[K]);
    uint32_t n = uni(tb.off[K + 1u]) - o;
    if (n > p.tally_cap) n = p.tally_cap;          // the region's size (no row of any table exceeds it)
    const unsigned long long *src = tb.thr + o;
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

// Receiver c's counts (c0, c1) of the phase among m senders: benor_tally3.hip's draw3.
__device__ __forceinline__ void draw3(const uint64_t *__restrict__ row, const PhaseC &ph, uint32_t m, uint32_t q,
                                      uint32_t k0, uint32_t k1, uint32_t tlo, uint32_t thi, uint32_t c, uint32_t r,
                                      uint32_t phase, uint64_t u, uint32_t &c0, uint32_t &c1) {
  uint32_t cA = ph.lo;
  if (ph.n != 0u) cA += row_count(row, ph.n, ph.steps, u);
  uint32_t cS = 0u;
  if (ph.KS != 0u) {
    if (m == q) {
      cS = ph.KS;                                  // every alive sender is in the inbox
    } else {
      const uint32_t slots = q - cA;               // inbox slots left to the senders outside A
      const uint32_t dtop = m - ph.KA;             // ... of which there are this many (>= slots, >= KS)
      const uint32_t c3 = (r - 1u) | (phase << 16) | (kStreamWalk << 24);
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

}  // namespace

}  // namespace benor
