// benor_tally_partial.hip -- count-level random delivery with crashes during the
// run whose last broadcast is partial (BO_MODE_CRASH_PARTIAL with a non-empty
// schedule).
//
// The model is benor_tally_crash.hip's with one change.  The reference broadcasts
// in ascending node id (node.ts:72-80, :149-157, :173-185), so a node that crashes
// in the middle of its step-s broadcast reaches a prefix of the receivers: crasher
// p has a cut, cut_p in [0, m0], and its step-s message (its x at an R-step, the
// proposal it formed at step s - 1 at a P-step) reaches exactly the receivers with
// compact index c < cut_p.  It does not receive at step s.  Receiver c of the alive
// set A_s draws from the pool A_s + H_c, H_c = { p in C_s : c < cut_p }: draw3 with
// m = m_s + |H_c| and the class sizes counted over that pool.
//
// The cuts of a step split the compact indices into at most |C_s| + 1 contiguous
// segments inside which H_c, and so the pool size, the table and the three class
// sizes, are the same for every receiver.  So the kernel keeps
// benor_tally_crash.hip's wave-uniform machinery -- phase_setup, the row staged in
// LDS, draw3 -- and runs it once per segment instead of once per step: the next
// boundary is the smallest cut above the current position (a wave reduction over
// the step's crasher list), the groups that overlap the segment are drawn with the
// lanes outside it masked out of the ballots.  A step without crashers (or whose
// cuts are all 0) is one segment, benor_tally_crash.hip's step.  The tables are
// those of the pool sizes, found through the same directory: the pool of m_s + j
// nodes is entry (m0 - m_s) - j.
//
// Layout, planes, schedule, histogram and the state launch are
// benor_tally_crash.hip's; the per-wave LDS adds the step's crasher list, one word
// (cut | class << 16) per entry, filled by step_begin: the cut is the plan's or
// one draw below m0 + 1 from Philox stream 8, blocks {trial_lo, trial_hi,
// c | b << 12, 8 << 24} keyed by the crasher's compact index c; the class is read
// from the frozen planes before the step overwrites anything (X1, and X0 in round
// 1 -- later every alive x is binary -- at an R-step, P1 / P0 at a P-step).  No
// floating point runs on the device.
#include "benor_tally_crash.h"

namespace benor {

namespace {

constexpr uint32_t kCutRandom = 0xFFFFFFFFu;       // KParams::cr_cut: a cut per trial and crasher

// One segment of a step: the receivers pos <= c < end hear the same j crashers.
struct Segment {
  uint32_t end;                                    // the smallest cut above pos, m0 if none
  uint32_t j, d0, d1;                              // |H_c|, and how many of them vote 0 and 1
};

// The segment that starts at pos: over the step's n crashers CL[i] = cut | class << 16.
__device__ __forceinline__ Segment next_segment(const uint32_t *__restrict__ CL, uint32_t n, uint32_t pos, uint32_t m0,
                                                uint32_t lane) {
  Segment sg;
  sg.end = m0, sg.j = 0u, sg.d0 = 0u, sg.d1 = 0u;
  for (uint32_t base = 0u; base < n; base += 64u) {
    const uint32_t i = base + lane;
    const uint32_t e = i < n ? CL[i] : 0u;
    const uint32_t cut = e & 0xFFFFu, cls = e >> 16;
    const bool in = i < n && cut > pos;            // this crasher's message reaches the segment
    const uint64_t hb = ballot(in);
    if (hb) {
      sg.j += (uint32_t)__builtin_popcountll(hb);
      sg.d0 += (uint32_t)__builtin_popcountll(ballot(in && cls == 0u));
      sg.d1 += (uint32_t)__builtin_popcountll(ballot(in && cls == 1u));
      uint32_t v = in ? cut : m0;
      for (uint32_t o = 32u; o != 0u; o >>= 1) {
        const uint32_t w = (uint32_t)__shfl_xor((int)v, (int)o, 64);
        v = w < v ? w : v;
      }
      v = uni(v);
      sg.end = v < sg.end ? v : sg.end;
    }
  }
  return sg;
}

// (five waves per SIMD, benor_tally_crash.hip's occupancy: without the bound the segment walk's
// live values take 101 VGPRs and one wave per SIMD less)
__global__ void __launch_bounds__(256, 5) benor_tally_partial_kernel(KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t m0 = p.m, F = p.F, W = p.W, q = p.q, ncr = p.cr_n;
  const uint32_t WP = (W + 1u) & ~1u;

  uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);
  const bool states = p.node_out != nullptr;       // a state launch: X0 and DEC planes of their own
  const uint32_t capE = (p.tally_cap + 1u) & ~1u;
  uint64_t *AL = reinterpret_cast<uint64_t *>(smem + p.hist_bytes + wv * p.wave_bytes);   // [W] alive
  uint64_t *X1 = AL + WP;                                                                 // [W] x = 1
  uint64_t *P1 = X1 + WP, *P0 = P1 + WP;                                                  // [W] proposals 1, 0
  uint64_t *X0 = states ? P0 + WP : P0;                                                   // [W] x = 0 (round 1)
  uint64_t *DEC = X0 + WP;                                                                // [W] decided (state launch)
  uint64_t *row = AL + (states ? 6u : 4u) * WP;                                           // [tally_cap] thresholds
  // [256] stream-7 words: in the row region when it is large enough (no row is staged while a schedule is drawn)
  uint32_t *WB = reinterpret_cast<uint32_t *>(2u * capE >= kSchedWords ? row : row + capE);
  uint32_t *SC = reinterpret_cast<uint32_t *>(row + capE) +
                 (p.cr_random && 2u * capE < kSchedWords ? kSchedWords : 0u);             // [ncr] the schedule
  uint32_t *CL = SC + ((ncr + 3u) & ~3u);                                                 // [ncr] the step's crashers

  for (uint32_t i = threadIdx.x; i < p.hist_len; i += blockDim.x) lhist[i] = 0u;
  __syncthreads();

  if (!p.cr_random)                                // an explicit schedule is the plan's, the same for every trial
    for (uint32_t i = lane; i < ncr; i += 64u) SC[i] = p.cr_list[i];

  const uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32);
  const uint64_t waves_total = (uint64_t)gridDim.x * kWavesPerBlock;

  for (uint64_t t = (uint64_t)blockIdx.x * kWavesPerBlock + wv; t < p.trial_count; t += waves_total) {
    const uint64_t trial = p.trial_begin + t;
    const uint32_t tlo = uni((uint32_t)trial), thi = uni((uint32_t)(trial >> 32));
    __builtin_amdgcn_wave_barrier();               // the previous trial's state reads are done
    if (lane < W) {
      AL[lane] = group_mask(lane, m0);
      P1[lane] = 0ull;                             // the schedule draw's chosen set
    }
    if (p.init_mode == BO_INIT_RANDOM) {           // /start (node.ts:167-188): stream 1, as every batch mode
      const uint32_t nph = (W + 1u) >> 1;
      if (lane < nph) {
        uint4 r;
        if (m0 <= 32u) r = make_uint4(init_word_small(k0, k1, trial), 0u, 0u, 0u);   // shared block (m <= 32)
        else r = philox4x32_10(k0, k1, make_uint4(tlo, thi, lane, kStreamInit << 24));
        const uint32_t w0 = 2u * lane, w1 = w0 + 1u;
        const uint64_t g0 = group_mask(w0, m0), a0 = ((uint64_t)r.y << 32 | r.x) & g0;
        X1[w0] = a0, X0[w0] = g0 & ~a0;
        if (w1 < W) {
          const uint64_t g1 = group_mask(w1, m0), a1 = ((uint64_t)r.w << 32 | r.z) & g1;
          X1[w1] = a1, X0[w1] = g1 & ~a1;
        }
      }
    } else {
      for (uint32_t w = lane; w < W; w += 64u) {
        const uint4 rc = p.init_plane[w];
        X0[w] = (uint64_t)rc.y << 32 | rc.x;
        X1[w] = (uint64_t)rc.w << 32 | rc.z;
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (p.cr_random) draw_schedule(SC, WB, P1, p, k0, k1, tlo, thi, lane);

    // The crashers of step s (phase 0: an R-step of round r, 1: a P-step) go into CL
    // with their cut and the class of their last message, and leave the alive set;
    // then the step's live count.
    uint32_t ncs = 0u;                             // the step's crashers
    const auto step_begin = [&](uint32_t s, uint32_t phase, uint32_t r) {
      __builtin_amdgcn_wave_barrier();             // the previous step's plane writes and list reads are done
      uint32_t n = 0u;
      for (uint32_t base = 0u; base < ncr; base += 64u) {
        const uint32_t i = base + lane;
        const uint32_t e = i < ncr ? SC[i] : 0xFFFFFFFFu;
        const bool hit = i < ncr && (e >> 12) == s;
        const uint64_t hb = ballot(hit);
        if (!hb) continue;
        if (hit) {
          const uint32_t c = e & 0xFFFu, j = c >> 6, b = c & 63u;
          uint32_t cls;
          if (phase == 0u) cls = ((X1[j] >> b) & 1ull) ? 1u : (r == 1u && !((X0[j] >> b) & 1ull) ? 2u : 0u);
          else cls = ((P1[j] >> b) & 1ull) ? 1u : (((P0[j] >> b) & 1ull) ? 0u : 2u);
          uint32_t cut = p.cr_cut;
          if (cut == kCutRandom) {                 // below(m0 + 1) from stream 8's words, in order
            const uint32_t d = m0 + 1u, rem = (0u - d) % d;
            bool have = false;
            for (uint32_t blk = 0u; !have; ++blk) {
              const uint4 w4 = philox4x32_10(k0, k1, make_uint4(tlo, thi, c | (blk << 12), kStreamCut << 24));
              const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
              for (uint32_t k = 0u; k < 4u; ++k) {
                const uint64_t mm = (uint64_t)w[k] * d;
                if (!have && (uint32_t)mm >= rem) cut = (uint32_t)(mm >> 32), have = true;
              }
            }
          }
          CL[n + (uint32_t)__builtin_popcountll(hb & ((1ull << lane) - 1ull))] = cut | cls << 16;
          atomicAnd(reinterpret_cast<unsigned long long *>(&AL[j]), ~(1ull << b));
        }
        n += (uint32_t)__builtin_popcountll(hb);
      }
      ncs = n;
      __builtin_amdgcn_wave_barrier();
      uint32_t ms = 0;
      for (uint32_t j = 0; j < W; ++j) ms += (uint32_t)__builtin_popcountll(AL[j]);
      return uni(ms);
    };
    // The table of a pool of m nodes: m0 - m <= ncr crashes so far.
    const auto table_of = [&](uint32_t m) {
      const CrashDir de = p.cr_dir[m0 - m];
      Table tb;
      tb.m = m;
      tb.off = p.tally_off + uni(de.off_base);
      tb.thr = p.tally_thr + uni64(de.thr_base);
      return tb;
    };
    // The lanes of group j inside the segment [pos, end), end > 64 j, pos < 64 j + 64.
    const auto segment_mask = [](uint32_t j, uint32_t pos, uint32_t end) {
      const uint32_t lo = j * 64u;
      uint64_t sm = ~0ull;
      if (pos > lo) sm &= ~0ull << (pos - lo);
      if (end < lo + 64u) sm &= ~0ull >> (lo + 64u - end);
      return sm;
    };

    uint64_t dec = 0ull;                           // bit j: node 64 j + lane has decided (sticky)
    uint32_t R = 0;
    bool all_dec = false, none = false;
    for (uint32_t r = 1; r <= p.k_max; ++r) {
      // ---- R-phase ("proposal phase", node.ts:46-82), step 2 (r - 1)
      uint32_t ms = step_begin(2u * (r - 1u), 0u, r);
      if (ms == 0u) { none = true; break; }
      uint32_t K0 = 0, K1 = 0;
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t al = AL[j];
        if (r == 1u) K0 += (uint32_t)__builtin_popcountll(X0[j] & al);
        K1 += (uint32_t)__builtin_popcountll(X1[j] & al);
      }
      K1 = uni(K1);
      K0 = r == 1u ? uni(K0) : ms - K1;            // after a P-phase every alive x is binary
      for (uint32_t pos = 0u; pos < m0;) {
        const Segment sg = next_segment(CL, ncs, pos, m0, lane);
        const uint32_t mp = ms + sg.j;             // the segment's pool
        const Table tb = table_of(mp);
        const PhaseC ph = phase_setup(row, p, tb, K0 + sg.d0, K1 + sg.d1, mp - K0 - K1 - sg.d0 - sg.d1, lane);
        for (uint32_t j = pos >> 6; j <= (sg.end - 1u) >> 6; ++j) {
          const uint64_t al = uni64(AL[j]) & segment_mask(j, pos, sg.end);
          uint64_t p0 = 0ull, p1 = 0ull;
          if (al) {                                // an emptied group draws nothing
            const uint32_t c = j * 64u + lane;
            // the round's block of receiver c: u_R = out[1] << 32 | out[0], u_P = out[3] << 32 | out[2]
            const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
            uint32_t c0, c1;
            draw3(row, ph, mp, q, k0, k1, tlo, thi, c, r, 0u, (uint64_t)b.y << 32 | b.x, c0, c1);
            p0 = ballot(c0 > c1) & al;
            p1 = ballot(c1 > c0) & al;
          }
          if (lane == 0) {
            if (pos > j * 64u) P0[j] |= p0, P1[j] |= p1;   // the group's earlier segments
            else P0[j] = p0, P1[j] = p1;
          }
        }
        pos = sg.end;
      }
      // ---- P-phase ("voting phase", node.ts:83-158), step 2 (r - 1) + 1: a node that
      // proposed and crashes here does not vote; its proposal reaches the receivers below its cut
      ms = step_begin(2u * (r - 1u) + 1u, 1u, r);
      if (ms == 0u) { none = true; break; }
      K0 = 0, K1 = 0;
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t al = AL[j];
        K0 += (uint32_t)__builtin_popcountll(P0[j] & al);
        K1 += (uint32_t)__builtin_popcountll(P1[j] & al);
      }
      K0 = uni(K0), K1 = uni(K1);
      bool undecided = false;
      for (uint32_t pos = 0u; pos < m0;) {
        const Segment sg = next_segment(CL, ncs, pos, m0, lane);
        const uint32_t mp = ms + sg.j;
        const Table tb = table_of(mp);
        const PhaseC ph = phase_setup(row, p, tb, K0 + sg.d0, K1 + sg.d1, mp - K0 - K1 - sg.d0 - sg.d1, lane);
        for (uint32_t j = pos >> 6; j <= (sg.end - 1u) >> 6; ++j) {
          const uint64_t al = uni64(AL[j]) & segment_mask(j, pos, sg.end);
          if (!al) continue;
          const uint32_t c = j * 64u + lane;
          const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
          uint32_t c0, c1;
          draw3(row, ph, mp, q, k0, k1, tlo, thi, c, r, 1u, (uint64_t)b.w << 32 | b.z, c0, c1);
          const bool d0l = c0 > F, d1l = !d0l && c1 > F;
          const uint64_t d0 = ballot(d0l) & al;
          const uint64_t d1 = ballot(d1l) & al;
          const uint64_t rest = al & ~(d0 | d1);
          uint64_t x1 = d1;
          if (rest) {
            x1 |= ballot(c1 > c0) & rest;
            const uint64_t tie = ballot(c1 == c0) & rest;              // an empty tally included
            if (tie) x1 |= coin_ballot(k0, k1, tlo, thi, j, r, tie);
          }
          const bool mine = (al >> lane) & 1ull;   // this lane's node is alive and in the segment
          if (mine && (d0l || d1l)) dec |= 1ull << j;                  // sticky
          if (lane == 0) {                         // the bits of crashed nodes stay as of their crash
            X1[j] = (X1[j] & ~al) | x1;
            if (states) X0[j] = (X0[j] & ~al) | (al & ~x1);
          }
          undecided = undecided || (mine && !((dec >> j) & 1ull));
        }
        pos = sg.end;
      }
      R = r;
      all_dec = !__any(undecided);                 // over the alive nodes
      if (all_dec) break;
    }
    __builtin_amdgcn_wave_barrier();
    uint32_t K = 0, ms = 0;                        // the nodes alive at the end, and those with x = 1
    for (uint32_t j = 0; j < W; ++j) {
      const uint64_t al = AL[j];
      ms += (uint32_t)__builtin_popcountll(al);
      K += (uint32_t)__builtin_popcountll(X1[j] & al);
    }
    K = uni(K), ms = uni(ms);
    const uint32_t v = none ? 2u : ((K != 0u && K != ms) ? 2u : (K != 0u ? 1u : 0u));
    if (none) all_dec = false;                     // nobody left: bin[2], rounds 0
    if (lane == 0) {
      atomicAdd(&lhist[all_dec ? (R * 3u + v) : v], 1u);
      if (all_dec && v == 2u) atomicAdd(&lhist[p.hist_len - 1u], 1u);
      if (p.rounds_out) *p.rounds_out = all_dec ? R : 0u;
    }
    if (states) {
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t d = ballot((dec >> j) & 1ull);
        if (lane == 0) DEC[j] = d;
      }
      __builtin_amdgcn_wave_barrier();
      for (uint32_t c = lane; c < m0; c += 64u) {
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
      for (uint32_t i = lane; i < ncr; i += 64u) {   // crashed: x and decided as of the crash, k its round
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

  __syncthreads();
  flush_hist(lhist, p);
}

}  // namespace

// A batch launch's per-wave LDS: benor_tally_crash.hip's (four planes, the row
// region, the stream-7 words where the row region is too small for them, the
// schedule) and the step's crasher list.
uint32_t partial_wave_bytes(uint32_t W, uint32_t cap, uint32_t ncr, bool random) {
  return crash_wave_bytes(W, cap, ncr, random) + ((ncr + 3u) & ~3u) * 4u;
}

// Workgroups of the kernel that one CU holds at once (registers and LDS; 0 = unknown).
int partial_blocks_per_cu(const KParams &p) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, benor_tally_partial_kernel, 64 * kWavesPerBlock,
                                                                    p.lds_bytes);
  return e == hipSuccess ? n : 0;
}

hipError_t launch_tally_partial(const KParams &plan, int grid, hipStream_t s) {
  KParams p = plan;
  if (p.node_out) {                                // a state launch (one trial): two more planes per wave
    p.wave_bytes += crash_state_bytes(p.W);
    p.lds_bytes += kWavesPerBlock * crash_state_bytes(p.W);
  }
  // (an explicit schedule whose steps all lie beyond 2 k_max leaves an empty list)
  if (!p.tally_off || !p.tally_thr || !p.cr_dir || p.W > kMaxW || p.cr_n > p.m ||
      (!p.cr_random && p.cr_n != 0u && !p.cr_list) || (p.cr_random && (p.cr_n == 0u || p.crash_window == 0u)) ||
      (p.cr_cut != kCutRandom && p.cr_cut > p.m) ||
      plan.wave_bytes < partial_wave_bytes(p.W, p.tally_cap, p.cr_n, p.cr_random != 0u))
    return hipErrorInvalidValue;
  if (p.lds_bytes > 64u * 1024u) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&benor_tally_partial_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(benor_tally_partial_kernel, dim3(grid), dim3(64 * kWavesPerBlock), p.lds_bytes, s, p);
  return hipGetLastError();
}

}  // namespace benor
