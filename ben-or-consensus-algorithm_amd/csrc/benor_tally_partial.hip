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
// benor_tally_common.h's wave-uniform machinery -- phase_setup, the row staged in
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
#include "benor_tally_common.h"

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

  uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);
  const bool states = p.node_out != nullptr;       // a state launch: X0 and DEC planes of their own
  const Planes S(smem + p.hist_bytes + wv * p.wave_bytes,
                 crash_layout(W, p.tally_cap, ncr, p.cr_random != 0u, states, true));
  uint64_t *const AL = S.AL, *const X1 = S.X1, *const P1 = S.P1, *const P0 = S.P0, *const X0 = S.X0, *const row = S.row;
  uint32_t *const SC = S.SC, *const CL = S.CL;

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
    crash_trial_start(S, p, k0, k1, trial, tlo, thi, lane);

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
        const Table tb = dir_table(p, mp);
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
        const Table tb = dir_table(p, mp);
        const PhaseC ph = phase_setup(row, p, tb, K0 + sg.d0, K1 + sg.d1, mp - K0 - K1 - sg.d0 - sg.d1, lane);
        for (uint32_t j = pos >> 6; j <= (sg.end - 1u) >> 6; ++j) {
          const uint64_t al = uni64(AL[j]) & segment_mask(j, pos, sg.end);
          if (!al) continue;
          const uint32_t c = j * 64u + lane;
          const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
          uint32_t c0, c1;
          draw3(row, ph, mp, q, k0, k1, tlo, thi, c, r, 1u, (uint64_t)b.w << 32 | b.z, c0, c1);
          bool decided;
          const uint64_t x1 = p_rule(c0, c1, F, al, k0, k1, tlo, thi, j, r, decided);
          const bool mine = (al >> lane) & 1ull;   // this lane's node is alive and in the segment
          if (mine && decided) dec |= 1ull << j;   // sticky
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
    crash_trial_end(S, lhist, p, none, all_dec, R, dec, lane);
  }

  __syncthreads();
  flush_hist(lhist, p);
}

}  // namespace

// Workgroups of the kernel that one CU holds at once (registers and LDS; 0 = unknown).
int partial_blocks_per_cu(const KParams &p) { return blocks_per_cu(benor_tally_partial_kernel, p); }

hipError_t launch_tally_partial(const KParams &plan, int grid, hipStream_t s) {
  const KParams p = state_launch(plan, crash_state_bytes(plan.W));
  // (an explicit schedule whose steps all lie beyond 2 k_max leaves an empty list)
  if (!p.tally_off || !p.tally_thr || !p.cr_dir || p.W > kMaxW || p.cr_n > p.m ||
      (!p.cr_random && p.cr_n != 0u && !p.cr_list) || (p.cr_random && (p.cr_n == 0u || p.crash_window == 0u)) ||
      (p.cr_cut != kCutRandom && p.cr_cut > p.m) ||
      plan.wave_bytes < crash_wave_bytes(p.W, p.tally_cap, p.cr_n, p.cr_random != 0u, true))
    return hipErrorInvalidValue;
  return launch_lds(benor_tally_partial_kernel, p, grid, s);
}

}  // namespace benor
