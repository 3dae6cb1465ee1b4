// benor_tally_subset.hip -- count-level random delivery with crashes during the
// run whose last broadcast reaches an arbitrary subset of the receivers
// (BO_MODE_CRASH_SUBSET with a non-empty schedule).
//
// The model is benor_tally_partial.hip's with one change: a crasher has no cut.
// Crasher p's step-s message (its x at an R-step, the proposal it formed at step
// s - 1 at a P-step) reaches receiver c iff crash_reach == UINT32_MAX or
// word(p, c) < crash_reach, word(p, c) = element c & 3 of the Philox block
// {trial_lo, trial_hi, p | (c >> 2) << 12, 9 << 24} (stream 9; p and c compact
// indices).  Receiver c of the alive set A_s draws from the pool A_s + H_c,
// H_c = { p in C_s : p reaches c }: draw3 with m = m_s + |H_c| and the class
// sizes counted over that pool.
//
// H_c differs from lane to lane inside a group, so no contiguous run of receivers
// shares a pool.  What the draw needs of a receiver is only its profile (|H_c|,
// how many of H_c vote 0, how many vote 1): pool size, table, class sizes and row
// follow from it.  Per group and step:
//   1. the reach pass: the wave walks the step's crasher list four entries at a
//      time; lane l computes the block of entry i0 + (l & 3) for its quad of
//      receivers, the four lanes of a quad exchange words (three lane reads), and
//      every lane accumulates its own profile.  Skipped for an empty list, for
//      reach 0 (nobody) and for reach UINT32_MAX (every alive lane hears the whole
//      list);
//   2. the draw: the step has a base profile, the one every lane has when the
//      reach pass is skipped and the empty one otherwise.  Its phase is set up
//      once per step with the row staged in LDS (benor_tally_common.h's
//      wave-uniform phase_setup and draw3: a step without a reaching crasher is
//      that kernel's step), and the lanes with that profile draw from it.  The
//      other lanes, each with a pool of its own, draw in one more pass from their
//      own rows in global memory (draw3_lane: the same class choice, count and walk
//      with every quantity per lane).  The first form of this kernel staged a row
//      per distinct profile of the group instead and ran draw3 once per profile;
//      that cost 3.5-14.5 times mode 6's random cuts.
// draw3 is a pure function of (trial, c, r, phase, pool size, class sizes), so the
// order of the visits changes no result.  The tables are those of the pool sizes,
// found through benor_tally_crash.hip's directory: the pool of m_s + j nodes is
// entry (m0 - m_s) - j.
//
// Layout, planes, schedule, histogram and the state launch are
// benor_tally_crash.hip's; the per-wave LDS adds the step's crasher list, one word
// (compact index | class << 16) per entry, filled by step_begin: the class is read
// from the frozen planes before the step overwrites anything (X1, and X0 in round
// 1 -- later every alive x is binary -- at an R-step, P1 / P0 at a P-step).  No
// floating point runs on the device.
#include "benor_tally_common.h"

namespace benor {

namespace {

constexpr uint32_t kReachAll = 0xFFFFFFFFu;        // KParams::cr_reach: every crasher reaches every receiver

// (five waves per SIMD, benor_tally_crash.hip's occupancy)
__global__ void __launch_bounds__(256, 5) benor_tally_subset_kernel(KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t m0 = p.m, F = p.F, W = p.W, q = p.q, ncr = p.cr_n, reach = p.cr_reach;

  uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);
  const bool states = p.node_out != nullptr;       // a state launch: X0 and DEC planes of their own
  const Planes S(smem + p.hist_bytes + wv * p.wave_bytes,
                 crash_layout(W, p.tally_cap, ncr, p.cr_random != 0u, states, true));
  uint64_t *const AL = S.AL, *const X1 = S.X1, *const P1 = S.P1, *const P0 = S.P0, *const X0 = S.X0, *const row = S.row;
  uint32_t *const SC = S.SC, *const CL = S.CL;
  // A lane with a pool of its own searches its row where it lies in global memory, through the
  // directory; the halving starts from the plan's cap, which bounds every row (a wave-uniform loop).
  const uint32_t own_steps = search_steps(p.tally_cap);
  const auto own_table = [&](uint32_t m) {
    const CrashDir de = p.cr_dir[m0 - m];
    return Table{m, p.tally_off + de.off_base, p.tally_thr + de.thr_base};
  };

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
    // with the class of their last message, and leave the alive set; then the step's
    // live count.
    uint32_t ncs = 0u, nc0 = 0u, nc1 = 0u;         // the step's crashers, and those that vote 0 and 1
    const auto step_begin = [&](uint32_t s, uint32_t phase, uint32_t r) {
      __builtin_amdgcn_wave_barrier();             // the previous step's plane writes and list reads are done
      uint32_t n = 0u, n0 = 0u, n1 = 0u;
      for (uint32_t base = 0u; base < ncr; base += 64u) {
        const uint32_t i = base + lane;
        const uint32_t e = i < ncr ? SC[i] : 0xFFFFFFFFu;
        const bool hit = i < ncr && (e >> 12) == s;
        const uint64_t hb = ballot(hit);
        if (!hb) continue;
        uint32_t cls = 3u;
        if (hit) {
          const uint32_t c = e & 0xFFFu, j = c >> 6, b = c & 63u;
          if (phase == 0u) cls = ((X1[j] >> b) & 1ull) ? 1u : (r == 1u && !((X0[j] >> b) & 1ull) ? 2u : 0u);
          else cls = ((P1[j] >> b) & 1ull) ? 1u : (((P0[j] >> b) & 1ull) ? 0u : 2u);
          CL[n + (uint32_t)__builtin_popcountll(hb & ((1ull << lane) - 1ull))] = c | cls << 16;
          atomicAnd(reinterpret_cast<unsigned long long *>(&AL[j]), ~(1ull << b));
        }
        n += (uint32_t)__builtin_popcountll(hb);
        n0 += (uint32_t)__builtin_popcountll(ballot(cls == 0u));
        n1 += (uint32_t)__builtin_popcountll(ballot(cls == 1u));
      }
      ncs = n, nc0 = n0, nc1 = n1;
      __builtin_amdgcn_wave_barrier();
      uint32_t ms = 0;
      for (uint32_t j = 0; j < W; ++j) ms += (uint32_t)__builtin_popcountll(AL[j]);
      return uni(ms);
    };
    // The profile of receiver 64 j + lane at this step: pf = |H_c| | (members of H_c that vote 0) << 16,
    // pd1 = members that vote 1.
    const auto reach_pass = [&](uint32_t j, uint32_t &pf, uint32_t &pd1) {
      pf = 0u, pd1 = 0u;
      // Four neighbouring lanes share a block: lane l draws the block of entry i0 + (l & 3) for its
      // quad; in turn t it hands word (l - t) & 3 to the lane t places below it in the quad (cyclically),
      // which so reads its own word, l' & 3, of the block of entry i0 + ((l' + t) & 3).  One Philox
      // block and three lane reads per lane serve four crashers; the block alone is of the order of a
      // hundred vector operations, four per lane would be the plain form.
      const uint32_t pos = lane & 3u, quad = j * 16u + (lane >> 2);
      for (uint32_t i0 = 0u; i0 < ncs; i0 += 4u) {
        const uint32_t im = i0 + pos;
        const uint32_t pe = CL[im < ncs ? im : ncs - 1u] & 0xFFFu;
        const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, pe | quad << 12, kStreamReach << 24));
#pragma unroll
        for (uint32_t tn = 0u; tn < 4u; ++tn) {
          const uint32_t k = (pos + tn) & 3u, el = (pos - tn) & 3u;
          const uint32_t send = el == 0u ? b.x : (el == 1u ? b.y : (el == 2u ? b.z : b.w));
          const uint32_t w = tn == 0u ? send : (uint32_t)__shfl((int)send, (int)((lane & ~3u) | k), 64);
          const uint32_t i = i0 + k;
          const uint32_t cls = CL[i < ncs ? i : ncs - 1u] >> 16;
          if (i < ncs && w < reach) {
            pf += 1u + (cls == 0u ? 1u << 16 : 0u);
            pd1 += cls == 1u ? 1u : 0u;
          }
        }
      }
    };

    // The step's base profile (wave-uniform): everybody's when no reach pass runs -- the whole list at
    // reach UINT32_MAX, else nothing -- and the empty one with a reach pass.  Its phase is set up once
    // per step, by the first group with a lane that has it.
    bool varied = false, staged = false;
    uint32_t bf = 0u, bd1 = 0u, mp = 0u;
    PhaseC ph = phase_none();
    const auto base_profile = [&]() {
      const bool all = ncs != 0u && reach == kReachAll;
      varied = ncs != 0u && reach != 0u && reach != kReachAll;
      bf = all ? ncs | nc0 << 16 : 0u, bd1 = all ? nc1 : 0u;
      staged = false;
    };
    const auto stage = [&](uint32_t ms, uint32_t K0, uint32_t K1) {
      if (staged) return;
      const uint32_t hj = bf & 0xFFFFu, d0 = bf >> 16;
      mp = ms + hj;                                // the base profile's pool
      const Table tb = dir_table(p, mp);
      ph = phase_setup(row, p, tb, K0 + d0, K1 + bd1, mp - K0 - K1 - d0 - bd1, lane);
      staged = true;
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
      base_profile();
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t al = uni64(AL[j]);
        uint64_t p0 = 0ull, p1 = 0ull;
        if (al) {                                  // an emptied group draws nothing
          const uint32_t c = j * 64u + lane;
          // the round's block of receiver c: u_R = out[1] << 32 | out[0], u_P = out[3] << 32 | out[2]
          const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
          const uint64_t u = (uint64_t)b.y << 32 | b.x;
          uint32_t pf = bf, pd1 = bd1;
          uint64_t own = 0ull;                     // the lanes with a pool of their own
          if (varied) {
            reach_pass(j, pf, pd1);
            own = ballot(pf != 0u) & al;
          }
          uint32_t c0 = 0u, c1 = 0u;
          if (al & ~own) {
            stage(ms, K0, K1);
            draw3(row, ph, mp, q, k0, k1, tlo, thi, c, r, 0u, u, c0, c1);
          }
          if (own) {
            const bool mine = (own >> lane) & 1ull;
            uint32_t o0, o1;
            draw3_lane(own_table, p.tally_cap, own_steps, ms + (pf & 0xFFFFu), q, K0 + (pf >> 16), K1 + pd1, k0, k1, tlo, thi, c, r,
                       0u, u, mine, o0, o1);
            if (mine) c0 = o0, c1 = o1;
          }
          p0 = ballot(c0 > c1) & al;
          p1 = ballot(c1 > c0) & al;
        }
        if (lane == 0) P0[j] = p0, P1[j] = p1;
      }
      // ---- P-phase ("voting phase", node.ts:83-158), step 2 (r - 1) + 1: a node that
      // proposed and crashes here does not vote; its proposal reaches the receivers it reaches
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
      base_profile();
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t al = uni64(AL[j]);
        if (!al) continue;
        const uint32_t c = j * 64u + lane;
        const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
        const uint64_t u = (uint64_t)b.w << 32 | b.z;
        uint32_t pf = bf, pd1 = bd1;
        uint64_t own = 0ull;
        if (varied) {
          reach_pass(j, pf, pd1);
          own = ballot(pf != 0u) & al;
        }
        uint32_t c0 = 0u, c1 = 0u;
        if (al & ~own) {
          stage(ms, K0, K1);
          draw3(row, ph, mp, q, k0, k1, tlo, thi, c, r, 1u, u, c0, c1);
        }
        if (own) {
          const bool mo = (own >> lane) & 1ull;
          uint32_t o0, o1;
          draw3_lane(own_table, p.tally_cap, own_steps, ms + (pf & 0xFFFFu), q, K0 + (pf >> 16), K1 + pd1, k0, k1, tlo, thi, c, r,
                     1u, u, mo, o0, o1);
          if (mo) c0 = o0, c1 = o1;
        }
        bool decided;
        const uint64_t x1 = p_rule(c0, c1, F, al, k0, k1, tlo, thi, j, r, decided);
        const bool mine = (al >> lane) & 1ull;     // this lane's node is alive
        if (mine && decided) dec |= 1ull << j;     // sticky
        undecided = undecided || (mine && !((dec >> j) & 1ull));
        if (lane == 0) {                           // the bits of crashed nodes stay as of their crash
          X1[j] = (X1[j] & ~al) | x1;
          if (states) X0[j] = (X0[j] & ~al) | (al & ~x1);
        }
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
int subset_blocks_per_cu(const KParams &p) { return blocks_per_cu(benor_tally_subset_kernel, p); }

hipError_t launch_tally_subset(const KParams &plan, int grid, hipStream_t s) {
  const KParams p = state_launch(plan, crash_state_bytes(plan.W));
  // (an explicit schedule whose steps all lie beyond 2 k_max leaves an empty list)
  if (!p.tally_off || !p.tally_thr || !p.cr_dir || p.W > kMaxW || p.cr_n > p.m ||
      (!p.cr_random && p.cr_n != 0u && !p.cr_list) || (p.cr_random && (p.cr_n == 0u || p.crash_window == 0u)) ||
      plan.wave_bytes < crash_wave_bytes(p.W, p.tally_cap, p.cr_n, p.cr_random != 0u, true))
    return hipErrorInvalidValue;
  return launch_lds(benor_tally_subset_kernel, p, grid, s);
}

}  // namespace benor
