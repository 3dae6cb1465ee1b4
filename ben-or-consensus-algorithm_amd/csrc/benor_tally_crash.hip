// benor_tally_crash.hip -- count-level random delivery with crashes during the
// run (BO_MODE_CRASH_TALLY with a non-empty schedule).
//
// The model is benor_tally3.hip's with the live set no longer constant: a node
// may crash at a step boundary (step 2(r - 1) = the R-phase of round r, step
// 2(r - 1) + 1 = its P-phase).  At step s the senders and the receivers are the
// alive set A_s, m_s = |A_s| >= q, the class sizes are counted over A_s, and a
// receiver's (c0, c1) is benor_tally_common.h's draw3 with m = m_s: one count from
// row K_A of the HG(m_s, ., q) table, the smallest class walked from stream 6.
// So the plan holds one table per reachable live count, found through a small
// directory indexed by the number of crashes so far (CrashDir), and m_s, the
// table choice and every class size are wave-uniform.
//
// One wave = one trial, lane l of receiver group j = compact index 64 j + l over
// the initially-live nodes, fixed for the run: a crashed node is a hole in its
// group, never compacted, and a group may become empty.  Per-wave LDS state:
// ballot planes of W words -- AL (alive), X0 / X1 (x = 0, x = 1; neither: "?"),
// P0 / P1 (the round's proposals) -- and the sticky decided bits, bit j of a
// lane's register for group j.  A bit of a crashed node is never written again,
// so it holds the node's state as of its crash.  That state is only reported by
// a per-node-state launch; in a batch launch X0 is dead once round 1 has counted
// its classes (after a P-phase every alive x is binary), so P0 takes its words
// and a wave holds four planes, which at N = 4096 keeps three workgroups on a
// CU as benor_tally3.hip has; a state launch adds X0 and a decided plane of its
// own (crash_state_bytes).  The schedule is a list of (step << 12 | compact
// index), step clamped to 2^20 - 1 (no run reaches step 2 BO_MAX_K): the plan's
// for an explicit schedule, drawn per trial by Floyd's algorithm from Philox
// stream 7 for a random one.  No floating point runs on the device.
#include "benor_tally_common.h"

namespace benor {

namespace {

__global__ void __launch_bounds__(256) benor_tally_crash_kernel(KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t F = p.F, W = p.W, q = p.q, ncr = p.cr_n;

  uint32_t *lhist = reinterpret_cast<uint32_t *>(smem);
  const bool states = p.node_out != nullptr;       // a state launch: X0 and DEC planes of their own
  const Planes S(smem + p.hist_bytes + wv * p.wave_bytes,
                 crash_layout(W, p.tally_cap, ncr, p.cr_random != 0u, states, false));
  uint64_t *const AL = S.AL, *const X1 = S.X1, *const P1 = S.P1, *const P0 = S.P0, *const X0 = S.X0, *const row = S.row;
  uint32_t *const SC = S.SC;

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

    // The crashes of step s, then the step's live count and its table.
    Table tb;
    const auto step_begin = [&](uint32_t s) {
      __builtin_amdgcn_wave_barrier();             // the previous step's plane writes are done
      for (uint32_t i = lane; i < ncr; i += 64u) {
        const uint32_t e = SC[i];
        if ((e >> 12) == s) {
          const uint32_t c = e & 0xFFFu;
          atomicAnd(reinterpret_cast<unsigned long long *>(&AL[c >> 6]), ~(1ull << (c & 63u)));
        }
      }
      __builtin_amdgcn_wave_barrier();
      uint32_t ms = 0;
      for (uint32_t j = 0; j < W; ++j) ms += (uint32_t)__builtin_popcountll(AL[j]);
      ms = uni(ms);
      tb = dir_table(p, ms);
      return ms;
    };

    uint64_t dec = 0ull;                           // bit j: node 64 j + lane has decided (sticky)
    uint32_t R = 0;
    bool all_dec = false, none = false;
    for (uint32_t r = 1; r <= p.k_max; ++r) {
      // ---- R-phase ("proposal phase", node.ts:46-82), step 2 (r - 1)
      uint32_t ms = step_begin(2u * (r - 1u));
      if (ms == 0u) { none = true; break; }
      uint32_t K0 = 0, K1 = 0;
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t al = AL[j];
        if (r == 1u) K0 += (uint32_t)__builtin_popcountll(X0[j] & al);
        K1 += (uint32_t)__builtin_popcountll(X1[j] & al);
      }
      K1 = uni(K1);
      K0 = r == 1u ? uni(K0) : ms - K1;            // after a P-phase every alive x is binary
      PhaseC ph = phase_setup(row, p, tb, K0, K1, ms - K0 - K1, lane);
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t al = uni64(AL[j]);
        uint64_t p0 = 0ull, p1 = 0ull;
        if (al) {                                  // an emptied group draws nothing
          const uint32_t c = j * 64u + lane;
          // the round's block of receiver c: u_R = out[1] << 32 | out[0], u_P = out[3] << 32 | out[2]
          const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
          uint32_t c0, c1;
          draw3(row, ph, ms, q, k0, k1, tlo, thi, c, r, 0u, (uint64_t)b.y << 32 | b.x, c0, c1);
          p0 = ballot(c0 > c1) & al;
          p1 = ballot(c1 > c0) & al;
        }
        if (lane == 0) P0[j] = p0, P1[j] = p1;
      }
      // ---- P-phase ("voting phase", node.ts:83-158), step 2 (r - 1) + 1: a node that
      // proposed and crashes here does not vote
      ms = step_begin(2u * (r - 1u) + 1u);
      if (ms == 0u) { none = true; break; }
      K0 = 0, K1 = 0;
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t al = AL[j];
        K0 += (uint32_t)__builtin_popcountll(P0[j] & al);
        K1 += (uint32_t)__builtin_popcountll(P1[j] & al);
      }
      K0 = uni(K0), K1 = uni(K1);
      ph = phase_setup(row, p, tb, K0, K1, ms - K0 - K1, lane);
      bool undecided = false;
      for (uint32_t j = 0; j < W; ++j) {
        const uint64_t al = uni64(AL[j]);
        if (!al) continue;
        const uint32_t c = j * 64u + lane;
        const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
        uint32_t c0, c1;
        draw3(row, ph, ms, q, k0, k1, tlo, thi, c, r, 1u, (uint64_t)b.w << 32 | b.z, c0, c1);
        bool decided;
        const uint64_t x1 = p_rule(c0, c1, F, al, k0, k1, tlo, thi, j, r, decided);
        const bool mine = (al >> lane) & 1ull;     // this lane's node is alive
        if (mine && decided) dec |= 1ull << j;     // sticky
        if (lane == 0) {                           // the bits of crashed nodes stay as of their crash
          X1[j] = (X1[j] & ~al) | x1;
          if (states) X0[j] = (X0[j] & ~al) | (al & ~x1);
        }
        undecided = undecided || (mine && !((dec >> j) & 1ull));
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
int crash_blocks_per_cu(const KParams &p) { return blocks_per_cu(benor_tally_crash_kernel, p); }

hipError_t launch_tally_crash(const KParams &plan, int grid, hipStream_t s) {
  const KParams p = state_launch(plan, crash_state_bytes(plan.W));
  // (an explicit schedule whose steps all lie beyond 2 k_max leaves an empty list)
  if (!p.tally_off || !p.tally_thr || !p.cr_dir || p.W > kMaxW || p.cr_n > p.m ||
      (!p.cr_random && p.cr_n != 0u && !p.cr_list) || (p.cr_random && (p.cr_n == 0u || p.crash_window == 0u)) ||
      plan.wave_bytes < crash_wave_bytes(p.W, p.tally_cap, p.cr_n, p.cr_random != 0u, false))
    return hipErrorInvalidValue;
  return launch_lds(benor_tally_crash_kernel, p, grid, s);
}

}  // namespace benor
