// benor_tally.hip -- count-level random delivery (BO_MODE_RANDOM_TALLY).
//
// The receiver's rule (node.ts:52-69 R-phase, :88-113 P-phase) reads only the
// counts (c0, c1) of its inbox.  Under the random-delivery model the inbox is a
// uniform q-subset of the m live senders, independent per (receiver, round,
// phase), so with K senders holding a 1 the count c1 is Hypergeometric(m, K, q)
// and c0 = q - c1.  This kernel draws c1 directly: one Philox block per
// receiver-round (stream 5) gives two 64-bit uniforms, and each is turned into
// a count by a search in row K of the host-built threshold table
// (benor_runtime.cpp tally_row; bo_tally_cdf returns the same row).  Scope: q odd
// and no "?" initial value, so every vote is binary, no tally ties and no coin
// is drawn.
//
// One wave = one trial, lane l of receiver group j = live node 64 j + l
// (compact index c).  Per phase the wave stages row K (at most min(q, m - q)
// thresholds) into its LDS region, then every lane runs the same number of
// binary-search steps, ceil(log2(width + 1)), with one ds_read_b64 each: no
// divergent loop.  A row of width 0 (K = 0, K = m, or m = q) needs neither.
// K is the popcount of the phase's ballots, accumulated on the scalar side.
// No floating point runs on the device: results are a function of the table
// and Philox alone.
#include "benor_tally_common.h"

namespace benor {

namespace {

template <int WT>
__global__ void __launch_bounds__(256) benor_tally_kernel(KParams p) {
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
    trial_start<false>(X1, nullptr, p, k0, k1, trial, tlo, thi, lane);
    __builtin_amdgcn_wave_barrier();
    uint32_t K = 0;                                // live nodes with x = 1
    for (uint32_t j = 0; j < W; ++j) {
      const uint64_t xw = X1[j];
      K += (uint32_t)__builtin_popcountll(xw);
    }
    K = uni(K);
    uint64_t dec = 0ull;
    uint32_t R = 0;
    bool all_dec = false;
    for (uint32_t r = 1; r <= p.k_max; ++r) {
      // ---- R-phase ("proposal phase", node.ts:46-82): c1 ~ HG(m, K, q) per receiver
      const uint32_t loR = K + q > m ? K + q - m : 0u;
      uint32_t n = 0, steps = 0;
      if (K != 0u && K != m && m != q) {
        n = stage_row(row, p.tally_off, p.tally_thr, p.tally_cap, K, lane);
        steps = search_steps(n);
      }
      uint64_t uP[WT];
      uint32_t KP = 0;                             // live nodes proposing 1
      // The lane id and the group count are laundered once per phase: the
      // unrolled groups' compares (c < m, j < W) would otherwise be hoisted out
      // of the round loop, one SGPR pair each per group, and spill.
      uint32_t ln = lane, Wr = W;
      asm volatile("" : "+v"(ln), "+s"(Wr));
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        if ((uint32_t)j < Wr) {
          // the round's block of receiver c: u_R = out[1] << 32 | out[0], u_P = out[3] << 32 | out[2]
          const uint32_t c = (uint32_t)j * 64u + ln;
          const uint4 b = philox4x32_10(k0, k1, make_uint4(tlo, thi, c, (r - 1u) | (kStreamTally << 24)));
          uP[j] = (uint64_t)b.w << 32 | b.z;
          uint32_t c1 = loR;
          if (n != 0u) c1 += count_le(row, n, steps, (uint64_t)b.y << 32 | b.x);
          const uint64_t prop = ballot(c < m && 2u * c1 > q);   // c1 > c0 = q - c1 (q odd: no tie)
          KP += (uint32_t)__builtin_popcountll(prop);
        }
      }
      KP = uni(KP);
      // ---- P-phase ("voting phase", node.ts:83-158): c1 ~ HG(m, K', q) per receiver
      const uint32_t loP = KP + q > m ? KP + q - m : 0u;
      n = 0, steps = 0;
      if (KP != 0u && KP != m && m != q) {
        n = stage_row(row, p.tally_off, p.tally_thr, p.tally_cap, KP, lane);
        steps = search_steps(n);
      }
      uint32_t Kn = 0;
      ln = lane, Wr = W;
      asm volatile("" : "+v"(ln), "+s"(Wr));
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        if ((uint32_t)j < Wr) {
          uint32_t c1 = loP;
          if (n != 0u) c1 += count_le(row, n, steps, uP[j]);
          const uint32_t c0 = q - c1;
          const bool d0l = c0 > F, d1l = !d0l && c1 > F;
          const uint64_t x1 = ballot((uint32_t)j * 64u + ln < m && !d0l && (d1l || c1 > c0));
          if (lane == 0) X1[j] = x1;
          Kn += (uint32_t)__builtin_popcountll(x1);
          if (d0l || d1l) dec |= 1ull << j;        // sticky
        }
      }
      K = uni(Kn);
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

// Receiver groups the kernel is unrolled for (its u_P registers): the smallest instantiation that holds W.
uint32_t tally_groups(uint32_t W) { return W <= 1u ? 1u : W <= 4u ? 4u : W <= 16u ? 16u : W <= 32u ? 32u : 64u; }

// f(the instantiation that serves W).
template <class F>
auto with_kernel(uint32_t W, F f) {
  switch (tally_groups(W)) {
    case 1: return f(benor_tally_kernel<1>);
    case 4: return f(benor_tally_kernel<4>);
    case 16: return f(benor_tally_kernel<16>);
    case 32: return f(benor_tally_kernel<32>);
    default: return f(benor_tally_kernel<64>);
  }
}

}  // namespace

// Workgroups of this shape's kernel that one CU holds at once (registers and
// LDS; 0 = unknown): the u_P registers grow with the unroll, and a grid larger
// than what is resident runs its surplus workgroups as a second, emptier pass.
int tally_blocks_per_cu(const KParams &p) {
  return with_kernel(p.W, [&](auto kernel) { return blocks_per_cu(kernel, p); });
}

hipError_t launch_tally(const KParams &p, int grid, hipStream_t s) {
  if (!p.tally_off || !p.tally_thr || p.W > kMaxW || p.wave_bytes < tally_wave_bytes(p.W, p.tally_cap))
    return hipErrorInvalidValue;
  return with_kernel(p.W, [&](auto kernel) { return launch_lds(kernel, p, grid, s); });
}

}  // namespace benor
