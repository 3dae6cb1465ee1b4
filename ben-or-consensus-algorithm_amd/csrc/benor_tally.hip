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
#include "benor_device.h"

namespace benor {

namespace {

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// Row K of the table into the wave's LDS region; returns its width (<= cap).
__device__ __forceinline__ uint32_t stage_row(uint64_t *__restrict__ row, const KParams &p, uint32_t K,
                                              uint32_t lane) {
  const uint32_t o = uni(p.tally_off[K]);
  uint32_t n = uni(p.tally_off[K + 1u]) - o;
  if (n > p.tally_cap) n = p.tally_cap;            // the region's size (the host table never exceeds it)
  const unsigned long long *src = p.tally_thr + o;
  for (uint32_t i = lane; i < n; i += 64u) row[i] = src[i];
  __builtin_amdgcn_wave_barrier();                 // a wave's LDS operations retire in order
  return n;
}

// #{ j < n : T[j] <= u }: `steps` = ceil(log2(n + 1)) wave-uniform steps.
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
        n = stage_row(row, p, K, lane);
        steps = 32u - (uint32_t)__builtin_clz(n | 1u);
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
          if (n != 0u) c1 += row_count(row, n, steps, (uint64_t)b.y << 32 | b.x);
          const uint64_t prop = ballot(c < m && 2u * c1 > q);   // c1 > c0 = q - c1 (q odd: no tie)
          KP += (uint32_t)__builtin_popcountll(prop);
        }
      }
      KP = uni(KP);
      // ---- P-phase ("voting phase", node.ts:83-158): c1 ~ HG(m, K', q) per receiver
      const uint32_t loP = KP + q > m ? KP + q - m : 0u;
      n = 0, steps = 0;
      if (KP != 0u && KP != m && m != q) {
        n = stage_row(row, p, KP, lane);
        steps = 32u - (uint32_t)__builtin_clz(n | 1u);
      }
      uint32_t Kn = 0;
      ln = lane, Wr = W;
      asm volatile("" : "+v"(ln), "+s"(Wr));
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        if ((uint32_t)j < Wr) {
          uint32_t c1 = loP;
          if (n != 0u) c1 += row_count(row, n, steps, uP[j]);
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

template <int WT>
hipError_t launch_wt(const KParams &p, int grid, hipStream_t s) {
  const void *fn = reinterpret_cast<const void *>(&benor_tally_kernel<WT>);
  if (p.lds_bytes > 64u * 1024u) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((benor_tally_kernel<WT>), dim3(grid), dim3(64 * kWavesPerBlock), p.lds_bytes, s, p);
  return hipGetLastError();
}

// Receiver groups the kernel is unrolled for (its u_P registers): the smallest instantiation that holds W.
uint32_t tally_groups(uint32_t W) { return W <= 1u ? 1u : W <= 4u ? 4u : W <= 16u ? 16u : W <= 32u ? 32u : 64u; }

template <int WT>
int blocks_per_cu_wt(const KParams &p) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, benor_tally_kernel<WT>, 64 * kWavesPerBlock,
                                                                    p.lds_bytes);
  return e == hipSuccess ? n : 0;
}

}  // namespace

uint32_t tally_wave_bytes(uint32_t W, uint32_t cap) { return (((W + 1u) & ~1u) + cap) * 8u; }

// Workgroups of this shape's kernel that one CU holds at once (registers and
// LDS; 0 = unknown): the u_P registers grow with the unroll, and a grid larger
// than what is resident runs its surplus workgroups as a second, emptier pass.
int tally_blocks_per_cu(const KParams &p) {
  switch (tally_groups(p.W)) {
    case 1: return blocks_per_cu_wt<1>(p);
    case 4: return blocks_per_cu_wt<4>(p);
    case 16: return blocks_per_cu_wt<16>(p);
    case 32: return blocks_per_cu_wt<32>(p);
    default: return blocks_per_cu_wt<64>(p);
  }
}

hipError_t launch_tally(const KParams &p, int grid, hipStream_t s) {
  if (!p.tally_off || !p.tally_thr || p.W > kMaxW || p.wave_bytes < tally_wave_bytes(p.W, p.tally_cap))
    return hipErrorInvalidValue;
  switch (tally_groups(p.W)) {
    case 1: return launch_wt<1>(p, grid, s);
    case 4: return launch_wt<4>(p, grid, s);
    case 16: return launch_wt<16>(p, grid, s);
    case 32: return launch_wt<32>(p, grid, s);
    default: return launch_wt<64>(p, grid, s);
  }
}

}  // namespace benor
