// benor_mfma_strip.h -- the strip form of the matrix-core kernel's paired KIND 0
// form (benor_mfma.h, STRIP): which shapes take it, the lane maps of the two
// product shapes, the row swap that turns one into the other, and the live-row
// masks of the strip's packed proposals.  Plain C++ (no HIP header), so a host
// program can include it and model the 64 lanes (tests/strip_layout_check.cpp).
#pragma once

#include <stdint.h>

#include "benor_mfma_pair.h"

namespace benor {
namespace stripf {

constexpr int kMinW = 5;       // the W <= 4 interleaved form has no strip
constexpr int kRows = 16;      // receiver rows of the 16-row product
// The planner takes the form from this W on: measured against the 32-row form
// in one process, the strip's range of times lies wholly below the other's at
// W = 7 .. 16; at W = 5 and 6 the medians gain as much (0.984, 0.989) but the
// ranges overlap (profiles/r18_mfma_strip_ab_w.jsonl), so there it stays
// behind BENOR_MFMA_STRIP=1.
constexpr int kPlannedMinW = 7;

// 32-receiver tiles of a shape (W chunks of 64 senders; the last chunk may
// hold <= 32) and the live rows of the last one, 1..32.
BENOR_PAIR_HD constexpr uint32_t tiles(uint32_t W, uint32_t m) { return 2u * W - (m <= 64u * (W - 1u) + 32u ? 1u : 0u); }
BENOR_PAIR_HD constexpr uint32_t last_rows(uint32_t W, uint32_t m) { return m - 32u * (tiles(W, m) - 1u); }
BENOR_PAIR_HD constexpr bool eligible(uint32_t W, uint32_t m) { return W >= (uint32_t)kMinW && last_rows(W, m) <= (uint32_t)kRows; }
BENOR_PAIR_HD constexpr bool planned(uint32_t W, uint32_t m) { return W >= (uint32_t)kPlannedMinW && eligible(W, m); }

// Lane maps.  32-row shape (v_mfma_scale_f32_32x32x64_f8f6f4): lane l brings
// trial column l & 31 and the 32 senders of word 2c + (l >> 5) of chunk c;
// result j is row (j & 3) + 8 (j >> 2) + 4 (l >> 5).  16-row shape
// (..._16x16x128_...): column l & 15, K block l >> 4 of 32 senders; result j
// is row 4 (l >> 4) + j.
BENOR_PAIR_HD constexpr uint32_t col32(uint32_t l) { return l & 31u; }
BENOR_PAIR_HD constexpr uint32_t row32(uint32_t l, uint32_t j) { return (j & 3u) + 8u * (j >> 2) + 4u * (l >> 5); }
BENOR_PAIR_HD constexpr uint32_t col16(uint32_t l) { return l & 15u; }
BENOR_PAIR_HD constexpr uint32_t row16(uint32_t l, uint32_t j) { return 4u * (l >> 4) + j; }

// v_permlane16_swap_b32 a, b over the 64 lanes: the odd 16-lane rows of a
// trade places with the even rows of b.
template <typename T>
inline void row_swap_model(T (&a)[64], T (&b)[64]) {
  for (uint32_t l = 16; l < 64; l += 32)
    for (uint32_t i = 0; i < 16; ++i) {
      const T t = a[l + i];
      a[l + i] = b[l - 16 + i];
      b[l - 16 + i] = t;
    }
}

// After the swap back, packed word w (0, 1) of a lane in half h = l >> 5
// holds rows 8h + 4w + i of the last tile in the low nibbles i = 0..3
// (pairf::nib_lo): the rows below `rows` are live.
BENOR_PAIR_HD constexpr uint32_t live_mask(uint32_t rows, uint32_t h, uint32_t w) {
  uint32_t mask = 0;
  for (uint32_t i = 0; i < 4; ++i)
    if (8u * h + 4u * w + i < rows) mask |= pairf::nib_lo((int)i);
  return mask;
}

}  // namespace stripf
}  // namespace benor
