// benor_mfma_pair.h -- constants of the matrix-core kernel's paired KIND 0 form
// (benor_mfma.h): two 32-receiver tiles share one f32 accumulator, each
// tile's count in a bit field of its own.  Plain C++ (no HIP header), so a
// host program can include it and check the arithmetic (tests/pair_fields_check.cpp).
//
// An accumulator starts at 2^23 + b (1 + 2^S) and receives the low tile's
// products at scale 2^0 and the high tile's at scale 2^S, so it ends at the
// integer 2^23 + (b + c_lo) + 2^S (b + c_hi) < 2^24: exact in f32, and its
// mantissa bits are that integer's.  With b = 2^k - thr, bit k of a field is
// "count >= thr" as long as b + count < 2^(k+1):
//  * R-phase: S = 12, k = 9, thr = t = floor(M1 / 2) + 1 (M1 <= 1023 odd binary
//    votes): b + c <= 2^9 + (M1 - 1) / 2 < 2^10.  Bits 9 / 21 = proposal 1.
//  * P-phase: S = 11, k = 10, thr = m - F (<= 1023; 2F < m): b + c <= 2^10 + F
//    < 2^11.  Bits 10 / 21 = decide 1; clear = decide 0.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BENOR_PAIR_HD __host__ __device__
#else
#define BENOR_PAIR_HD
#endif

namespace benor {
namespace pairf {

constexpr int kShiftR = 12;                       // high tile's A scale, R-phase
constexpr int kShiftP = 11;                       // ... P-phase
constexpr uint32_t kBase = 1u << 23;              // ulp 1 on [2^23, 2^24)
constexpr uint32_t kIndR = (1u << 9) | (1u << 21);    // proposal-1 bits (byte 1 bit 1, byte 2 bit 5)
constexpr uint32_t kIndP = 0x00200400u;           // decide-1 bits 10 and 21
constexpr uint32_t kIndPHigh = 0x00200000u;       // the high field's
// Packing four results u0..u3 into one B-operand dword (eight e2m1 nibbles,
// 1.0 = 0x2 where the receiver proposes 1): X = bytes [b1(u0), b1(u1), b2(u0),
// b2(u1)], Y = bytes [b2(u2), b2(u3), b1(u2), b1(u3)] (v_perm_b32 selectors,
// source {u_odd : u_even}), out = (X & kMaskX) | (Y & kMaskY): the low tile's
// receivers in the low nibbles of bytes 0, 1 (u0, u1) and 2, 3 (u2, u3), the
// high tile's in the high nibbles of bytes 2, 3 (u0, u1) and 0, 1 (u2, u3).
constexpr uint32_t kSelX = 0x06020501u, kSelY = 0x05010602u;
constexpr uint32_t kMaskX = 0x20200202u, kMaskY = 0x02022020u;

BENOR_PAIR_HD constexpr uint32_t thr_r(uint32_t M1) { return (M1 >> 1) + 1u; }
BENOR_PAIR_HD constexpr uint32_t thr_p(uint32_t m, uint32_t F) { return m - F; }

// Initial accumulator values as integers (< 2^24) and as the f32 the kernel loads.
BENOR_PAIR_HD constexpr uint32_t bias_r2_int(uint32_t M1) { return kBase + ((1u << 9) - thr_r(M1)) * (1u + (1u << kShiftR)); }
BENOR_PAIR_HD constexpr uint32_t bias_p2_int(uint32_t m, uint32_t F) {
  return kBase + ((1u << 10) - thr_p(m, F)) * (1u + (1u << kShiftP));
}
BENOR_PAIR_HD constexpr float bias_r2(uint32_t M1) { return (float)bias_r2_int(M1); }
BENOR_PAIR_HD constexpr float bias_p2(uint32_t m, uint32_t F) { return (float)bias_p2_int(m, F); }

// v_perm_b32 for selectors 0..7 (bytes 0..3 of lo, 4..7 of hi).
BENOR_PAIR_HD constexpr uint32_t perm_bytes(uint32_t hi, uint32_t lo, uint32_t sel) {
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t s = (sel >> (8 * i)) & 7u;
    r |= (((s < 4u ? lo : hi) >> (8u * (s & 3u))) & 0xFFu) << (8 * i);
  }
  return r;
}

// The packing as the kernel computes it (there through __builtin_amdgcn_perm).
BENOR_PAIR_HD constexpr uint32_t pack4_model(uint32_t u0, uint32_t u1, uint32_t u2, uint32_t u3) {
  return (perm_bytes(u1, u0, kSelX) & kMaskX) | (perm_bytes(u3, u2, kSelY) & kMaskY);
}

// Nibble of result i (0..3) of a packed dword: the low tile's / the high tile's.
BENOR_PAIR_HD constexpr uint32_t nib_lo(int i) { return 0x02u << (8 * i); }
BENOR_PAIR_HD constexpr uint32_t nib_hi(int i) { return 0x20u << (8 * ((i + 2) & 3)); }

}  // namespace pairf
}  // namespace benor
