// Host check of the paired KIND 0 form's bit-field arithmetic
// (csrc/benor_mfma_pair.h), in the f32 arithmetic the accumulator uses: the
// bias, then the low tile's products at scale 1 and the high tile's at scale
// 2^S, added 64 senders at a time as the kernel's product chain adds them.
// Lockstep GPU runs carry equal counts in both fields; this program runs every
// combination of the extreme and threshold counts in the two fields.
// Built and run by tests/test_mfma_pair.py; exit status 0 = no mismatch.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "benor_mfma_pair.h"

using namespace benor::pairf;

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// C + scale * count, one chunk of <= 64 unit products per step.
static float chain(float acc, uint32_t count, float scale) {
  while (count) {
    const uint32_t k = count < 64u ? count : 64u;
    volatile float step = acc + scale * (float)k;   // volatile: rounded to f32 at every step
    acc = step;
    count -= k;
  }
  return acc;
}

static long failures = 0, cases = 0;

static void fail(const char *what, uint32_t a, uint32_t b, uint32_t ca, uint32_t cb) {
  if (failures++ < 20) std::fprintf(stderr, "%s: (%u, %u) counts (%u, %u)\n", what, a, b, ca, cb);
}

// One accumulator: fields of `shift`, indicator bit `k` in each, threshold thr.
static uint32_t run(float bias, uint32_t bias_int, int shift, int k, uint32_t thr, uint32_t ca, uint32_t cb, bool lone,
                    const char *what, uint32_t p0, uint32_t p1) {
  float acc = chain(bias, ca, 1.0f);
  if (!lone) acc = chain(acc, cb, (float)(1u << shift));
  const uint64_t want = (uint64_t)bias_int + ca + (lone ? 0u : ((uint64_t)cb << shift));
  ++cases;
  if (want >= (1u << 24)) fail("field sum reaches 2^24", p0, p1, ca, cb);
  if (acc != (float)want || (double)acc != (double)want) fail("accumulation not exact", p0, p1, ca, cb);
  const uint32_t u = bits(acc);
  if ((u & 0x7FFFFFu) != (uint32_t)(want - kBase)) fail("mantissa is not the integer", p0, p1, ca, cb);
  if (((u >> k) & 1u) != (ca >= thr ? 1u : 0u)) fail(what, p0, p1, ca, cb);
  const uint32_t hi = (u >> (k + shift)) & 1u;
  if (k + shift != 21) fail("high indicator is not bit 21", p0, p1, ca, cb);
  if (hi != (!lone && cb >= thr ? 1u : 0u)) fail(what, p0, p1, ca, cb);
  return u;
}

int main() {
  static_assert(kIndR == ((1u << 9) | (1u << 21)) && kIndP == ((1u << 10) | (1u << 21)), "indicator bits");
  static_assert(kMaskX == 0x20200202u && kMaskY == 0x02022020u && (kMaskX & kMaskY) == 0u, "packing masks");
  // R-phase: every odd binary vote count
  for (uint32_t M1 = 1; M1 <= 1023; M1 += 2) {
    const uint32_t t = thr_r(M1), cs[4] = {0u, t - 1u, t, M1};
    if (bias_r2(M1) != (float)bias_r2_int(M1) || bits(bias_r2(M1)) != (0x4B000000u | (bias_r2_int(M1) - kBase)))
      fail("R bias", M1, 0, 0, 0);
    uint32_t u[16], want_lo[16], want_hi[16];
    int n = 0;
    for (uint32_t ca : cs)
      for (uint32_t cb : cs) {
        want_lo[n] = ca >= t;
        want_hi[n] = cb >= t;
        u[n++] = run(bias_r2(M1), bias_r2_int(M1), kShiftR, 9, t, ca, cb, false, "R indicator", M1, t);
        const uint32_t l = run(bias_r2(M1), bias_r2_int(M1), kShiftR, 9, t, ca, cb, true, "R indicator (lone tile)", M1, t);
        if (pack4_model(l, l, l, l) & 0xF0F0F0F0u) fail("lone tile sets a high nibble", M1, t, ca, cb);
      }
    // the packed dword: every group of four results, every rotation of it
    for (int g = 0; g < 16; ++g)
      for (int s = 1; s < 16; s += 5) {
        const int i[4] = {g, (g + s) & 15, (g + 2 * s) & 15, (g + 3 * s) & 15};
        const uint32_t d = pack4_model(u[i[0]], u[i[1]], u[i[2]], u[i[3]]);
        uint32_t want = 0;
        for (int r = 0; r < 4; ++r) want |= (want_lo[i[r]] ? nib_lo(r) : 0u) | (want_hi[i[r]] ? nib_hi(r) : 0u);
        ++cases;
        if (d & ~0x22222222u) fail("packed dword holds other bits than e2m1 1.0", M1, t, d, 0);
        if (d != want) fail("packed dword", M1, t, d, want);
      }
  }
  // the eight nibble positions are distinct
  uint32_t all = 0;
  for (int r = 0; r < 4; ++r) {
    if ((all & (nib_lo(r) | nib_hi(r))) || nib_lo(r) == nib_hi(r)) fail("nibble positions overlap", r, 0, 0, 0);
    all |= nib_lo(r) | nib_hi(r);
  }
  if (all != 0x22222222u) fail("nibble positions do not cover the dword", all, 0, 0, 0);
  // P-phase: every odd m, F at the ends and inside 2F < m
  for (uint32_t m = 65; m <= 1023; m += 2) {
    const uint32_t Fs[4] = {0u, 1u, (m - 1u) / 3u, (m - 1u) / 2u};
    for (uint32_t F : Fs) {
      const uint32_t thr = thr_p(m, F), cs[4] = {0u, thr - 1u, thr, m};
      if (bias_p2(m, F) != (float)bias_p2_int(m, F)) fail("P bias", m, F, 0, 0);
      for (uint32_t ca : cs)
        for (uint32_t cb : cs) {
          const uint32_t u = run(bias_p2(m, F), bias_p2_int(m, F), kShiftP, 10, thr, ca, cb, false, "P indicator", m, F);
          if (((u & kIndP) != 0u) != (ca >= thr || cb >= thr)) fail("P any-1 fold", m, F, ca, cb);
          if (((~u & kIndP) != 0u) != (ca < thr || cb < thr)) fail("P any-0 fold", m, F, ca, cb);
          const uint32_t l = run(bias_p2(m, F), bias_p2_int(m, F), kShiftP, 10, thr, ca, cb, true, "P indicator (lone tile)", m, F);
          if (((l & kIndP) != 0u) != (ca >= thr)) fail("P any-1 fold (lone tile)", m, F, ca, cb);
          if (((~(l | kIndPHigh) & kIndP) != 0u) != (ca < thr)) fail("P any-0 fold (lone tile)", m, F, ca, cb);
        }
    }
  }
  std::printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
