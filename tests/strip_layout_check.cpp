// Host model of the strip form of the paired KIND 0 matrix-core kernel
// (csrc/benor_mfma.h STRIP, csrc/benor_mfma_strip.h): the 64 lanes, the two
// product shapes' lane maps and the row swap between them, with every operand
// nibble carried as a label instead of a vote.  For every eligible (W, tile
// parity, live rows of the last tile <= 16) it checks that
//  * every (trial, sender) enters the R-phase strip exactly once, in its
//    trial's column;
//  * every (trial, proposal), the strip's rows included, enters each main
//    P-phase product and the strip's exactly once, and no padded row does;
//  * the strip's folded decisions reach the lanes of their own trial, for
//    trial counts that end inside a trial half too.
// Built and run by tests/test_mfma_strip.py; exit status 0 = no mismatch.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "benor_mfma_strip.h"

using namespace benor;

// One VGPR of a B operand over the wave: eight nibbles per lane, each empty
// (-1) or the label (trial << 16 | sender or receiver).
struct Reg {
  int32_t n[8];
};
typedef Reg Wave[64];
struct Frag {
  Wave v[4];
};

static long failures = 0, cases = 0;
static void fail(const char *what, unsigned W, unsigned m, unsigned a, unsigned b) {
  if (failures++ < 20) std::fprintf(stderr, "%s: W=%u m=%u (%u, %u)\n", what, W, m, a, b);
}

static void clear(Wave &w) { std::memset(w, 0xFF, sizeof(Wave)); }
static int nib_index(uint32_t bit) {   // e2m1 1.0 = 0x2 of nibble k
  for (int k = 0; k < 8; ++k)
    if (bit == (0x2u << (4 * k))) return k;
  return -1;
}

// strip_operands: chunks c, c + 1 (or zeros) -> lo (trials 0..15), hi (16..31)
static void strip_operands(std::vector<Frag> &x, size_t c, Frag &lo, Frag &hi) {
  for (int v = 0; v < 4; ++v) {
    std::memcpy(lo.v[v], x[c].v[v], sizeof(Wave));
    if (c + 1 < x.size()) std::memcpy(hi.v[v], x[c + 1].v[v], sizeof(Wave));
    else clear(hi.v[v]);
    stripf::row_swap_model(lo.v[v], hi.v[v]);
  }
}

// A 16-row product's B operand adds, into column col16(l) of trial half hh,
// every nibble of lane l: seen[trial][label] counts them.
static void feed16(const Frag &f, unsigned hh, std::vector<std::vector<int>> &seen, unsigned W, unsigned m, const char *what) {
  for (uint32_t l = 0; l < 64; ++l)
    for (int v = 0; v < 4; ++v)
      for (int k = 0; k < 8; ++k) {
        const int32_t id = f.v[v][l].n[k];
        if (id < 0) continue;
        const uint32_t trial = 16u * hh + stripf::col16(l);
        if ((uint32_t)(id >> 16) != trial) fail(what, W, m, trial, (uint32_t)id);
        else ++seen[trial][id & 0xFFFF];
      }
}
static void feed32(const Frag &f, std::vector<std::vector<int>> &seen, unsigned W, unsigned m, const char *what) {
  for (uint32_t l = 0; l < 64; ++l)
    for (int v = 0; v < 4; ++v)
      for (int k = 0; k < 8; ++k) {
        const int32_t id = f.v[v][l].n[k];
        if (id < 0) continue;
        if ((uint32_t)(id >> 16) != stripf::col32(l)) fail(what, W, m, stripf::col32(l), (uint32_t)id);
        else ++seen[stripf::col32(l)][id & 0xFFFF];
      }
}
static void expect_once(const std::vector<std::vector<int>> &seen, unsigned live, unsigned W, unsigned m, const char *what) {
  for (uint32_t t = 0; t < 32; ++t)
    for (uint32_t s = 0; s < seen[t].size(); ++s) {
      ++cases;
      if (seen[t][s] != (s < live ? 1 : 0)) fail(what, W, m, t, s);
    }
}

static void check_shape(unsigned W, unsigned m) {
  const unsigned MT = stripf::tiles(W, m), mrem = stripf::last_rows(W, m), MTM = MT - 1, KP = (MT + 1) / 2;
  // ---- R-phase operand: nibble i of VGPR v of chunk c = sender 32 (2c + h) + 4i + v
  std::vector<Frag> bx(W);
  for (unsigned c = 0; c < W; ++c)
    for (int v = 0; v < 4; ++v)
      for (uint32_t l = 0; l < 64; ++l)
        for (int i = 0; i < 8; ++i) {
          const uint32_t s = 32u * (2u * c + (l >> 5)) + 4u * i + v;
          bx[c].v[v][l].n[i] = s < m ? (int32_t)(stripf::col32(l) << 16 | s) : -1;   // senders >= m: zero bits
        }
  std::vector<std::vector<int>> seen(32, std::vector<int>(64 * W, 0));
  for (unsigned c = 0; c < W; c += 2) {
    Frag lo, hi;
    strip_operands(bx, c, lo, hi);
    feed16(lo, 0, seen, W, m, "R strip: sender in another trial's column");
    feed16(hi, 1, seen, W, m, "R strip: sender in another trial's column");
  }
  expect_once(seen, m, W, m, "R strip: sender not counted exactly once");

  // ---- proposals: pb[a][k] from the 32-row tiles, then the strip's
  std::vector<Frag> pb(KP);
  for (auto &f : pb)
    for (int v = 0; v < 4; ++v) clear(f.v[v]);
  for (unsigned a = 0; a < (MTM + 1) / 2; ++a)
    for (int k = 0; k < 4; ++k)
      for (uint32_t l = 0; l < 64; ++l)
        for (int i = 0; i < 4; ++i) {
          const uint32_t row = stripf::row32(l, 4 * k + i), t = stripf::col32(l);
          pb[a].v[k][l].n[nib_index(pairf::nib_lo(i))] = (int32_t)(t << 16 | (32u * (2u * a) + row));
          if (2 * a + 1 < MTM) pb[a].v[k][l].n[nib_index(pairf::nib_hi(i))] = (int32_t)(t << 16 | (32u * (2u * a + 1u) + row));
        }
  Wave q[2];
  for (unsigned hh = 0; hh < 2; ++hh) {
    clear(q[hh]);
    for (uint32_t l = 0; l < 64; ++l)
      for (uint32_t j = 0; j < 4; ++j)
        q[hh][l].n[nib_index(pairf::nib_lo((int)j))] =
            (int32_t)((16u * hh + stripf::col16(l)) << 16 | (32u * MTM + stripf::row16(l, j)));
  }
  stripf::row_swap_model(q[0], q[1]);
  for (unsigned w = 0; w < 2; ++w)
    for (uint32_t l = 0; l < 64; ++l) {
      const uint32_t live = stripf::live_mask(mrem, l >> 5, w);
      for (int k = 0; k < 8; ++k) {
        int32_t &id = q[w][l].n[k];
        if (id >= 0 && (uint32_t)(id & 0xFFFF) != 32u * MTM + 8u * (l >> 5) + 4u * w + (uint32_t)(k >> 1))
          fail("strip proposal is not the row its mask assumes", W, m, l, (uint32_t)id);
        if (!((live >> (4 * k + 1)) & 1u)) id = -1;
      }
      // placement: the high nibbles of dwords 0, 1 (MT even), or dwords 0, 1 of a free chunk
      for (int k = 0; k < 8; ++k) {
        if (q[w][l].n[k] < 0) continue;
        int32_t &slot = pb[KP - 1].v[w][l].n[(MTM & 1) ? k + 1 : k];
        if (slot >= 0) fail("strip proposal lands on a used nibble", W, m, l, (uint32_t)k);
        slot = q[w][l].n[k];
      }
    }
  // ---- P-phase: the main tiles read pb[] in the 32-trial layout, the strip after the swaps
  std::vector<std::vector<int>> pseen(32, std::vector<int>(32 * MT, 0));
  for (unsigned c = 0; c < KP; ++c) feed32(pb[c], pseen, W, m, "P main: proposal in another trial's column");
  expect_once(pseen, m, W, m, "P main: proposal not counted exactly once (or a padded row counted)");
  std::vector<std::vector<int>> sseen(32, std::vector<int>(32 * MT, 0));
  for (unsigned c = 0; c < KP; c += 2) {
    Frag lo, hi;
    strip_operands(pb, c, lo, hi);
    feed16(lo, 0, sseen, W, m, "P strip: proposal in another trial's column");
    feed16(hi, 1, sseen, W, m, "P strip: proposal in another trial's column");
  }
  expect_once(sseen, m, W, m, "P strip: proposal not counted exactly once (or a padded row counted)");

  // ---- fold: OR / AND words of the two halves, swapped, then the ballot
  // over lanes n and n + 32 -> bit n.  Label: the trial whose rows it folds.
  int32_t o[2][64];
  for (unsigned hh = 0; hh < 2; ++hh)
    for (uint32_t l = 0; l < 64; ++l) o[hh][l] = (int32_t)(16u * hh + stripf::col16(l));
  stripf::row_swap_model(o[0], o[1]);
  for (uint32_t l = 0; l < 64; ++l)
    for (unsigned w = 0; w < 2; ++w) {
      ++cases;
      if ((uint32_t)o[w][l] != stripf::col32(l)) fail("folded decision in another trial's lane", W, m, l, (uint32_t)o[w][l]);
    }
  // every strip row of a trial reaches one of its two lanes' folds: lane n
  // folds the rows of 16-layout lanes in rows 0 / 1 and 2 / 3 of both words
  for (unsigned count : {1u, 15u, 16u, 17u, 31u, 32u}) {
    uint32_t halt = 0, decided = 0;
    for (uint32_t l = 0; l < 64; ++l) {
      if (stripf::col32(l) < count) halt |= 1u << (l & 31u);
      decided |= 1u << (uint32_t)o[0][l];
    }
    ++cases;
    if ((decided & halt) != (count >= 32 ? ~0u : (1u << count) - 1u)) fail("trial count inside a half", W, m, count, decided & halt);
  }
}

int main() {
  unsigned shapes = 0;
  for (unsigned W = 2; W <= 16; ++W)
    for (unsigned m = 64 * (W - 1) + 1; m <= 64 * W && m <= 1023; m += 2) {   // KIND 0: m odd
      const bool want = W >= 5 && (m - 32 * (stripf::tiles(W, m) - 1)) <= 16;
      if (stripf::eligible(W, m) != want) fail("eligibility", W, m, 0, 0);
      if (stripf::tiles(W, m) != (m + 31) / 32) fail("tile count", W, m, 0, 0);
      if (stripf::planned(W, m) != (want && W >= 7)) fail("planner's rule", W, m, 0, 0);
      if (!stripf::eligible(W, m)) continue;
      ++shapes;
      check_shape(W, m);
    }
  // both tile parities and every odd live-row count occurred at every W
  if (shapes != 12u * 2u * 8u) fail("eligible shapes", shapes, 0, 0, 0);
  std::printf("%ld cases, %ld failures\n", cases, failures);
  return failures ? 1 : 0;
}
