// Host check of the per-wave LDS layouts in csrc/benor_tally_common.h
// (tests/test_tally_layout.py builds and runs it; plain C++, so it can also be
// built with -fsanitize=address,undefined by hand).
//
// The kernels take their region pointers and the host its sizes from one
// function, plane_layout.  Swept over every W, a set of caps and schedule
// lengths around the layout's branch points, both schedule kinds, batch and
// state launches, with and without the crasher list:
//   * every region starts on 8 bytes, WB (written as uint4) and the wave's
//     stride on 16;
//   * the regions are pairwise disjoint, apart from the two documented
//     aliases: X0 on P0 in a batch launch, WB inside `row` when 2 capE >= 256;
//   * the last region ends at or below what the size functions give the host.
#include <cstdint>
#include <cstdio>

#include "benor.h"
#include "benor_tally_common.h"

namespace {

constexpr uint32_t kMaxW = BO_MAX_N / 64;
unsigned long checks = 0, failures = 0;

struct Region {
  const char *name;
  uint32_t at, bytes;
};

struct Case {
  uint32_t W, cap, ncr;
  bool random, states, cl;
};

void expect(bool ok, const char *what, const char *a, const char *b, const Case &c) {
  ++checks;
  if (ok) return;
  ++failures;
  std::fprintf(stderr, "FAIL %s %s %s: W=%u cap=%u ncr=%u random=%d states=%d cl=%d\n", what, a, b, c.W, c.cap, c.ncr,
               c.random, c.states, c.cl);
}

void check(const benor::PlaneLayout &L, const Case &c, bool own_x0, uint32_t size) {
  const uint32_t capE = (c.cap + 1u) & ~1u;
  const Region r[] = {{"AL", L.AL, c.W * 8u},
                      {"X1", L.X1, c.W * 8u},
                      {"P1", L.P1, c.W * 8u},
                      {"P0", L.P0, c.W * 8u},
                      {"X0", L.X0, c.W * 8u},
                      {"DEC", L.DEC, c.states ? c.W * 8u : 0u},
                      {"row", L.row, c.cap * 8u},
                      {"WB", L.WB, c.random ? benor::kSchedWords * 4u : 0u},
                      {"SC", L.SC, c.ncr * 4u},
                      {"CL", L.CL, c.cl ? c.ncr * 4u : 0u}};
  constexpr int n = sizeof r / sizeof r[0];
  const bool wb_in_row = 2u * capE >= benor::kSchedWords;
  for (int i = 0; i < n; ++i) {
    expect(r[i].at % 8u == 0u, "alignment 8 of", r[i].name, "", c);
    expect(r[i].at + r[i].bytes <= size, "end beyond the size function of", r[i].name, "", c);
    for (int j = i + 1; j < n; ++j) {
      const bool overlap = r[i].bytes && r[j].bytes && r[i].at < r[j].at + r[j].bytes && r[j].at < r[i].at + r[i].bytes;
      const bool x0_on_p0 = r[i].name[0] == 'P' && r[i].name[1] == '0' && r[j].name[0] == 'X' && !own_x0;
      const bool wb_on_row = r[i].name[0] == 'r' && r[j].name[0] == 'W' && wb_in_row;
      if (x0_on_p0) expect(r[i].at == r[j].at, "alias", r[i].name, r[j].name, c);
      else if (wb_on_row) expect(r[j].at == r[i].at && r[j].bytes <= capE * 8u, "alias", r[i].name, r[j].name, c);
      else expect(!overlap, "overlap of", r[i].name, r[j].name, c);
    }
  }
  expect(L.WB % 16u == 0u, "alignment 16 of", "WB", "", c);
  expect(L.end <= size && L.end % 8u == 0u, "size function below", "end", "", c);
}

}  // namespace

int main() {
  const uint32_t caps[] = {0u, 1u, 2u, 63u, 127u, 128u, 2047u};
  const uint32_t ncrs[] = {0u, 1u, 3u, 4u, 65u, 4095u};
  for (uint32_t W = 1u; W <= kMaxW; ++W) {
    // a state launch's stride stays a multiple of 16 bytes over the plan's rounded batch stride
    const Case w{W, 0u, 0u, false, true, false};
    expect(benor::crash_state_bytes(W) % 16u == 0u && benor::byz_state_bytes(W) % 16u == 0u, "stride 16 of", "state bytes",
           "", w);
    for (uint32_t cap : caps) {
      for (int states = 0; states < 2; ++states) {
        const Case b{W, cap, 0u, false, states != 0, false};
        check(benor::byz_layout(W, cap, b.states), b, false,
              benor::byz_wave_bytes(W, cap) + (b.states ? benor::byz_state_bytes(W) : 0u));
        for (uint32_t ncr : ncrs)
          for (int random = 0; random < 2; ++random)
            for (int cl = 0; cl < 2; ++cl) {
              const Case c{W, cap, ncr, random != 0, states != 0, cl != 0};
              check(benor::crash_layout(W, cap, ncr, c.random, c.states, c.cl), c, c.states,
                    benor::crash_wave_bytes(W, cap, ncr, c.random, c.cl) + (c.states ? benor::crash_state_bytes(W) : 0u));
            }
      }
    }
  }
  std::printf("%lu checks, %lu failures\n", checks, failures);
  return failures ? 1 : 0;
}
