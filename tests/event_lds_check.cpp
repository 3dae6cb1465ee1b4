// Host check of the workgroup-batched event kernel's sizing (csrc/benor_event_sizes.h; tests/test_event_order.py
// builds and runs it; plain C++, so it can also be built with -fsanitize=address,undefined by hand).
//
// The planner, the launcher and the kernel's carve-up read one set of functions.  Without arguments, swept over every
// N, the planner's wave count and the four forced ones, and random /stop schedules from none to N stops:
//   * the regions, laid out in the kernel's order with the kernel's alignments, end at or below event_wg_bytes;
//   * the hash table has 8, 4 or 2 slots per event lane, a power of two of them, and a factor above 2 only where the
//     workgroup then stays at or below kEventWgLdsTarget;
//   * event_wg_fits is exactly "the workgroup is at most kEventWgLdsLimit", and the limit is the device's 160 KiB;
//   * with no random schedule every shape fits: what a live run and an explicit schedule can plan.
// `bounds`: the sizes at which the sizing takes another path, for the generator of tests/test_event_order.py.
// `size N m forced rstops ...`: one line per quadruple, "N W factor slots pool_in_lds bytes fits pool_regs one_register".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "benor_event_sizes.h"

namespace {

constexpr uint32_t kMaxN = 4096u;
unsigned long checks = 0, failures = 0;

void expect(bool ok, const char *what, uint32_t N, uint32_t W, uint32_t r) {
  ++checks;
  if (ok) return;
  ++failures;
  std::fprintf(stderr, "FAIL %s: N=%u W=%u rstops=%u\n", what, N, W, r);
}

// The kernel's carve-up (benor_event_wg_kernel): each region where the one before it ends.
uint32_t carved(uint32_t N, uint32_t W, uint32_t HS, uint32_t cap, uint32_t r) {
  const uint32_t T = 64u * W;
  uint32_t at = (benor::kEventWgCtlBytes + 15u) & ~15u;
  at += 8u * 2u * N;                      // ibox
  at += 8u * 64u * 2u + 8u * 256u;        // killed, decided, comp
  at += 8u * HS + 8u * 64u + 8u * r;      // ht, rset, rstops
  at += 4u * 2u * N + 3u * 4u * T;        // smax; bmax, nxt, tvs
  at += 2u * ((N + 7u) & ~7u) * 2u;       // ks, cidx
  at += (N + 15u) & ~15u;                 // xs
  if (benor::event_wg_pool_in_lds(cap)) at += 4u * cap;
  return at;
}

void check(uint32_t N, uint32_t forced, uint32_t r) {
  const uint32_t W = benor::event_wg_waves_for(N, forced), cap = benor::event_pool_cap(N);
  const uint32_t f = benor::event_wg_slot_factor(N, W, cap, r), HS = benor::event_wg_slots(N, W, cap, r);
  const uint32_t bytes = benor::event_wg_total_bytes(N, W, cap, r);
  expect(W == 1u || W == 3u || W == 7u || W == 15u, "wave count", N, W, r);
  expect(f == 8u || f == 4u || f == 2u, "slot factor", N, W, r);
  expect(HS >= f * 64u * W && HS < 2u * f * 64u * W && (HS & (HS - 1u)) == 0u, "slots: a power of two", N, W, r);
  expect(HS >= 2u * 64u * W, "two slots per event lane at least", N, W, r);
  expect(f == 2u || bytes <= benor::kEventWgLdsTarget, "a larger table only below the target", N, W, r);
  expect(f == 8u || benor::event_wg_bytes(N, W, benor::event_pow2_ceil(2u * f * 64u * W), cap, r) > benor::kEventWgLdsTarget,
         "the largest table the target allows", N, W, r);
  expect(carved(N, W, HS, cap, r) <= bytes, "the carve-up ends inside the size", N, W, r);
  expect(bytes % 8u == 0u, "size a multiple of 8", N, W, r);
  expect(benor::event_wg_fits(N, W, cap, r) == (bytes <= benor::kEventWgLdsLimit), "fits = within the limit", N, W, r);
  if (r == 0u) expect(benor::event_wg_fits(N, W, cap, r), "no random schedule: every shape fits", N, W, r);
}

uint32_t factor15(uint32_t N) { return benor::event_wg_slot_factor(N, 15u, benor::event_pool_cap(N), 0u); }

}  // namespace

int main(int argc, char **argv) {
  static_assert(benor::kEventWgLdsLimit == 160u * 1024u, "gfx950: 160 KiB of LDS per workgroup");
  static_assert(benor::kEventWgLdsTarget < benor::kEventWgLdsLimit, "the target leaves room below the limit");
  if (argc > 1 && std::strcmp(argv[1], "size") == 0) {
    for (int i = 2; i + 3 < argc; i += 4) {
      const uint32_t N = (uint32_t)std::atoi(argv[i]), m = (uint32_t)std::atoi(argv[i + 1]);
      const uint32_t forced = (uint32_t)std::atoi(argv[i + 2]), r = (uint32_t)std::atoi(argv[i + 3]);
      const uint32_t W = benor::event_wg_waves_for(N, forced), cap = benor::event_pool_cap(N);
      std::printf("%u %u %u %u %d %u %d %u %d\n", N, W, benor::event_wg_slot_factor(N, W, cap, r),
                  benor::event_wg_slots(N, W, cap, r), benor::event_wg_pool_in_lds(cap) ? 1 : 0,
                  benor::event_wg_total_bytes(N, W, cap, r), benor::event_wg_fits(N, W, cap, r) ? 1 : 0,
                  benor::event_reg_pool_regs(cap), benor::event_reg_one_register(m, N) ? 1 : 0);
    }
    return 0;
  }
  if (argc > 1 && std::strcmp(argv[1], "bounds") == 0) {
    uint32_t pool = 0, f8 = 0, f4 = 0, stops = 0;
    for (uint32_t N = 1u; N <= kMaxN; ++N) {
      if (benor::event_wg_pool_in_lds(benor::event_pool_cap(N))) pool = N;
      if (factor15(N) == 8u) f8 = N;
      if (factor15(N) >= 4u) f4 = N;
    }
    for (uint32_t r = 0u; r <= kMaxN; ++r)
      if (benor::event_wg_fits(kMaxN, 15u, benor::event_pool_cap(kMaxN), r)) stops = r;
    std::printf("pool_lds_max_n %u\n", pool);
    for (uint32_t N = 1u; N < kMaxN; ++N)
      if (benor::event_wg_waves_for(N, 0u) != benor::event_wg_waves_for(N + 1u, 0u)) std::printf("waves_step %u\n", N);
    std::printf("slots8_max_n %u\nslots4_max_n %u\nmax_n %u\nmax_n_stops %u\n", f8, f4, kMaxN, stops);
    return 0;
  }
  const uint32_t forced[] = {0u, 1u, 3u, 7u, 15u};
  for (uint32_t N = 1u; N <= kMaxN; ++N)
    for (uint32_t fw : forced) {
      const uint32_t rs[] = {0u, 1u, 2u, 63u, 64u, 65u, N / 3u, N / 2u, 1500u, 1600u, 1650u, 1700u, 1800u, 2048u, N - 1u, N};
      for (uint32_t r : rs)
        if (r <= N) check(N, fw, r);
    }
  std::printf("%lu checks, %lu failures\n", checks, failures);
  return failures ? 1 : 0;
}
