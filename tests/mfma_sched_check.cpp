// Host check of csrc/benor_mfma_sched.h (tests/test_mfma_dynamic.py builds and
// runs it; plain C++, so it can also be built with -fsanitize=thread by hand).
//
// Claim protocol: 64 threads stand in for the waves of a launch and run
// sched::wave_run over std::atomic words, yielding at random.  Every group of
// [0, ngroups) must be visited exactly once, no wave may find the invariant
// broken, and both words must be 0 afterwards; each case runs three launches
// back to back on the same words (the threads of a launch are joined before
// the next one starts, as launches on one stream are ordered).
//
// Planner rule: the headline shape is dynamic with the chosen chunk, a small W
// and a short launch are static.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <random>
#include <thread>
#include <vector>

#include "benor_mfma_sched.h"

namespace {

struct Words {
  std::atomic<uint32_t> next{0}, done{0};
};

struct HostAtomics {
  Words &w;
  std::minstd_rand rng;
  void maybe_yield() {
    if ((rng() & 7u) == 0u) std::this_thread::yield();
  }
  uint32_t claim(uint32_t C) {
    maybe_yield();
    const uint32_t r = w.next.fetch_add(C, std::memory_order_relaxed);
    maybe_yield();
    return r;
  }
  uint32_t arrive() {
    maybe_yield();
    return w.done.fetch_add(1u, std::memory_order_acq_rel);
  }
  uint32_t take_next() {
    maybe_yield();
    return w.next.exchange(0u, std::memory_order_relaxed);
  }
  void clear_done() { w.done.store(0u, std::memory_order_relaxed); }
};

constexpr uint32_t kWaves = 64;
unsigned long checks = 0, failures = 0;

void expect(bool ok, const char *what, uint32_t ngroups, uint32_t C, int launch) {
  ++checks;
  if (ok) return;
  ++failures;
  std::fprintf(stderr, "FAIL %s: ngroups=%u C=%u launch=%d\n", what, ngroups, C, launch);
}

void run_case(Words &w, uint32_t ngroups, uint32_t C, uint32_t seed) {
  for (int launch = 0; launch < 3; ++launch) {
    std::vector<std::atomic<uint32_t>> visits(ngroups);
    for (auto &v : visits) v.store(0u, std::memory_order_relaxed);
    std::atomic<uint32_t> broken{0};
    std::vector<std::thread> waves;
    for (uint32_t t = 0; t < kWaves; ++t)
      waves.emplace_back([&, t] {
        HostAtomics a{w, std::minstd_rand(seed * 977u + t * 31u + (uint32_t)launch + 1u)};
        std::minstd_rand body_rng(seed + t);
        const bool ok = benor::sched::wave_run(a, ngroups, kWaves, C, [&](uint32_t g) {
          visits[g].fetch_add(1u, std::memory_order_relaxed);
          if ((body_rng() & 63u) == 0u) std::this_thread::yield();
        });
        if (!ok) broken.fetch_add(1u, std::memory_order_relaxed);
      });
    for (auto &t : waves) t.join();
    uint32_t bad = 0;
    for (auto &v : visits) bad += v.load(std::memory_order_relaxed) != 1u;
    expect(bad == 0u, "every group exactly once", ngroups, C, launch);
    expect(broken.load() == 0u, "invariant on next", ngroups, C, launch);
    expect(w.next.load() == 0u && w.done.load() == 0u, "both words 0 afterwards", ngroups, C, launch);
  }
}

}  // namespace

int main() {
  Words w;
  uint32_t seed = 1;
  for (uint32_t C : {1u, 3u, 8u, 16u})
    for (uint32_t ngroups : {0u, 1u, C - 1u, C, C + 1u, kWaves * C - 1u, kWaves * C + 1u, 100000u})
      run_case(w, ngroups, C, seed++);

  using benor::sched::rule;
  const uint64_t resident = 256u * 3u * 4u;   // the headline kernel: 3 workgroups of 4 waves on each of 256 CUs
  const benor::sched::Rule headline = rule(11, 22, 3125000, resident);
  expect(headline.dynamic && headline.chunk == 8u, "headline: dynamic, C = 8", 3125000, headline.chunk, 0);
  expect(!rule(3, 6, 312500, 256u * 8u * 4u).dynamic, "W = 3: static", 312500, 0, 0);
  expect(!rule(11, 22, 626, resident).dynamic, "626 groups: static", 626, 0, 0);
  expect(benor::sched::expected_next(1, 1, 8) == 16u, "expected_next", 1, 8, 0);

  std::printf("%lu checks, %lu failures\n", checks, failures);
  return failures ? 1 : 0;
}
