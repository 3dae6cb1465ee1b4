// benor_mfma_sched.h -- how the KIND 0 matrix-core kernel (benor_mfma.h)
// spreads its 32-trial groups over its waves: the planner's rule and the
// claim protocol of the dynamic form.  Plain C++ that also compiles on the
// host (tests/mfma_sched_check.cpp runs the protocol on std::atomic threads
// and checks the rule).
//
// Static form: wave w runs groups w, w + waves, w + 2 waves, ...
// Dynamic form: the plan owns two words, `next` and `done`, both 0 between
// launches.  A wave claims chunks of C consecutive groups,
//   base = fetch_add(next, C);  groups [base, min(base + C, ngroups)),
// until a claim returns base >= ngroups: every wave ends with exactly one
// failing claim.  It then adds 1 to `done`; the wave that reads waves - 1 is
// the last one, after every other wave's last claim: it takes `next`, which
// must be C (ceil(ngroups / C) + waves) -- every successful claim and one
// failing claim per wave -- and leaves both words 0 for the next launch on the
// stream.  No wave waits for another: no spin, no barrier, no flag poll; every
// loop is bounded by ngroups.  The outcome histogram is a sum over trials, so
// which wave runs which group changes no bin.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BENOR_SCHED_HD __host__ __device__ inline
#else
#define BENOR_SCHED_HD inline
#endif

namespace benor {
namespace sched {

constexpr uint32_t kMaxChunk = 16;         // the rule keeps the static form where it would need more
constexpr uint32_t kInvariantBit = 4u;     // KParams::overflow: `next` was off at the end of a launch
constexpr uint32_t kDoneWord = 32;         // `done` sits 128 bytes behind `next`: a line of its own
constexpr uint32_t kWords = 64;            // the plan's allocation, u32 words

struct Rule {
  bool dynamic;
  uint32_t chunk;   // C of the dynamic form (the rule's value also where it keeps the static form)
};

// Groups the chip runs per microsecond: 1024 SIMDs, one 32x32x64 product per
// 16 cycles at ~2250 MHz, MT (W + KP) products per group.
BENOR_SCHED_HD uint32_t groups_per_us(uint32_t W, uint32_t MT) {
  const uint32_t KP = (MT + 1u) / 2u;
  return 1024u * 2250u / (32u * MT * (W + KP));
}

// One atomic word serves ~88 claims per microsecond; C keeps the claim rate
// at a twentieth of the group rate, far below that, and bounds a wave's idle
// time at the end of the launch to C groups.  Static where that needs
// C > kMaxChunk (small W: the groups are too short for one word) and where a
// launch has fewer than 4 C groups per resident wave (nothing to balance).
BENOR_SCHED_HD Rule rule(uint32_t W, uint32_t MT, uint64_t ngroups, uint64_t resident_waves) {
  const uint32_t c = (groups_per_us(W, MT) + 19u) / 20u;
  Rule r;
  r.chunk = c < 1u ? 1u : c;
  r.dynamic = r.chunk <= kMaxChunk && ngroups >= 4ull * r.chunk * resident_waves;
  return r;
}

// `next` at the end of a launch.
BENOR_SCHED_HD uint32_t expected_next(uint32_t ngroups, uint32_t waves, uint32_t C) {
  return C * ((ngroups + C - 1u) / C + waves);
}

BENOR_SCHED_HD uint32_t chunk_end(uint32_t base, uint32_t ngroups, uint32_t C) {
  return ngroups - base < C ? ngroups : base + C;   // base < ngroups
}

// The protocol over an atomics policy A:
//   uint32_t claim(uint32_t C)   relaxed fetch_add on `next`
//   uint32_t arrive()            acq_rel fetch_add(done, 1)
//   uint32_t take_next()         exchange(next, 0)
//   void clear_done()            store(done, 0)
template <class A>
BENOR_SCHED_HD uint32_t claim(A &a, uint32_t C) {
  return a.claim(C);
}

// After a wave's failing claim.  Returns false when this wave was the last
// one and found `next` off.
template <class A>
BENOR_SCHED_HD bool finish(A &a, uint32_t ngroups, uint32_t waves, uint32_t C) {
  if (a.arrive() != waves - 1u) return true;
  const uint32_t n = a.take_next();
  a.clear_done();
  return n == expected_next(ngroups, waves, C);
}

// One wave's whole run, as the kernel does it: the next claim is issued
// before the current chunk's groups and consumed after them.
template <class A, class Body>
inline bool wave_run(A &a, uint32_t ngroups, uint32_t waves, uint32_t C, Body body) {
  uint32_t pending = claim(a, C);
  for (;;) {
    const uint32_t base = pending;
    if (base >= ngroups) break;
    pending = claim(a, C);
    for (uint32_t g = base, e = chunk_end(base, ngroups, C); g < e; ++g) body(g);
  }
  return finish(a, ngroups, waves, C);
}

}  // namespace sched
}  // namespace benor
