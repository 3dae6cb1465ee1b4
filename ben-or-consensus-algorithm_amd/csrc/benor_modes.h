// benor_modes.h -- the one place that knows the delivery modes (BO_MODE_*, include/benor.h)
// and the kernels' variant numbers (KParams::variant 0..21): which family a mode belongs to,
// what it is called in an error text, which plan a shared-coin mode becomes without its coin,
// which count-level variant runs which rule and coin, and what a launch of a matrix-core plan
// is (batch or state launch, small or big W, sure or deferring).  The runtime's validation and
// planning (benor_runtime.cpp), the geometry and dispatch (benor_kernels.hip) and the launch
// checks of benor_tally_byz.hip and benor_tally_sched.hip ask this header and nothing else.
// Plain C++17 over benor.h, no HIP: tests/modes_check.cpp checks it on the host against a list
// written out by hand.  Adding a mode: DESIGN.md §4.3.8.
#pragma once

#include <stdint.h>

#include "benor.h"

namespace benor {

// What the host asks about a mode.
enum ModeFlag : uint32_t {
  kModeRandom = 1u << 0,      // random delivery: at most F nodes crashed from the start (the others: exactly F)
  kModeCountLevel = 1u << 1,  // a count-level kernel (benor_tally*.hip) runs it
  kModeCrash = 1u << 2,       // crashes during the run: crash_at or crash_count / crash_window, f + scheduled <= F
  kModeByz = 1u << 3,         // faulty[i] == 2 is Byzantine; the crash_count word is byz_strategy, crash_cut byz_one
  kModeRuleB = 1u << 4,       // Ben-Or's Byzantine-tolerant rule (Protocol B)
  kModeCoin = 1u << 5,        // the crash_window word is coin_common
  kModeSched = 1u << 6,       // an adversarial scheduler: strategies BALANCE and SPLIT only, the plan keeps its mode
};

struct ModeTraits {
  uint32_t mode;              // the row's own BO_MODE_* (kModes is indexed by it)
  const char *name;           // as the error texts spell it
  uint32_t flags;
  uint32_t coin_parent;       // kModeCoin: the mode of a plan with coin_common == 0 (a kModeSched mode: itself)
  uint32_t variant;           // kModeCountLevel: the variant of the mode's own plan (kModeSched: with local coins)
  constexpr bool is(uint32_t flag) const { return (flags & flag) != 0u; }
};

// KParams::variant: BO_KERNEL_*'s numbers (bo_plan_kernel reports the variant), and one internal value.
enum : uint32_t {
  kVarBlocked = BO_KERNEL_BLOCKED,        // blocked popcount lockstep (W > 32)
  kVarW = BO_KERNEL_W,                    // W-specialised popcount lockstep (W <= 32)
  kVarRandom = BO_KERNEL_RANDOM,          // random delivery
  kVarEventLane = BO_KERNEL_EVENT,        // event level, one lane per trial (N <= 256)
  kVarEventWave = 5,                      // event level, one wave or workgroup per trial (N > 256, live runs): no
                                          // BO_KERNEL_* of its own, the runtime reports BO_KERNEL_EVENT
  kVarLane = BO_KERNEL_LANE,              // lane lockstep (m <= 64)
  kVarMfma = BO_KERNEL_MFMA,              // matrix-core lockstep, round 1; its base popcount kernel (kVarW or
                                          // kVarBlocked) serves its state launches and the trials it defers
  kVarMfmaSmall = BO_KERNEL_MFMA_SMALL,   // packed matrix-core lockstep (2 <= m <= 32); the lane kernel serves
                                          // its state launches and its short launches
  // the count-level kernels
  kVarTally = BO_KERNEL_TALLY,
  kVarTally3 = BO_KERNEL_TALLY3,
  kVarCrash = BO_KERNEL_TALLY_CRASH,
  kVarPartial = BO_KERNEL_TALLY_PARTIAL,
  kVarSubset = BO_KERNEL_TALLY_SUBSET,
  kVarByz = BO_KERNEL_TALLY_BYZ,          // + 1: Protocol B's rule, + 2: a shared coin
  kVarSched = BO_KERNEL_TALLY_SCHED,      // the same
  kVarCountLevelEnd = BO_KERNEL_TALLY_SCHED_B_COIN + 1,
};

#define BENOR_MODE(m, flags, parent, variant) {m, #m, flags, parent, variant}
constexpr uint32_t kTallyFlags = kModeRandom | kModeCountLevel;
constexpr uint32_t kByzFlags = kTallyFlags | kModeByz;
constexpr ModeTraits kModes[] = {
    BENOR_MODE(BO_MODE_LOCKSTEP, 0u, 0u, 0u),
    BENOR_MODE(BO_MODE_RANDOM_DELIVERY, kModeRandom, 0u, 0u),
    BENOR_MODE(BO_MODE_EVENT, 0u, 0u, 0u),
    BENOR_MODE(BO_MODE_RANDOM_TALLY, kTallyFlags, 0u, kVarTally),
    BENOR_MODE(BO_MODE_RANDOM_TALLY3, kTallyFlags, 0u, kVarTally3),
    BENOR_MODE(BO_MODE_CRASH_TALLY, kTallyFlags | kModeCrash, 0u, kVarCrash),
    BENOR_MODE(BO_MODE_CRASH_PARTIAL, kTallyFlags | kModeCrash, 0u, kVarPartial),
    BENOR_MODE(BO_MODE_CRASH_SUBSET, kTallyFlags | kModeCrash, 0u, kVarSubset),
    BENOR_MODE(BO_MODE_BYZ_TALLY, kByzFlags, 0u, kVarByz),
    BENOR_MODE(BO_MODE_BYZ_RULE_B, kByzFlags | kModeRuleB, 0u, kVarByz + 1u),
    BENOR_MODE(BO_MODE_BYZ_COIN, kByzFlags | kModeCoin, BO_MODE_BYZ_TALLY, kVarByz + 2u),
    BENOR_MODE(BO_MODE_BYZ_RULE_B_COIN, kByzFlags | kModeRuleB | kModeCoin, BO_MODE_BYZ_RULE_B, kVarByz + 3u),
    BENOR_MODE(BO_MODE_SCHED_TALLY, kByzFlags | kModeCoin | kModeSched, BO_MODE_SCHED_TALLY, kVarSched),
    BENOR_MODE(BO_MODE_SCHED_RULE_B, kByzFlags | kModeRuleB | kModeCoin | kModeSched, BO_MODE_SCHED_RULE_B, kVarSched + 1u),
};
#undef BENOR_MODE
constexpr uint32_t kModeCount = sizeof(kModes) / sizeof(kModes[0]);
static_assert(kModeCount == BO_MODE_SCHED_RULE_B + 1, "one row per BO_MODE_*");

constexpr bool modes_in_order() {
  for (uint32_t i = 0; i < kModeCount; ++i)
    if (kModes[i].mode != i) return false;
  return true;
}
static_assert(modes_in_order(), "kModes is indexed by the mode's value");

// The row of a mode, nullptr for a value that is no mode.
constexpr const ModeTraits *mode_traits(uint32_t mode) { return mode < kModeCount ? &kModes[mode] : nullptr; }

// ---- The matrix-core kernel's KIND (KParams::G of a kVarMfma plan; benor_mfma.h), as plan_geometry picks it
enum : uint32_t {
  kKindSure = 0,      // every vote count odd and m > 2F: every trial halts in round 1, nothing is deferred
  kKindMajority = 1,  // m > 2F: a trial that ties in round 1 is deferred
  kKindMinority = 2,  // F < m <= 2F: ... and so is one in which a receiver does not decide
};
constexpr uint32_t kMfmaRegMaxW = 16;   // W <= 16: operands in registers (benor_mfma.h); beyond, the big-network form

// What a launch of a kVarMfma plan is.  A state launch (per-node state: the network API) runs the plan's base
// popcount kernel, a batch launch the matrix cores.  Scalar forms over (variant, KIND, W, state launch), so that
// the host check reaches them; benor_internal.h has the KParams forms.
constexpr bool mfma_batch(uint32_t v, uint32_t, uint32_t, bool state) { return v == kVarMfma && !state; }
constexpr bool mfma_small_w_batch(uint32_t v, uint32_t kind, uint32_t W, bool state) {
  return mfma_batch(v, kind, W, state) && W <= kMfmaRegMaxW;
}
constexpr bool mfma_big_batch(uint32_t v, uint32_t kind, uint32_t W, bool state) {   // benor_mfma_big.hip, _coop.hip
  return mfma_batch(v, kind, W, state) && W > kMfmaRegMaxW;
}
constexpr bool mfma_sure_batch(uint32_t v, uint32_t kind, uint32_t W, bool state) {  // the paired kernel and its forms
  return mfma_small_w_batch(v, kind, W, state) && kind == kKindSure;
}
constexpr bool mfma_defers(uint32_t v, uint32_t kind, uint32_t W, bool state) {      // at every W: the deferral passes
  return mfma_batch(v, kind, W, state) && kind > kKindSure;
}

// ---- KParams::variant, the count-level kernels
constexpr bool variant_count_level(uint32_t v) { return v >= kVarTally && v < kVarCountLevelEnd; }
constexpr bool variant_crash(uint32_t v) { return v >= kVarCrash && v <= kVarSubset; }    // tables per live count
constexpr bool variant_byz(uint32_t v) { return v >= kVarByz && v < kVarSched; }          // benor_tally_byz.hip
constexpr bool variant_sched(uint32_t v) { return v >= kVarSched && v < kVarCountLevelEnd; }   // benor_tally_sched.hip
// ... of the two files whose variants differ in rule and coin alone
constexpr bool variant_rule_b(uint32_t v) { return (variant_byz(v) || variant_sched(v)) && ((v - kVarByz) & 1u) != 0u; }
constexpr bool variant_shared_coin(uint32_t v) { return (variant_byz(v) || variant_sched(v)) && ((v - kVarByz) & 2u) != 0u; }

// A Byzantine mode's variant (a shared-coin mode's plan has coin_common != 0: at 0 it is its parent's plan), and a
// scheduler mode's, which keeps its mode and takes the shared-coin entry when coin_common != 0.
constexpr uint32_t byz_variant(uint32_t mode) { return kModes[mode].variant; }
constexpr uint32_t sched_variant(uint32_t mode, bool shared_coin) { return kModes[mode].variant + (shared_coin ? 2u : 0u); }
// The variant of a count-level plan: kp.mode after the planner's demotions, and whether it carries a coin word.
constexpr uint32_t count_level_variant(uint32_t mode, bool shared_coin) {
  return kModes[mode].is(kModeSched) ? sched_variant(mode, shared_coin) : kModes[mode].variant;
}

}  // namespace benor
