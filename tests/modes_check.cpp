// Host check of csrc/benor_modes.h (tests/test_modes.py builds it with
// -fsanitize=address,undefined and runs it): the modes table against a list
// written out here by hand, the variant predicates against the BO_KERNEL_*
// comments of include/benor.h, the names of the variants 0..8, the matrix-core
// launch predicates over their whole grid, and the Byzantine and scheduler
// variant functions.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "benor.h"
#include "benor_modes.h"

namespace {

unsigned long checks = 0, failures = 0;

void expect(bool ok, const char *what, uint32_t a, uint32_t b = 0u) {
  ++checks;
  if (ok) return;
  ++failures;
  std::fprintf(stderr, "FAIL %s (%u, %u)\n", what, a, b);
}

// include/benor.h, mode by mode: at most F crashed (else exactly F); a count-level kernel; crashes
// during the run; Byzantine senders; Protocol B's rule; a coin_common word; an adversarial scheduler;
// and the mode whose plan a coin_common == 0 configuration is (-1: no coin word).
struct Want {
  uint32_t mode;
  const char *name;
  bool random, count_level, crash, byz, rule_b, coin, sched;
  int coin_parent;
};
const Want kWant[] = {
    {0, "BO_MODE_LOCKSTEP", false, false, false, false, false, false, false, -1},
    {1, "BO_MODE_RANDOM_DELIVERY", true, false, false, false, false, false, false, -1},
    {2, "BO_MODE_EVENT", false, false, false, false, false, false, false, -1},
    {3, "BO_MODE_RANDOM_TALLY", true, true, false, false, false, false, false, -1},
    {4, "BO_MODE_RANDOM_TALLY3", true, true, false, false, false, false, false, -1},
    {5, "BO_MODE_CRASH_TALLY", true, true, true, false, false, false, false, -1},
    {6, "BO_MODE_CRASH_PARTIAL", true, true, true, false, false, false, false, -1},
    {7, "BO_MODE_CRASH_SUBSET", true, true, true, false, false, false, false, -1},
    {8, "BO_MODE_BYZ_TALLY", true, true, false, true, false, false, false, -1},
    {9, "BO_MODE_BYZ_RULE_B", true, true, false, true, true, false, false, -1},
    {10, "BO_MODE_BYZ_COIN", true, true, false, true, false, true, false, 8},
    {11, "BO_MODE_BYZ_RULE_B_COIN", true, true, false, true, true, true, false, 9},
    {12, "BO_MODE_SCHED_TALLY", true, true, false, true, false, true, true, 12},
    {13, "BO_MODE_SCHED_RULE_B", true, true, false, true, true, true, true, 13},
};

void check_modes() {
  using namespace benor;
  expect(sizeof(kWant) / sizeof(kWant[0]) == kModeCount, "row count", kModeCount);
  for (const Want &w : kWant) {
    const ModeTraits *t = mode_traits(w.mode);
    expect(t != nullptr, "a mode without a row", w.mode);
    if (!t) continue;
    expect(t->mode == w.mode, "row index", w.mode, t->mode);
    expect(std::strcmp(t->name, w.name) == 0, "name", w.mode);
    expect(t->is(kModeRandom) == w.random, "random delivery", w.mode);
    expect(t->is(kModeCountLevel) == w.count_level, "count level", w.mode);
    expect(t->is(kModeCrash) == w.crash, "crash family", w.mode);
    expect(t->is(kModeByz) == w.byz, "Byzantine family", w.mode);
    expect(t->is(kModeRuleB) == w.rule_b, "rule B", w.mode);
    expect(t->is(kModeCoin) == w.coin, "shared-coin word", w.mode);
    expect(t->is(kModeSched) == w.sched, "adversarial scheduler", w.mode);
    if (w.coin_parent >= 0) expect(t->coin_parent == (uint32_t)w.coin_parent, "coin parent", w.mode, t->coin_parent);
  }
  for (uint32_t bad : {14u, 15u, 255u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu})
    expect(mode_traits(bad) == nullptr, "a row for a value that is no mode", bad);
}

// BO_KERNEL_* (include/benor.h): 9 TALLY, 10 TALLY3, 11..13 the crash family, 14..17 TALLY_BYZ (15 and 17
// Protocol B's rule, 16 and 17 the shared coin), 18..21 TALLY_SCHED (19 and 21 the rule, 20 and 21 the coin).
void check_variants() {
  using namespace benor;
  for (uint32_t v = 0; v < 40u; ++v) {
    const bool crash = v >= 11u && v <= 13u, byz = v >= 14u && v <= 17u, sched = v >= 18u && v <= 21u;
    expect(variant_count_level(v) == (v >= 9u && v <= 21u), "count level", v);
    expect(variant_crash(v) == crash, "crash family", v);
    expect(variant_byz(v) == byz, "Byzantine kernels", v);
    expect(variant_sched(v) == sched, "scheduler kernel", v);
    expect(variant_rule_b(v) == (v == 15u || v == 17u || v == 19u || v == 21u), "rule B", v);
    expect(variant_shared_coin(v) == (v == 16u || v == 17u || v == 20u || v == 21u), "shared coin", v);
    // a partition: the two plain kernels, then exactly one family
    const int plain = v == 9u || v == 10u;
    expect(plain + (int)variant_crash(v) + (int)variant_byz(v) + (int)variant_sched(v) == (int)variant_count_level(v),
           "partition", v);
  }
  expect(kVarTally == 9u && kVarTally3 == 10u && kVarCrash == 11u && kVarPartial == 12u && kVarSubset == 13u &&
             kVarByz == 14u && kVarSched == 18u && kVarCountLevelEnd == 22u, "variant names", 0u);
}

// The lockstep, random-delivery and event-level variants: BO_KERNEL_*'s numbers (include/benor.h) and 5, the
// wave-per-trial event kernel, which has no BO_KERNEL_* of its own; none of them is a count-level variant.
void check_variant_names() {
  using namespace benor;
  expect(kVarBlocked == 0u && BO_KERNEL_BLOCKED == 0, "kVarBlocked", kVarBlocked);
  expect(kVarW == 1u && BO_KERNEL_W == 1, "kVarW", kVarW);
  expect(kVarRandom == 2u && BO_KERNEL_RANDOM == 2, "kVarRandom", kVarRandom);
  expect(kVarEventLane == 4u && BO_KERNEL_EVENT == 4, "kVarEventLane", kVarEventLane);
  expect(kVarEventWave == 5u, "kVarEventWave", kVarEventWave);
  expect(kVarLane == 6u && BO_KERNEL_LANE == 6, "kVarLane", kVarLane);
  expect(kVarMfma == 7u && BO_KERNEL_MFMA == 7, "kVarMfma", kVarMfma);
  expect(kVarMfmaSmall == 8u && BO_KERNEL_MFMA_SMALL == 8, "kVarMfmaSmall", kVarMfmaSmall);
  for (uint32_t v = 0; v <= 8u; ++v) expect(!variant_count_level(v), "a lockstep variant counted as count-level", v);
  expect(kKindSure == 0u && kKindMajority == 1u && kKindMinority == 2u, "matrix-core KIND names", 0u);
}

// What a launch of a matrix-core plan is, against the conditions as the host code spelt them before the
// predicates existed: variant 7 with no node_out and no rounds_out, then W <= 16 or W > 16, G == 0 or G > 0.
void check_launch_predicates() {
  using namespace benor;
  for (uint32_t v = 0; v <= 21u; ++v)
    for (uint32_t kind = 0; kind <= 2u; ++kind)
      for (uint32_t W : {1u, 2u, 16u, 17u, 64u})
        for (bool state : {false, true}) {
          const uint32_t id = v << 16 | kind << 8 | W;
          expect(mfma_batch(v, kind, W, state) == (v == 7u && !state), "mfma_batch", id, state);
          expect(mfma_small_w_batch(v, kind, W, state) == (v == 7u && !state && W <= 16u), "mfma_small_w_batch", id, state);
          expect(mfma_big_batch(v, kind, W, state) == (v == 7u && W > 16u && !state), "mfma_big_batch", id, state);
          expect(mfma_sure_batch(v, kind, W, state) == !(v != 7u || kind != 0u || W > 16u || state), "mfma_sure_batch", id, state);
          expect(mfma_defers(v, kind, W, state) == (v == 7u && kind > 0u && !state), "mfma_defers", id, state);
        }
}

void check_variant_functions() {
  using namespace benor;
  expect(byz_variant(BO_MODE_BYZ_TALLY) == BO_KERNEL_TALLY_BYZ, "byz_variant", BO_MODE_BYZ_TALLY);
  expect(byz_variant(BO_MODE_BYZ_RULE_B) == BO_KERNEL_TALLY_BYZ_B, "byz_variant", BO_MODE_BYZ_RULE_B);
  expect(byz_variant(BO_MODE_BYZ_COIN) == BO_KERNEL_TALLY_BYZ_COIN, "byz_variant", BO_MODE_BYZ_COIN);
  expect(byz_variant(BO_MODE_BYZ_RULE_B_COIN) == BO_KERNEL_TALLY_BYZ_B_COIN, "byz_variant", BO_MODE_BYZ_RULE_B_COIN);
  expect(sched_variant(BO_MODE_SCHED_TALLY, false) == BO_KERNEL_TALLY_SCHED, "sched_variant", 12u, 0u);
  expect(sched_variant(BO_MODE_SCHED_RULE_B, false) == BO_KERNEL_TALLY_SCHED_B, "sched_variant", 13u, 0u);
  expect(sched_variant(BO_MODE_SCHED_TALLY, true) == BO_KERNEL_TALLY_SCHED_COIN, "sched_variant", 12u, 1u);
  expect(sched_variant(BO_MODE_SCHED_RULE_B, true) == BO_KERNEL_TALLY_SCHED_B_COIN, "sched_variant", 13u, 1u);
  // the plan's variant: the coin word moves a scheduler mode alone
  const uint32_t plain[][2] = {{BO_MODE_RANDOM_TALLY, 9u}, {BO_MODE_RANDOM_TALLY3, 10u}, {BO_MODE_CRASH_TALLY, 11u},
                               {BO_MODE_CRASH_PARTIAL, 12u}, {BO_MODE_CRASH_SUBSET, 13u}, {BO_MODE_BYZ_TALLY, 14u},
                               {BO_MODE_BYZ_RULE_B, 15u}, {BO_MODE_BYZ_COIN, 16u}, {BO_MODE_BYZ_RULE_B_COIN, 17u}};
  for (const auto &p : plain)
    for (bool coin : {false, true}) expect(count_level_variant(p[0], coin) == p[1], "count_level_variant", p[0], coin);
  for (bool coin : {false, true}) {
    expect(count_level_variant(BO_MODE_SCHED_TALLY, coin) == 18u + (coin ? 2u : 0u), "count_level_variant", 12u, coin);
    expect(count_level_variant(BO_MODE_SCHED_RULE_B, coin) == 19u + (coin ? 2u : 0u), "count_level_variant", 13u, coin);
  }
}

}  // namespace

int main() {
  check_modes();
  check_variants();
  check_variant_names();
  check_launch_predicates();
  check_variant_functions();
  std::printf("%lu checks, %lu failures\n", checks, failures);
  return failures ? 1 : 0;
}
