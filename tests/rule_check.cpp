// Host check of csrc/benor_rule.h (tests/test_rule.py builds it with
// -fsanitize=address,undefined and runs it): the presets and the validation, the
// threshold rule at Protocol B's words against Protocol B written out here by hand at
// every (N, F, c0, c1) with N <= 40, at (0, 0, 2F) against the reference's rule for
// N <= 3F + 1 with the count at which they part above it, Protocol A's steps against
// the paper's text, and lumped::RuleT (csrc/benor_lumped.h) as the same two steps.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "benor.h"
#include "benor_lumped.h"
#include "benor_rule.h"

namespace {

unsigned long checks = 0, failures = 0;

void expect(bool ok, const char *what, uint32_t a = 0u, uint32_t b = 0u, uint32_t c = 0u, uint32_t d = 0u) {
  ++checks;
  if (ok) return;
  ++failures;
  std::fprintf(stderr, "FAIL %s (%u, %u, %u, %u)\n", what, a, b, c, d);
}

using benor::rule::kNone;
using benor::rule::p_step;
using benor::rule::r_step;

// ---- the two compile-time rules, by hand from include/benor.h's mode texts
// BYZ_RULE_B: propose 0 if 2 c0 > N + F, else 1 if 2 c1 > N + F, else "?".
uint32_t b_r(uint32_t c0, uint32_t c1, uint32_t N, uint32_t F) {
  if (2u * c0 > N + F) return 0u;
  if (2u * c1 > N + F) return 1u;
  return kNone;
}
// ... v = the value with the strictly larger count; with c_v > F: x = v, decided iff 2 c_v > N + F; else the coin.
uint32_t b_p(uint32_t c0, uint32_t c1, uint32_t N, uint32_t F, bool &decided) {
  decided = false;
  if (c0 == c1) return kNone;
  const uint32_t v = c1 > c0 ? 1u : 0u, cv = v ? c1 : c0;
  if (cv <= F) return kNone;
  decided = 2u * cv > N + F;
  return v;
}
// The reference (node.ts:46-158): propose the bare majority; c0 > F decides 0, else c1 > F decides 1, else the
// strict majority, else the coin.
uint32_t ref_r(uint32_t c0, uint32_t c1) { return c0 > c1 ? 0u : (c1 > c0 ? 1u : kNone); }
uint32_t ref_p(uint32_t c0, uint32_t c1, uint32_t F, bool &decided) {
  decided = true;
  if (c0 > F) return 0u;
  if (c1 > F) return 1u;
  decided = false;
  return c1 > c0 ? 1u : (c0 > c1 ? 0u : kNone);
}

void check_presets() {
  const bo_rule a = benor::rule::protocol_a(64u, 20u), b = benor::rule::protocol_b(64u, 12u);
  expect(a.propose_gt2 == 64u && a.adopt_gt == 0u && a.decide_gt2 == 40u && a.reserved == 0u, "protocol_a(64, 20)");
  expect(b.propose_gt2 == 76u && b.adopt_gt == 12u && b.decide_gt2 == 76u && b.reserved == 0u, "protocol_b(64, 12)");
  const bo_rule top = benor::rule::protocol_b(1u << 24, (1u << 24) - 1u);
  expect(top.propose_gt2 == (1u << 25) - 1u && benor::rule::check(top, nullptr) == BO_OK, "protocol_b at the top of lumped's range");
  expect(benor::rule::preset_fits(1u << 24, (1u << 24) - 1u), "preset_fits 2^24");
  expect(benor::rule::preset_fits(0x7FFFFFFFu, 0u) && !benor::rule::preset_fits(0x7FFFFFFFu, 1u), "preset_fits N + F");
  expect(!benor::rule::preset_fits(0u, 0x40000000u) && benor::rule::preset_fits(0x40000000u, 0x3FFFFFFFu), "preset_fits 2 F");
}

void check_validation() {
  const char *msg = nullptr;
  bo_rule t{10u, 0u, 8u, 0u};
  expect(benor::rule::check(t, &msg) == BO_OK && msg && !*msg, "a valid rule");
  expect(benor::rule::check(bo_rule{0x7FFFFFFFu, 0x7FFFFFFFu, 0x7FFFFFFFu, 0u}, nullptr) == BO_OK, "the largest words");
  expect(benor::rule::check(bo_rule{0u, 0u, 0u, 0u}, nullptr) == BO_OK, "all zero");
  struct Bad {
    bo_rule t;
    const char *word;
  };
  const Bad bad[] = {{{0x80000000u, 0u, 0u, 0u}, "propose_gt2"}, {{0u, 0x80000000u, 0u, 0u}, "adopt_gt"},
                     {{0u, 0u, 0x80000000u, 0u}, "decide_gt2"}, {{0xFFFFFFFFu, 0u, 0u, 0u}, "propose_gt2"},
                     {{0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u}, "adopt_gt"}, {{10u, 0u, 8u, 1u}, "reserved"},
                     {{10u, 0u, 8u, 0x80000000u}, "reserved"}};
  for (const Bad &b : bad) {
    msg = nullptr;
    expect(benor::rule::check(b.t, &msg) == BO_ERR_INVALID_ARGUMENT, b.word);
    expect(msg && std::strstr(msg, b.word) != nullptr && std::strstr(msg, "bo_rule") != nullptr, "the text names the word");
    expect(benor::rule::check(b.t, nullptr) == BO_ERR_INVALID_ARGUMENT, "without a text");
  }
}

// Protocol B's words against Protocol B at every count an inbox of at most N messages can give.
void check_protocol_b() {
  for (uint32_t N = 1u; N <= 40u; ++N)
    for (uint32_t F = 0u; F < N; ++F) {
      const bo_rule t = benor::rule::protocol_b(N, F);
      for (uint32_t c0 = 0u; c0 <= N; ++c0)
        for (uint32_t c1 = 0u; c0 + c1 <= N; ++c1) {
          bool d = false, want_d = false;
          expect(r_step(t, c0, c1) == b_r(c0, c1, N, F), "Protocol B, R-step", N, F, c0, c1);
          const uint32_t got = p_step(t, c0, c1, d), want = b_p(c0, c1, N, F, want_d);
          expect(got == want && d == want_d, "Protocol B, P-step", N, F, c0, c1);
          // csrc/benor_lumped.h's compile-time rule is the same function
          bool dl = false;
          expect(benor::lumped::RuleB::r(c0, c1, N, F) == r_step(t, c0, c1), "lumped::RuleB::r", N, F, c0, c1);
          expect(benor::lumped::RuleB::p(c0, c1, N, F, dl) == got && dl == d, "lumped::RuleB::p", N, F, c0, c1);
        }
    }
}

// (0, 0, 2F) against the reference's rule where a quorum cannot hold more than F of both values.
void check_reference() {
  for (uint32_t N = 1u; N <= 40u; ++N)
    for (uint32_t F = 0u; F < N; ++F) {
      if (N > 3u * F + 1u) continue;
      const bo_rule t{0u, 0u, 2u * F, 0u};
      const uint32_t q = N - F;
      for (uint32_t c0 = 0u; c0 <= q; ++c0)
        for (uint32_t c1 = 0u; c0 + c1 <= q; ++c1) {
          bool d = false, want_d = false;
          expect(r_step(t, c0, c1) == ref_r(c0, c1), "reference, R-step", N, F, c0, c1);
          const uint32_t got = p_step(t, c0, c1, d), want = ref_p(c0, c1, F, want_d);
          expect(got == want && d == want_d, "reference, P-step", N, F, c0, c1);
        }
    }
  // N = 3F + 2 = 5: a quorum of 4 can hold F + 1 = 2 of both values; the reference decides 0, the rule takes the coin
  bool d = true, dr = false;
  const bo_rule t{0u, 0u, 2u, 0u};
  expect(ref_p(2u, 2u, 1u, dr) == 0u && dr, "the reference at (5, 1), (2, 2)");
  expect(p_step(t, 2u, 2u, d) == kNone && !d, "(0, 0, 2F) at (5, 1), (2, 2)");
  // ... and at N = 3F + 3 = 6 with (2, 3): the reference decides 0, the rule decides the larger count, 1
  expect(ref_p(2u, 3u, 1u, dr) == 0u && dr, "the reference at (6, 1), (2, 3)");
  expect(p_step(t, 2u, 3u, d) == 1u && d, "(0, 0, 2F) at (6, 1), (2, 3)");
}

// Protocol A by the paper's text: propose v iff more than N / 2 of the messages carry v; decide v on more than F
// proposals of v, adopt v on any proposal of v (at most one value is proposed), else the coin.
void check_protocol_a() {
  for (uint32_t N = 1u; N <= 40u; ++N)
    for (uint32_t F = 0u; 2u * F < N; ++F) {
      const bo_rule t = benor::rule::protocol_a(N, F);
      const benor::lumped::RuleT lt{t};
      for (uint32_t c0 = 0u; c0 <= N; ++c0)
        for (uint32_t c1 = 0u; c0 + c1 <= N; ++c1) {
          const uint32_t want_r = 2u * c0 > N ? 0u : (2u * c1 > N ? 1u : kNone);
          expect(r_step(t, c0, c1) == want_r, "Protocol A, R-step", N, F, c0, c1);
          bool d = false, dl = false;
          const uint32_t got = p_step(t, c0, c1, d);
          if (c0 == 0u || c1 == 0u) {                          // one value proposed, as Protocol A guarantees
            const uint32_t cv = c0 + c1, v = c1 ? 1u : 0u;
            expect(got == (cv ? v : kNone) && d == (cv > F), "Protocol A, P-step", N, F, c0, c1);
          } else {
            expect(got == (c0 == c1 ? kNone : (c1 > c0 ? 1u : 0u)), "Protocol A, P-step on two values", N, F, c0, c1);
          }
          expect(lt.r(c0, c1, N, F) == r_step(t, c0, c1), "lumped::RuleT::r", N, F, c0, c1);
          expect(lt.p(c0, c1, N, F, dl) == got && dl == d, "lumped::RuleT::p", N, F, c0, c1);
        }
    }
  // the largest counts: 2 c_v = 2^25 against words near it, no overflow
  bool d = false;
  const bo_rule top = benor::rule::protocol_a(1u << 24, (1u << 23) - 1u);
  expect(r_step(top, 0u, 1u << 24) == 1u && r_step(top, 1u << 23, 1u << 23) == kNone, "R-step at 2^24");
  expect(r_step(top, (1u << 23) + 1u, (1u << 23) - 1u) == 0u && r_step(top, 1u << 23, (1u << 23) - 1u) == kNone, "R-step at N / 2");
  expect(p_step(top, 1u << 23, 0u, d) == 0u && d, "P-step above F at 2^23");
  expect(p_step(top, (1u << 23) - 1u, 0u, d) == 0u && !d, "P-step at F");
  const bo_rule big{0x7FFFFFFFu, 0x7FFFFFFFu, 0x7FFFFFFFu, 0u};
  expect(r_step(big, 1u << 24, 0u) == kNone && p_step(big, 1u << 24, 0u, d) == kNone && !d, "the largest words never fire");
}

// One round of the lumped chain under lumped::RuleT at Protocol B's words is the round under lumped::RuleB.
struct NoCoin {
  uint32_t common(uint32_t) const { return 2u | 1u; }          // a common round with bit 1
  uint32_t binom(uint32_t, uint32_t, uint32_t) const { return 0u; }
};

void check_lumped_round() {
  bo_lumped_cfg c;
  std::memset(&c, 0, sizeof c);
  c.N = 64u, c.F = 12u, c.b = 12u, c.byz_even = 6u, c.k_max = 16u;
  const char *msg = nullptr;
  for (uint32_t strategy : {(uint32_t)BO_BYZ_BALANCE, (uint32_t)BO_BYZ_SPLIT}) {
    c.strategy = strategy;
    c.rule = 7u;                                               // not a rule of bo_lumped_cfg: the _rule entries do not read it
    expect(benor::lumped::check(c, &msg) == BO_ERR_INVALID_ARGUMENT && std::strstr(msg, "rule must be"), "cfg.rule is checked");
    expect(benor::lumped::check(c, &msg, false) == BO_OK, "cfg.rule is not read with a threshold rule");
    const benor::lumped::Shape s = benor::lumped::shape_of(c);
    const benor::lumped::RuleT t{benor::rule::protocol_b(c.N, c.F)};
    for (uint32_t H1 = 0u; H1 <= s.hh; ++H1) {
      benor::lumped::State a{s.hh - H1, H1, {0u, 0u}, 0u}, b = a;
      NoCoin src;
      const bool da = benor::lumped::round(t, s, 1u, a, src);
      const bool db = benor::lumped::round<benor::lumped::RuleB>(s, 1u, b, src);
      expect(da == db && a.a[0] == b.a[0] && a.a[1] == b.a[1] && a.dec == b.dec && a.H0 == b.H0 && a.H1 == b.H1,
             "a round at Protocol B's words", strategy, H1);
    }
  }
}

}  // namespace

int main() {
  check_presets();
  check_validation();
  check_protocol_b();
  check_reference();
  check_protocol_a();
  check_lumped_round();
  std::printf("%lu checks, %lu failures\n", checks, failures);
  return failures ? 1 : 0;
}
