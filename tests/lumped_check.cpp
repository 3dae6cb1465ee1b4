// Host check of csrc/benor_lumped.h, the class-level chain of the adversarial scheduler
// (DESIGN §4.3.12): the scheduler's closed forms, both rules' steps, a round, the outcome
// bins, the Binomial(n, 1/2) draw over a word source, and the validation, each against
// values written out by hand.  Plain C++17, no HIP, no device: tests/test_lumped.py builds
// it with the address and undefined-behaviour sanitizers and runs it as it is.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "benor.h"
#include "benor_lumped.h"

using namespace benor::lumped;

static int checks = 0, failures = 0;

#define CHECK(cond)                                                 \
  do {                                                              \
    ++checks;                                                       \
    if (!(cond)) {                                                  \
      ++failures;                                                   \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
    }                                                               \
  } while (0)

static bool is(Counts c, uint32_t c0, uint32_t c1) { return c.c0 == c0 && c.c1 == c1; }

// A word source that hands out a fixed list in order and counts the calls.
struct ListWords {
  std::vector<uint64_t> w;
  uint32_t calls = 0;
  uint64_t operator()(uint32_t j) {
    if (j != calls) ++failures, std::printf("FAILED: word %u asked for out of order\n", j);
    ++calls;
    return w.at(j);
  }
};

// Tables for k = 7 and 8 written by hand: thr = {10, 20, 30} with lo 5, and {100} with lo 7.
struct HandTables {
  std::vector<uint64_t> thr{10, 20, 30, 100};
  std::vector<uint32_t> off, lo;
  TableDir dir;
  HandTables() : off(kTables + 1, 4u), lo(kTables, 0u) {
    off[0] = 0, off[1] = 3, lo[0] = 5, lo[1] = 7;
    dir.thr = thr.data(), dir.off = off.data(), dir.lo = lo.data();
  }
};

// A chain source that scripts the coin and the draws.
struct Script {
  uint32_t coin;                                   // what common() answers
  uint32_t commons = 0, binoms = 0;
  uint32_t common(uint32_t) { return ++commons, coin; }
  uint32_t binom(uint32_t n, uint32_t pi, uint32_t r) { return ++binoms, (n + pi + r) % (n + 1u); }
};

static bo_lumped_cfg good() {
  bo_lumped_cfg c;
  std::memset(&c, 0, sizeof c);
  c.N = 11, c.F = 2, c.f = 0, c.b = 2, c.byz_even = 1, c.rule = 0, c.strategy = BO_BYZ_BALANCE, c.k_max = 16;
  c.init_mode = BO_INIT_RANDOM;
  return c;
}

static bool rejects(const bo_lumped_cfg &c, int code, const char *word) {
  const char *msg = nullptr;
  const int rc = check(c, &msg);
  return rc == code && msg && std::strstr(msg, "bo_lumped") && std::strstr(msg, word);
}

int main() {
  // ---- push: the most v any inbox allows, then the least 1 - v.  q = 6, H = (4, 3, 2), b = 1
  CHECK(is(push(0, 6, 4, 3, 2, 1), 5, 0));         // c0 = min(6, 4 + 1) = 5, rest 1, a "?" fills it
  CHECK(is(push(1, 6, 4, 3, 2, 1), 0, 4));         // c1 = 4, rest 2 = the two "?"
  CHECK(is(push(1, 6, 4, 3, 0, 1), 2, 4));         // no "?": the rest are 0s
  CHECK(is(push(0, 3, 4, 3, 2, 1), 3, 0));         // capped by q
  // ---- even: "?" first, then level.  q = 7, H = (4, 3, 2), b = 1: r = 5, lo = 5 - 4 = 1, hi = 5
  CHECK(is(even(0, 7, 4, 3, 2, 1), 2, 3));         // (5 + 0) >> 1 = 2
  CHECK(is(even(1, 7, 4, 3, 2, 1), 3, 2));         // (5 + 1) >> 1 = 3
  CHECK(is(even(0, 6, 6, 0, 0, 1), 5, 1));         // lo = 6 - 1 = 5: one liar is all the 1s there are
  CHECK(is(even(1, 4, 0, 9, 0, 0), 0, 4));         // hi = 0
  CHECK(is(even(0, 4, 1, 1, 9, 0), 0, 0));         // Hq >= q: an inbox of "?" alone
  CHECK(is(counts(BO_BYZ_SPLIT, 1, 6, 4, 3, 2, 1), 0, 4));
  CHECK(is(counts(BO_BYZ_BALANCE, 1, 7, 4, 3, 2, 1), 3, 2));

  // ---- the rules
  bool d = true;
  CHECK(RuleRef::r(3, 2, 10, 4) == 0u && RuleRef::r(2, 3, 10, 4) == 1u && RuleRef::r(2, 2, 10, 4) == kNone);
  CHECK(RuleRef::r(0, 0, 10, 4) == kNone);
  CHECK(RuleRef::p(5, 1, 10, 4, d) == 0u && d);    // c0 > F
  CHECK(RuleRef::p(1, 5, 10, 4, d) == 1u && d);
  CHECK(RuleRef::p(5, 5, 10, 4, d) == 0u && d);    // both above F: 0 first
  CHECK(RuleRef::p(3, 2, 10, 4, d) == 0u && !d);   // the strict majority
  CHECK(RuleRef::p(2, 3, 10, 4, d) == 1u && !d);
  CHECK(RuleRef::p(2, 2, 10, 4, d) == kNone && !d);
  CHECK(RuleRef::p(0, 0, 10, 4, d) == kNone && !d);
  CHECK(RuleB::r(7, 0, 11, 2) == 0u && RuleB::r(6, 0, 11, 2) == kNone);   // 2 c > 13
  CHECK(RuleB::r(0, 7, 11, 2) == 1u && RuleB::r(4, 5, 11, 2) == kNone);
  CHECK(RuleB::p(7, 2, 11, 2, d) == 0u && d);
  CHECK(RuleB::p(2, 6, 11, 2, d) == 1u && !d);     // adopted (6 > F), not decided (12 <= 13)
  CHECK(RuleB::p(2, 1, 11, 2, d) == kNone && !d);  // c_v = 2 is not above F
  CHECK(RuleB::p(4, 4, 11, 2, d) == kNone && !d);
  CHECK(RuleB::r(1u << 24, 0, 1u << 24, (1u << 24) - 1u) == 0u);          // 2^25 > 2^25 - 1: no overflow

  // ---- the outcome bins
  bool viol = true;
  CHECK(outcome_bin(0, 9, true, 3, viol) == 9u && !viol);
  CHECK(outcome_bin(9, 9, true, 3, viol) == 10u && !viol);
  CHECK(outcome_bin(4, 9, true, 3, viol) == 11u && viol);
  CHECK(outcome_bin(4, 9, false, 16, viol) == 2u && !viol);
  CHECK(outcome_bin(9, 9, false, 16, viol) == 1u && !viol);
  CHECK(outcome_bin(0, 0, true, 1, viol) == 2u && !viol);                 // nobody honest

  // ---- shape_of: (11, 2), liars at compact 3 and 8 -> one even, one odd
  bo_lumped_cfg c = good();
  Shape s = shape_of(c);
  CHECK(s.q == 9u && s.nb == 2u && s.h[0] == 5u && s.h[1] == 4u && s.hh == 9u);
  c.N = 3, c.F = 2, c.b = 2, c.byz_even = 2;       // both liars on even indices: h_0 = 0
  s = shape_of(c);
  CHECK(s.h[0] == 0u && s.h[1] == 1u && s.hh == 1u && s.q == 1u);
  c.N = 10, c.F = 4, c.f = 3, c.b = 1, c.byz_even = 0;   // m = 7: 4 even, 3 odd
  s = shape_of(c);
  CHECK(s.h[0] == 4u && s.h[1] == 2u && s.hh == 6u);

  // ---- a round.  (10, 4, b = 0), BALANCE, reference rule: q = 6, h = (5, 5)
  c = good();
  c.N = 10, c.F = 4, c.b = 0, c.byz_even = 0;
  s = shape_of(c);
  {
    // unanimous 1: counts (0, 6) for both parities, proposals 1, P-phase (0, 6): 6 > 4 decides 1
    State st{0u, 10u, {0u, 0u}, 0u};
    Script src{1u};
    CHECK(round<RuleRef>(s, 1u, st, src));
    CHECK(st.a[0] == 5u && st.a[1] == 5u && st.dec == 3u && st.H1 == 10u && st.H0 == 0u);
    CHECK(src.commons == 0u && src.binoms == 0u);  // no coin taken: nothing drawn
  }
  {
    // level start (5, 5): every inbox (3, 3), everybody proposes "?", P-phase counts (0, 0): both take the coin
    State st{5u, 5u, {0u, 0u}, 0u};
    Script src{1u};                                // local coins: binom(5, pi, 2) = (5 + pi + 2) % 6
    CHECK(!round<RuleRef>(s, 2u, st, src));
    CHECK(src.commons == 1u && src.binoms == 2u);
    CHECK(st.a[0] == 1u && st.a[1] == 2u && st.dec == 0u && st.H1 == 3u && st.H0 == 7u);
    Script one{3u};                                // a common round with bit 1
    st = State{5u, 5u, {0u, 0u}, 0u};
    CHECK(!round<RuleRef>(s, 2u, st, one));
    CHECK(one.binoms == 0u && st.a[0] == 5u && st.a[1] == 5u && st.dec == 0u);
    Script zero{2u};
    st = State{5u, 5u, {0u, 0u}, 0u};
    CHECK(!round<RuleRef>(s, 2u, st, zero));
    CHECK(st.a[0] == 0u && st.a[1] == 0u && st.H0 == 10u);
  }
  {
    // H = (4, 6), BALANCE: r = 6, lo = 0, hi = 4 -> even (3, 3) "?", odd (3, 3) "?": all take the coin.
    // SPLIT: even push(0) = (4, 2) proposes 0, odd push(1) = (0, 6) proposes 1; P-phase sizes (5, 5, 0):
    // even (5, 1) decides 0, odd (1, 5) decides 1: both decided, and they differ.
    bo_lumped_cfg cs = c;
    cs.strategy = BO_BYZ_SPLIT;
    const Shape ss = shape_of(cs);
    State st{4u, 6u, {0u, 0u}, 0u};
    Script src{1u};
    CHECK(round<RuleRef>(ss, 1u, st, src));
    CHECK(st.a[0] == 0u && st.a[1] == 5u && st.dec == 3u && src.binoms == 0u);
    bool v;
    CHECK(outcome_bin(st.a[0] + st.a[1], ss.hh, true, 1u, v) == 5u && v);
  }
  {
    // a parity without a node neither takes a coin nor holds the halt back: (3, 2, b = 2), both liars even
    bo_lumped_cfg c3 = good();
    c3.N = 3, c3.F = 2, c3.b = 2, c3.byz_even = 2, c3.rule = 1;
    const Shape s3 = shape_of(c3);                 // q = 1, h = (0, 1), N + F = 5
    State st{1u, 0u, {0u, 0u}, 0u};
    Script src{1u};
    // even(): r = 1, odd parity: lo = 1 - min(1, 0 + 2) = 0, hi = 1, c0 = 1: (1, 0); 2 > 5 fails: "?";
    // P-phase sizes (0, 0, 1): (0, 0): the coin, for the odd parity alone
    CHECK(!round<RuleB>(s3, 1u, st, src));
    CHECK(src.commons == 1u && src.binoms == 1u && st.a[0] == 0u && st.dec == 0u);
  }

  // ---- the Binomial draw
  HandTables tb;
  {
    ListWords w{{0xFFFFFFFFFFFFFFFFull}};
    CHECK(binom_half(0u, w, tb.dir) == 0u && w.calls == 0u);             // no set bit, no word
    for (uint32_t k = 0; k <= 6; ++k) {
      ListWords one{{0xFFFFFFFFFFFFFFFFull}}, none{{0ull}}, mix{{0xF0F0F0F0F0F0F0F5ull}};
      CHECK(binom_half(1u << k, one, tb.dir) == (1u << k) && one.calls == 1u);
      CHECK(binom_half(1u << k, none, tb.dir) == 0u);
      const uint64_t low = k == 6 ? ~0ull : (1ull << (1u << k)) - 1ull;
      CHECK(binom_half(1u << k, mix, tb.dir) == (uint32_t)__builtin_popcountll(0xF0F0F0F0F0F0F0F5ull & low));
    }
    // n = 0b1001011 = 75: bits 0, 1, 3, 6 take words 0, 1, 2, 3 in that order
    ListWords four{{1ull, 2ull, 0x1FFull, 0x8000000000000001ull}};
    CHECK(binom_half(75u, four, tb.dir) == 1u + 1u + 8u + 2u && four.calls == 4u);
    // n = 128 + 256 + 1: word 0 -> bit 0, word 1 -> k = 7 (lo 5, thresholds 10 20 30), word 2 -> k = 8 (lo 7, 100)
    ListWords t1{{1ull, 20ull, 99ull}};
    CHECK(binom_half(385u, t1, tb.dir) == 1u + (5u + 2u) + (7u + 0u) && t1.calls == 3u);
    ListWords t2{{0ull, 9ull, 100ull}};
    CHECK(binom_half(385u, t2, tb.dir) == 0u + 5u + 8u);
    ListWords t3{{~0ull, ~0ull}};
    CHECK(binom_half(384u, t3, tb.dir) == 8u + 8u && t3.calls == 2u);
  }
  {
    const uint64_t T[5] = {3, 3, 7, 9, 9};
    CHECK(count_le(T, 5, 2) == 0u && count_le(T, 5, 3) == 2u && count_le(T, 5, 8) == 3u && count_le(T, 5, 9) == 5u);
    CHECK(count_le(T, 0, 9) == 0u && count_le(T, 1, 3) == 1u && count_le(T, 3, ~0ull) == 3u);
  }

  // ---- validation: every error, each with a name in its text
  CHECK(check(good(), nullptr) == BO_OK);
  c = good(), c.N = 0;
  CHECK(rejects(c, BO_ERR_INVALID_ARGUMENT, "N must be"));
  c = good(), c.N = kMaxN + 1u;
  CHECK(rejects(c, BO_ERR_INVALID_ARGUMENT, "N must be"));
  c = good(), c.N = kMaxN, c.F = 3355443u, c.b = 0, c.byz_even = 0;
  CHECK(check(c, nullptr) == BO_OK);
  c = good(), c.F = 11;
  CHECK(rejects(c, BO_ERR_INVALID_ARGUMENT, "F must be below N"));
  c = good(), c.f = 1;
  CHECK(rejects(c, BO_ERR_FAULTY_COUNT, "at most F nodes crashed or Byzantine"));
  c = good(), c.f = 0xFFFFFFFFu, c.b = 2;
  CHECK(rejects(c, BO_ERR_FAULTY_COUNT, "at most F"));                    // no 32-bit wrap
  c = good(), c.byz_even = 3;
  CHECK(rejects(c, BO_ERR_INVALID_ARGUMENT, "byz_even must be"));
  c = good(), c.N = 3, c.F = 2, c.b = 2, c.byz_even = 0;                  // two liars on one odd index
  CHECK(rejects(c, BO_ERR_INVALID_ARGUMENT, "b - byz_even must be"));
  c = good(), c.N = 2, c.F = 1, c.f = 1, c.b = 0, c.byz_even = 0;
  CHECK(check(c, nullptr) == BO_OK);
  for (uint32_t bad : {0u, 1u, 2u, 5u, 0xFFFFFFFFu}) {
    c = good(), c.strategy = bad;
    CHECK(rejects(c, BO_ERR_INVALID_ARGUMENT, "strategy must be"));
  }
  c = good(), c.rule = 2;
  CHECK(rejects(c, BO_ERR_INVALID_ARGUMENT, "rule must be"));
  c = good(), c.k_max = 0;
  CHECK(rejects(c, BO_ERR_INVALID_ARGUMENT, "k_max must be"));
  c = good(), c.k_max = BO_MAX_K + 1u;
  CHECK(rejects(c, BO_ERR_INVALID_ARGUMENT, "k_max must be"));
  c = good(), c.init_mode = 2;
  CHECK(rejects(c, BO_ERR_INVALID_ARGUMENT, "init_mode must be"));
  c = good(), c.init_mode = BO_INIT_FIXED, c.init0 = 4, c.init1 = 4, c.initq = 0;
  CHECK(rejects(c, BO_ERR_INVALID_ARGUMENT, "init0 + init1 + initq must be"));
  c.initq = 1;
  CHECK(check(c, nullptr) == BO_OK);
  c.init0 = 0xFFFFFFFFu, c.init1 = 10u, c.initq = 0u;                     // wraps to 9 in 32 bits
  CHECK(rejects(c, BO_ERR_INVALID_ARGUMENT, "init0 + init1 + initq must be"));

  std::printf("%d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
