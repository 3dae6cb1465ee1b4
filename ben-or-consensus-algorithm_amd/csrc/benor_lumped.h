// benor_lumped.h -- the class-level ("lumped") chain of the adversarial scheduler
// (bo_lumped_*, include/benor.h): modes 12 and 13 with nodes replaced
// by the two receiver parities.  Under the scheduler every honest receiver of one parity
// applies the same rule to the same counts, so a trial is a Markov chain on
// (a_0, a_1, dec_0, dec_1): a_pi the honest nodes of parity pi with x = 1, dec_pi the
// parity's sticky decided flag.  This header is that chain on scalars -- the scheduler's
// two closed forms, both rules' R- and P-steps (and the threshold rule of benor_rule.h as
// a third rule type, bo_lumped_*_rule), one round, the outcome bins -- with the
// Binomial(n, 1/2) draw over a source of 64-bit words and the validation of a
// configuration.  Plain C++17 over benor.h, no HIP: benor_lumped.hip runs it one trial
// per lane, the runtime validates with it, and tests/lumped_check.cpp checks it on the
// host against values written out by hand.  No floating point anywhere.
#pragma once

#include <stdint.h>

#include "benor.h"
#include "benor_rule.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BENOR_LUMPED_HD __host__ __device__ inline
#else
#define BENOR_LUMPED_HD inline
#endif

namespace benor {
namespace lumped {

constexpr uint32_t kMaxN = 1u << 24;               // counts stay below 2^25: 2 c > N + F in 32 bits
constexpr uint32_t kStreamBinom = 13u;             // Philox stream of the Binomial words
constexpr uint32_t kPopcountMaxK = 6u;             // Binomial(2^k, 1/2), k <= 6: a popcount of 2^k bits of the word
constexpr uint32_t kTableMinK = 7u, kTableMaxK = 24u;   // beyond: a search in the thresholds of bo_binom_half_cdf
constexpr uint32_t kTables = kTableMaxK - kTableMinK + 1u;

// ---- the scheduler's closed forms, a receiver of parity `odd`
struct Counts {
  uint32_t c0, c1;
};

// The most v that any inbox allows, and then the least 1 - v.
BENOR_LUMPED_HD Counts push(uint32_t v, uint32_t q, uint32_t H0, uint32_t H1, uint32_t Hq, uint32_t nb) {
  const uint32_t Hv = v ? H1 : H0;
  const uint32_t cv = Hv + nb < q ? Hv + nb : q;
  const uint32_t rest = q - cv;
  const uint32_t co = rest - (rest < Hq ? rest : Hq);
  return v ? Counts{co, cv} : Counts{cv, co};
}

// "?" first, then the two tallies as level as the senders allow.
BENOR_LUMPED_HD Counts even(uint32_t odd, uint32_t q, uint32_t H0, uint32_t H1, uint32_t Hq, uint32_t nb) {
  const uint32_t hq = q < Hq ? q : Hq;
  const uint32_t r = q - hq;
  const uint32_t lo = r - (r < H1 + nb ? r : H1 + nb);
  const uint32_t hi = r < H0 + nb ? r : H0 + nb;   // lo <= hi: r <= H0 + H1 + 2 nb
  uint32_t c = (r + odd) >> 1;
  c = c < lo ? lo : c;
  c = c > hi ? hi : c;
  return Counts{c, r - c};
}

BENOR_LUMPED_HD Counts counts(uint32_t strategy, uint32_t odd, uint32_t q, uint32_t H0, uint32_t H1, uint32_t Hq,
                              uint32_t nb) {
  return strategy == BO_BYZ_SPLIT ? push(odd, q, H0, H1, Hq, nb) : even(odd, q, H0, H1, Hq, nb);
}

// ---- the two rules on a receiver's counts
// r: the proposal, 0, 1 or kNone ("?").  p: the new x, 0 or 1, or kNone for "takes the coin";
// `decided`: whether these counts decide.
constexpr uint32_t kNone = 2u;

struct RuleRef {                                   // the reference's crash-tolerant rule (node.ts:46-158)
  static constexpr uint32_t kRule = 0u;
  static BENOR_LUMPED_HD uint32_t r(uint32_t c0, uint32_t c1, uint32_t, uint32_t) {
    return c0 > c1 ? 0u : (c1 > c0 ? 1u : kNone);
  }
  static BENOR_LUMPED_HD uint32_t p(uint32_t c0, uint32_t c1, uint32_t, uint32_t F, bool &decided) {
    decided = c0 > F || c1 > F;
    if (c0 > F) return 0u;
    if (c1 > F) return 1u;
    return c1 > c0 ? 1u : (c0 > c1 ? 0u : kNone);  // a tie, an empty tally included, takes the coin
  }
};

struct RuleB {                                     // Ben-Or's Protocol B, t = F
  static constexpr uint32_t kRule = 1u;
  static BENOR_LUMPED_HD uint32_t r(uint32_t c0, uint32_t c1, uint32_t N, uint32_t F) {
    return 2u * c0 > N + F ? 0u : (2u * c1 > N + F ? 1u : kNone);
  }
  static BENOR_LUMPED_HD uint32_t p(uint32_t c0, uint32_t c1, uint32_t N, uint32_t F, bool &decided) {
    const uint32_t cv = c1 > c0 ? c1 : c0;
    const bool adopt = c0 != c1 && cv > F;
    decided = adopt && 2u * cv > N + F;
    return adopt ? (c1 > c0 ? 1u : 0u) : kNone;
  }
};

struct RuleT {                                     // a threshold rule of three runtime words (benor_rule.h)
  static constexpr uint32_t kRule = 2u;
  bo_rule t;
  BENOR_LUMPED_HD uint32_t r(uint32_t c0, uint32_t c1, uint32_t, uint32_t) const { return rule::r_step(t, c0, c1); }
  BENOR_LUMPED_HD uint32_t p(uint32_t c0, uint32_t c1, uint32_t, uint32_t, bool &decided) const {
    return rule::p_step(t, c0, c1, decided);
  }
};

// ---- a configuration's derived sizes
struct Shape {
  uint32_t N, F, q, nb;       // q = N - F, nb = b
  uint32_t h[2], hh;          // the honest nodes of either parity of the compact index, and together
  uint32_t strategy;
};

BENOR_LUMPED_HD Shape shape_of(const bo_lumped_cfg &c) {
  const uint32_t m = c.N - c.f;
  Shape s;
  s.N = c.N, s.F = c.F, s.q = c.N - c.F, s.nb = c.b;
  s.h[0] = (m + 1u) / 2u - c.byz_even;
  s.h[1] = m / 2u - (c.b - c.byz_even);
  s.hh = s.h[0] + s.h[1];
  s.strategy = c.strategy;
  return s;
}

// ---- one round
// The chain's state between rounds: the honest class sizes the next R-phase reads (round 1: the initial
// values'; later H1 = a_0 + a_1, H0 = h - H1), a[], and the decided flags (bit pi).
struct State {
  uint32_t H0, H1;
  uint32_t a[2];
  uint32_t dec;
};

// What a coin state says: 0 not drawn, 1 every node its own coin, 2 | v the round is common with bit v.
// `src.common(r)` answers 1 or 2 | v for round r; `src.binom(n, pi, r)` draws Binomial(n, 1/2) from parity
// pi's words of round r.  Neither is called unless a parity with a node takes the coin.
// Returns whether every parity that has a node has decided.  `rule`: the rule's object -- empty for the two
// compile-time rules, whose r and p are static, the words for RuleT.
template <class Rule, class Src>
BENOR_LUMPED_HD bool round(const Rule &rule, const Shape &s, uint32_t r, State &st, Src &src) {
  const uint32_t Hq = s.hh - st.H0 - st.H1;
  uint32_t P0 = 0u, P1 = 0u;                       // R-phase: a parity's h_pi members all propose alike
  for (uint32_t pi = 0u; pi < 2u; ++pi) {
    const Counts c = counts(s.strategy, pi, s.q, st.H0, st.H1, Hq, s.nb);
    const uint32_t prop = rule.r(c.c0, c.c1, s.N, s.F);
    P0 += prop == 0u ? s.h[pi] : 0u;
    P1 += prop == 1u ? s.h[pi] : 0u;
  }
  const uint32_t Pq = s.hh - P0 - P1;
  uint32_t act[2];                                 // P-phase
  bool take = false;
  for (uint32_t pi = 0u; pi < 2u; ++pi) {
    const Counts c = counts(s.strategy, pi, s.q, P0, P1, Pq, s.nb);
    bool decided;
    act[pi] = rule.p(c.c0, c.c1, s.N, s.F, decided);
    if (s.h[pi] != 0u && decided) st.dec |= 1u << pi;   // sticky
    take = take || (s.h[pi] != 0u && act[pi] == kNone);
  }
  const uint32_t coin = take ? src.common(r) : 0u;
  for (uint32_t pi = 0u; pi < 2u; ++pi) {
    if (s.h[pi] == 0u) st.a[pi] = 0u;
    else if (act[pi] != kNone) st.a[pi] = act[pi] * s.h[pi];
    else if (coin & 2u) st.a[pi] = (coin & 1u) * s.h[pi];
    else st.a[pi] = src.binom(s.h[pi], pi, r);
  }
  st.H1 = st.a[0] + st.a[1];
  st.H0 = s.hh - st.H1;
  return ((st.dec & 1u) != 0u || s.h[0] == 0u) && ((st.dec & 2u) != 0u || s.h[1] == 0u);
}
template <class Rule, class Src>
BENOR_LUMPED_HD bool round(const Shape &s, uint32_t r, State &st, Src &src) {
  return round(Rule{}, s, r, st, src);
}

// ---- the outcome (trial_end's bins, benor_tally_common.h)
// K of the h honest nodes hold x = 1: v = 0 / 1 if they agree, 2 if not (h = 0: 2, undecided).  Bin R * 3 + v if
// all decided in round R, else bin v; `violation`: the last bin counts the trial too.
BENOR_LUMPED_HD uint32_t outcome_bin(uint32_t K, uint32_t h, bool all_dec, uint32_t R, bool &violation) {
  const uint32_t v = h == 0u ? 2u : ((K != 0u && K != h) ? 2u : (K != 0u ? 1u : 0u));
  if (h == 0u) all_dec = false;
  violation = all_dec && v == 2u;
  return all_dec ? R * 3u + v : v;
}

// ---- the Binomial(n, 1/2) draw
// n by its set bits, ascending: the j-th set bit, k, takes the j-th word u and adds B_k ~ Binomial(2^k, 1/2) --
// for k <= 6 the popcount of the word's low 2^k bits, beyond it lo_k + #{ i : thr_k[i] <= u } from the table
// of bo_binom_half_cdf.  `word(j)` is called once per set bit, in order; `tables.count(k, u)` answers the
// table's B_k.  n < 2^25.
template <class Words, class Tables>
BENOR_LUMPED_HD uint32_t binom_half(uint32_t n, Words &word, const Tables &tables) {
  uint32_t sum = 0u, j = 0u;
  for (uint32_t k = 0u; (n >> k) != 0u; ++k) {
    if (!((n >> k) & 1u)) continue;
    const uint64_t u = word(j++);
    if (k <= kPopcountMaxK) sum += (uint32_t)__builtin_popcountll(k == kPopcountMaxK ? u : u & ((1ull << (1u << k)) - 1ull));
    else sum += tables.count(k, u);
  }
  return sum;
}

// #{ i < n : T[i] <= u } for ascending T[0..n): halving steps from the power of two at or above n, no
// divergent loop bound but the table's own.  n = 0 gives 0.
BENOR_LUMPED_HD uint32_t count_le(const uint64_t *T, uint32_t n, uint64_t u) {
  uint32_t st = 1u;
  while (st < n) st <<= 1;
  uint32_t pos = 0u;
  for (; st != 0u; st >>= 1) {
    const uint32_t i = pos + st - 1u;
    if (i < n && T[i] <= u) pos += st;
  }
  return pos;
}

// The tables of k = kTableMinK .. kTableMaxK as one array: table k is thr[off[k - 7] .. off[k - 6]) with
// its least count lo[k - 7]; off holds kTables + 1 entries, lo kTables.
struct TableDir {
  const uint64_t *thr;
  const uint32_t *off;
  const uint32_t *lo;
  BENOR_LUMPED_HD uint32_t count(uint32_t k, uint64_t u) const {
    const uint32_t i = k - kTableMinK;
    return lo[i] + count_le(thr + off[i], off[i + 1u] - off[i], u);
  }
};

// ---- validation (host and device need none of each other)
// BO_OK, or the error code with *msg set to a text that names what is wrong.  `own_rule`: the configuration runs
// the rule it names (c.rule); the bo_lumped_*_rule entries carry a threshold rule instead and do not read the word.
inline int check(const bo_lumped_cfg &c, const char **msg, bool own_rule = true) {
  const char *dummy;
  if (!msg) msg = &dummy;
  *msg = "";
  if (c.N < 1u || c.N > kMaxN) return *msg = "bo_lumped: N must be 1 .. 2^24", BO_ERR_INVALID_ARGUMENT;
  if (c.F >= c.N) return *msg = "bo_lumped: F must be below N (a quorum q = N - F of at least 1)", BO_ERR_INVALID_ARGUMENT;
  if ((uint64_t)c.f + c.b > c.F)
    return *msg = "bo_lumped needs at most F nodes crashed or Byzantine (f + b <= F)", BO_ERR_FAULTY_COUNT;
  const uint32_t m = c.N - c.f, even_n = (m + 1u) / 2u, odd_n = m / 2u;
  if (c.byz_even > c.b || c.byz_even > even_n)
    return *msg = "bo_lumped: byz_even must be at most b and at most ceil((N - f) / 2), the even compact indices",
           BO_ERR_INVALID_ARGUMENT;
  if (c.b - c.byz_even > odd_n)
    return *msg = "bo_lumped: b - byz_even must be at most floor((N - f) / 2), the odd compact indices",
           BO_ERR_INVALID_ARGUMENT;
  if (c.strategy != BO_BYZ_BALANCE && c.strategy != BO_BYZ_SPLIT)
    return *msg = "bo_lumped: strategy must be BO_BYZ_BALANCE or BO_BYZ_SPLIT", BO_ERR_INVALID_ARGUMENT;
  if (own_rule && c.rule > 1u) return *msg = "bo_lumped: rule must be 0 (the reference's) or 1 (Protocol B)", BO_ERR_INVALID_ARGUMENT;
  if (c.k_max < 1u || c.k_max > BO_MAX_K) return *msg = "bo_lumped: k_max must be 1 .. 1024", BO_ERR_INVALID_ARGUMENT;
  if (c.init_mode != BO_INIT_RANDOM && c.init_mode != BO_INIT_FIXED)
    return *msg = "bo_lumped: init_mode must be BO_INIT_RANDOM or BO_INIT_FIXED", BO_ERR_INVALID_ARGUMENT;
  if (c.init_mode == BO_INIT_FIXED && (uint64_t)c.init0 + c.init1 + c.initq != (uint64_t)(c.N - c.f - c.b))
    return *msg = "bo_lumped: init0 + init1 + initq must be h = N - f - b, the honest nodes", BO_ERR_INVALID_ARGUMENT;
  return BO_OK;
}

}  // namespace lumped
}  // namespace benor
