// benor_rule.h -- the one place that knows the threshold rule (struct bo_rule,
// include/benor.h): what a receiver does with its counts (c0, c1)
// under the three runtime words (propose_gt2, adopt_gt, decide_gt2).  With v the
// value of the strictly larger count (none on c0 == c1, an empty tally included):
//   R-phase: propose v iff v exists and 2 c_v > propose_gt2, else "?";
//   P-phase: if v exists and c_v > adopt_gt, x = v, decided iff also 2 c_v > decide_gt2;
//            otherwise x is the node's coin.
// This header is that rule on scalars, the two presets (Ben-Or's Protocol A and
// Protocol B) and the validation of a rule.  Plain C++17 over benor.h, host and
// device, no HIP: RuleT of benor_tally_common.h wraps it in ballots for the
// node-level kernels, lumped::RuleT of benor_lumped.h runs it on the two receiver
// parities, the runtime validates with it, and tests/rule_check.cpp checks it on the
// host against the compile-time rules written out by hand.  Counts are at most 2^24
// (lumped::kMaxN) and every word at most 2^31 - 1: 2 c_v and the compares stay in 32 bits.
#pragma once

#include <stdint.h>

#include "benor.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BENOR_RULE_HD __host__ __device__ inline
#else
#define BENOR_RULE_HD inline
#endif

namespace benor {
namespace rule {

constexpr uint32_t kNone = 2u;                     // "?" as a proposal, "takes the coin" as a P-step
constexpr uint32_t kMaxWord = 0x7FFFFFFFu;         // the largest value of a threshold word

// The R-step: the proposal, 0, 1 or kNone.
BENOR_RULE_HD uint32_t r_step(const bo_rule &t, uint32_t c0, uint32_t c1) {
  const uint32_t cv = c1 > c0 ? c1 : c0;
  if (c0 == c1 || 2u * cv <= t.propose_gt2) return kNone;
  return c1 > c0 ? 1u : 0u;
}

// The P-step: the new x, 0 or 1, or kNone for "takes the coin"; `decided`: whether these counts decide.
BENOR_RULE_HD uint32_t p_step(const bo_rule &t, uint32_t c0, uint32_t c1, bool &decided) {
  const uint32_t cv = c1 > c0 ? c1 : c0;
  const bool adopt = c0 != c1 && cv > t.adopt_gt;
  decided = adopt && 2u * cv > t.decide_gt2;
  return adopt ? (c1 > c0 ? 1u : 0u) : kNone;
}

// ---- the presets
// Protocol A, the crash-tolerant protocol of Ben-Or's paper (N > 2t, t = F): propose v iff more than N / 2
// of the messages heard carry v; adopt the strict majority of the proposals, decide on more than F of them.
BENOR_RULE_HD bo_rule protocol_a(uint32_t N, uint32_t F) { return bo_rule{N, 0u, 2u * F, 0u}; }
// Protocol B (N > 5t): RuleB of benor_tally_common.h and of benor_lumped.h at every count.
BENOR_RULE_HD bo_rule protocol_b(uint32_t N, uint32_t F) { return bo_rule{N + F, F, N + F, 0u}; }
// Whether a preset's words fit (N + F and 2 F at most kMaxWord).
BENOR_RULE_HD bool preset_fits(uint32_t N, uint32_t F) {
  return (uint64_t)N + F <= kMaxWord && 2ull * F <= kMaxWord;
}

// ---- validation (host and device need none of each other)
// BO_OK, or BO_ERR_INVALID_ARGUMENT with *msg set to a text that names the word.
inline int check(const bo_rule &t, const char **msg) {
  const char *dummy;
  if (!msg) msg = &dummy;
  *msg = "";
  if (t.propose_gt2 > kMaxWord) return *msg = "bo_rule: propose_gt2 must be at most 2^31 - 1", BO_ERR_INVALID_ARGUMENT;
  if (t.adopt_gt > kMaxWord) return *msg = "bo_rule: adopt_gt must be at most 2^31 - 1", BO_ERR_INVALID_ARGUMENT;
  if (t.decide_gt2 > kMaxWord) return *msg = "bo_rule: decide_gt2 must be at most 2^31 - 1", BO_ERR_INVALID_ARGUMENT;
  if (t.reserved != 0u) return *msg = "bo_rule: reserved must be 0", BO_ERR_INVALID_ARGUMENT;
  return BO_OK;
}

}  // namespace rule
}  // namespace benor
