// benor_event_sizes.h -- host-side sizing of the workgroup-batched event kernel
// (benor_event_live.hip): its wave count, where its message pool lives, its pick
// hash table and its dynamic LDS.  Plain C++ with no HIP header, so that the
// planner, the launcher and a host program (tests/event_lds_check.cpp) read one
// set of functions.
#pragma once

#include <stdint.h>

namespace benor {

// The message pool of an event-level trial: 4N^2 + 64 u32 words (two rounds'
// broadcasts of N live senders in flight, and a batch's slack).
constexpr uint32_t event_pool_cap(uint32_t N) { return 4u * N * N + 64u; }

// The wave-per-trial and the workgroup-batched event kernels keep the pool in
// LDS when it is at most this many bytes (4N^2 + 64 u32: N <= 78).
constexpr uint64_t kEventBigLdsPool = 96u * 1024u;

// One workgroup's LDS on gfx950: no launch can ask for more
// (hipFuncSetAttribute refuses it).  The hash table is sized to leave room
// below it: the largest of 8, 4 and 2 slots per event lane that keeps the
// workgroup at or below kEventWgLdsTarget.
constexpr uint32_t kEventWgLdsLimit = 160u * 1024u;
constexpr uint32_t kEventWgLdsTarget = 150u * 1024u;
constexpr uint32_t kEventWgCtlBytes = 80u;         // sizeof(Ctl), benor_event_live.hip (asserted there)

constexpr uint32_t event_pow2_ceil(uint32_t v) {
  uint32_t r = 1u;
  while (r < v) r <<= 1;
  return r;
}

// Event waves of the workgroup: BENOR_LIVE_WAVES (1, 3, 7 or 15; anything else: not forced), or by N.
constexpr uint32_t kEventWg1MaxN = 32u;            // one event wave up to here,
constexpr uint32_t kEventWg3MaxN = 128u;           // three,
constexpr uint32_t kEventWg7MaxN = 512u;           // seven; fifteen above
constexpr uint32_t event_wg_waves_for(uint32_t N, uint32_t forced) {
  if (forced == 1u || forced == 3u || forced == 7u || forced == 15u) return forced;
  if (N <= kEventWg1MaxN) return 1u;
  if (N <= kEventWg3MaxN) return 3u;
  if (N <= kEventWg7MaxN) return 7u;
  return 15u;
}

// The register kernel (N <= kEventRegMaxN): the pool in 16 or 32 VGPRs of 64 messages (0: it does not fit), and
// its one-register mode while the pool starts within one of them (m N messages).
constexpr uint32_t kEventRegRegsSmall = 16u;
constexpr uint32_t kEventRegRegsLarge = 32u;
constexpr uint32_t kEventRegOneRegMsgs = 64u;
constexpr uint32_t event_reg_pool_regs(uint32_t ev_cap) {
  const uint32_t need = (ev_cap + 63u) / 64u;
  return need <= kEventRegRegsSmall ? kEventRegRegsSmall : (need <= kEventRegRegsLarge ? kEventRegRegsLarge : 0u);
}
constexpr bool event_reg_one_register(uint32_t m, uint32_t N) { return m * N <= kEventRegOneRegMsgs; }

// The lane-per-trial kernel (N <= kMaxEventN): its node sets are one u64 up to here, four above.
constexpr uint32_t kEventLaneOneWordMaxN = 64u;

constexpr bool event_wg_pool_in_lds(uint32_t ev_cap) { return (uint64_t)ev_cap * 4u <= kEventBigLdsPool; }

// Dynamic LDS of a workgroup of W event waves with a hash table of HS slots and
// `rstops` keys of a random /stop schedule (the kernel's carve-up, in its order).
constexpr uint32_t event_wg_bytes(uint32_t N, uint32_t W, uint32_t HS, uint32_t ev_cap, uint32_t rstops) {
  uint32_t b = (kEventWgCtlBytes + 15u) & ~15u;
  b += 16u * N + 8u * 64u * 6u + 8u * HS + 8u * 64u + 8u * rstops;   // ibox, killed/decided/comp, hash, Floyd set, keys
  b += 8u * N + 3u * 4u * 64u * W;                                  // smax; bmax, nxt, tvs
  b += 2u * ((N + 7u) & ~7u) * 2u + ((N + 15u) & ~15u);             // ks, cidx, xs
  if (event_wg_pool_in_lds(ev_cap)) b += 4u * ev_cap;
  return b;
}

// Slots per event lane (8, 4 or 2) of the pick hash table, and the table's slots.
constexpr uint32_t event_wg_slot_factor(uint32_t N, uint32_t W, uint32_t ev_cap, uint32_t rstops) {
  for (uint32_t f = 8u; f > 2u; f >>= 1)
    if (event_wg_bytes(N, W, event_pow2_ceil(f * 64u * W), ev_cap, rstops) <= kEventWgLdsTarget) return f;
  return 2u;
}
constexpr uint32_t event_wg_slots(uint32_t N, uint32_t W, uint32_t ev_cap, uint32_t rstops) {
  return event_pow2_ceil(event_wg_slot_factor(N, W, ev_cap, rstops) * 64u * W);
}

// The smallest table is taken without a look at the target; the planner checks
// the result against the device: event_wg_fits (plan_host refuses the plan
// otherwise, BO_ERR_UNSUPPORTED).
constexpr uint32_t event_wg_total_bytes(uint32_t N, uint32_t W, uint32_t ev_cap, uint32_t rstops) {
  return event_wg_bytes(N, W, event_wg_slots(N, W, ev_cap, rstops), ev_cap, rstops);
}
constexpr bool event_wg_fits(uint32_t N, uint32_t W, uint32_t ev_cap, uint32_t rstops) {
  return event_wg_total_bytes(N, W, ev_cap, rstops) <= kEventWgLdsLimit;
}

}  // namespace benor
