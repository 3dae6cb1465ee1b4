/*
 * benor.h -- C ABI of the MI355X-native Ben-Or consensus simulator (libbenor.so).
 *
 * This is the drop-in boundary for the reference's hot path
 * (viviendbk/ben-or-consensus-algorithm, src/nodes/node.ts:43-163, the
 * POST /message round loop).  Each entry point names the reference interface
 * it replaces.  Plain C types only: pointers, sizes, integers.  No torch or
 * HIP types appear in any signature; streams are passed as `void*`
 * (a hipStream_t, NULL = default stream).
 *
 * Value encoding (src/types.ts:1-8, `Value = 0 | 1 | "?"`):
 *     int8  0 -> 0,  1 -> 1,  2 -> "?",  -1 -> null (faulty node's x)
 * `decided`: -1 -> null, 0 -> false, 1 -> true;  `k`: -1 -> null.
 *
 * Threading: every function may be called from any host thread.  Calls on one
 * bo_network handle are serialised by a lock in the handle; bo_consensus_start
 * holds it only to read the start state and to merge the results, so /stop,
 * /getState and /status stay served while its kernel runs (the N-API addon
 * runs it on a worker thread).  bo_network_destroy must not overlap any other
 * call on the handle.  bo_plan_launch is asynchronous on its stream; all other
 * calls are synchronous.
 */
#ifndef BENOR_H
#define BENOR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BENOR_ABI_VERSION 8

/* Return codes.  The first two are the reference's two launch errors. */
enum {
    BO_OK = 0,
    BO_ERR_ARRAYS_DONT_MATCH = 1,   /* launchNodes.ts:10-11  Error("Arrays don't match") */
    BO_ERR_FAULTY_COUNT = 2,        /* launchNodes.ts:12-13  Error("faultyList doesnt have F faulties") */
    BO_ERR_INVALID_ARGUMENT = 3,
    BO_ERR_NO_DEVICE = 4,           /* no gfx950 device visible: the product never falls back to CPU */
    BO_ERR_HIP = 5,
    BO_ERR_OUT_OF_RANGE = 6,        /* node index >= N */
    BO_ERR_UNSUPPORTED = 7,         /* configuration outside what this build simulates */
    BO_ERR_ALREADY_STARTED = 8,     /* second start on one network: its inboxes persist (node.ts:29-30) */
    BO_ERR_INTERNAL = 9             /* a device-side invariant failed: the affected results are invalid */
};

/* Delivery model.  LOCKSTEP is the reference's semantics for its admissible
 * inputs (exactly F crash faults, launchNodes.ts:12-13): every live node
 * receives every live node's message in every phase.
 * RANDOM_DELIVERY generalises to f <= F crashed nodes: in every phase each
 * live receiver tallies the first N-F arrivals, a uniformly random subset of
 * exactly N-F of the N-f live senders drawn from Philox (no
 * reference counterpart -- the reference rejects f != F).  At f == F the two
 * modes give identical results. */
/* EVENT is message-granular: the reference's handler
 * (node.ts:45-158) delivery by delivery, in a seeded random order, with the
 * reference's mid-run GET /stop (node.ts:191-194) applied at scheduled
 * delivery counts.  Exactly F crash-faulty nodes; N <= 4096 (one lane per
 * trial up to N = 256, one wave per trial above).  Both /stop schedules --
 * explicit (crash_at) and random (crash_count, crash_window) -- work at every
 * N <= 4096.  (Under the validation knob BENOR_EVENT_FORM=wg a batch plan runs
 * the live runs' workgroup kernel, which keeps a random schedule's keys in
 * LDS: N near 4096 with more than some 1600 random stops is then refused with
 * BO_ERR_UNSUPPORTED when the plan is made.) */
/* RANDOM_TALLY is RANDOM_DELIVERY at the level of counts.  A receiver's rule
 * (node.ts:52-69, :88-113) reads only how many 0s and 1s its inbox holds, and
 * the inbox is a uniform (N-F)-subset of the m = N-f live senders, independent
 * per (receiver, round, phase): with K senders holding a 1, its count of 1s is
 * Hypergeometric(m, K, N-F).  The mode draws that count directly, from one
 * Philox block per receiver-round (stream 5) and a host-built table of 64-bit
 * CDF thresholds (bo_tally_cdf), so the law over histograms and per-node states
 * is RANDOM_DELIVERY's (thresholds rounded at 2^-64) while the random stream,
 * and so each seed's outcome, differs.  Scope: the quorum N-F must be odd and
 * no initial value may be "?" (every vote is then binary, no tally ties, no
 * coin is drawn); other configurations return BO_ERR_UNSUPPORTED -- run them in
 * BO_MODE_RANDOM_DELIVERY.  Validation is RANDOM_DELIVERY's (at most F
 * faulty).  At f == F it equals LOCKSTEP bit for bit. */
/* RANDOM_TALLY3 is RANDOM_TALLY without its scope: any quorum, "?" initial
 * values allowed.  A phase's votes fall into three classes -- K0 zeros, K1 ones,
 * Kq "?" (K0 + K1 + Kq = m) -- and a receiver's (c0, c1, c?) is multivariate
 * hypergeometric over them with N-F draws.  One class count comes from the same
 * table and the same stream-5 uniform as RANDOM_TALLY; the smallest class is then
 * walked member by member (selection sampling, exact integer draws from Philox
 * stream 6), and the third count is the remainder.  R-phase ties
 * propose "?", P-phase ties and empty tallies take the node's coin (the coin
 * stream of every batch mode).  A configuration inside RANDOM_TALLY's scope (odd
 * quorum, no live "?") runs RANDOM_TALLY's kernel and gives its results bit for
 * bit; at f == F the mode equals LOCKSTEP bit for bit, "?" and even m included.
 * Validation is RANDOM_DELIVERY's (at most F faulty). */
/* CRASH_TALLY is RANDOM_TALLY3 with crashes during the run: up
 * to F - f of the m0 = N - f initially-live nodes crash cleanly at step
 * boundaries, step 2(r-1) = the R-phase of round r, step 2(r-1)+1 = its P-phase.
 * A node that crashes at step s completed step s-1; from step s on it neither
 * sends nor receives (one that proposed and crashes at the P-step does not
 * vote).  At every step the senders and receivers are the alive set, m_s >= N-F
 * of them, the class sizes are counted over it, and a receiver's counts are
 * RANDOM_TALLY3's draw with m replaced by m_s -- one threshold table per
 * reachable live count.  The schedule is explicit (crash_at[i] = node i's step)
 * or random (crash_count distinct initially-live nodes at uniform steps below
 * crash_window, drawn per trial from Philox stream 7).  The run halts after the
 * round in which every alive node has decided; the outcome is over the nodes
 * alive at the end.  Validation is RANDOM_DELIVERY's, and f + (scheduled
 * crashes) <= F (BO_ERR_FAULTY_COUNT), so a quorum of live senders always exists;
 * crash_count > 0 needs crash_window >= 1.  The tables of all reachable live
 * counts together may hold at most BO_CRASH_TABLE_MAX_BYTES of thresholds
 * (BO_ERR_UNSUPPORTED beyond).  An empty schedule is RANDOM_TALLY3's plan: its
 * kernel choice and its results bit for bit; a schedule no crash of which is
 * reached gives RANDOM_TALLY3's results bit for bit on this mode's kernel.  A
 * crash here is clean: a crasher's last message reaches everybody or nobody;
 * CRASH_PARTIAL models the broadcast cut short.  Batch API only (no network API,
 * no `sweep`). */
/* CRASH_PARTIAL is CRASH_TALLY with partial broadcasts.  The
 * reference broadcasts in ascending node id (node.ts:72-80, :149-157, :173-185),
 * so a node that crashes during its step-s broadcast reaches a prefix of the
 * receivers.  Every scheduled crasher p has a cut, cut_p in [0, m0], counted over
 * the initially-live nodes in ascending node id (the compact index; faulty nodes
 * never receive and are not counted): crash_cut <= m0 gives every crasher that
 * cut, crash_cut == BO_CUT_RANDOM draws each crasher's cut per trial, uniform on
 * 0..m0, from Philox stream 8 keyed by the crasher's compact index; any other
 * value is BO_ERR_INVALID_ARGUMENT.  A node that crashes at step s does not
 * receive at step s; its step-s message -- its x at an R-step, the proposal it
 * formed at step s-1 at a P-step -- reaches exactly the receivers with compact
 * index c < cut_p.  Receiver c of the alive set A_s draws its N-F messages from
 * the pool A_s + H_c, H_c = { p crashing at s : c < cut_p }: CRASH_TALLY's draw
 * with m = m_s + |H_c| and the class sizes counted over that pool.  Everything
 * else -- schedule, validation, halting, outcome, per-node states, the table
 * limit -- is CRASH_TALLY's.  An empty schedule is RANDOM_TALLY3's plan;
 * crash_cut = 0 gives CRASH_TALLY's results bit for bit on this mode's kernel; an
 * explicit schedule of even steps with crash_cut = m0 gives CRASH_TALLY's results
 * for the schedule with every step one later.  The tables are those of every pool
 * size: with a fixed cut CRASH_TALLY's set, with random cuts every m0 - j, j = 0
 * .. the number of scheduled crashes below step 2 k_max.  Not modelled: a cut
 * per node given explicitly; subsets that are no prefix are CRASH_SUBSET's.  Batch
 * API only (no network API, no `sweep`). */
/* CRASH_SUBSET is CRASH_PARTIAL with the prefix replaced by an arbitrary subset
 * (DESIGN §4.3.5): the model of the paper, in which the last message of a process
 * that crashes in the middle of a step is received by any subset of the others,
 * here an independent one per receiver.  The configuration word that
 * CRASH_PARTIAL reads as crash_cut is read as crash_reach, a probability in units
 * of 2^-32; every 32-bit value is valid.  Crasher p's step-s message reaches
 * receiver c (p, c compact indices) iff crash_reach == UINT32_MAX or
 * word(p, c) < crash_reach, word(p, c) = element c & 3 of the Philox4x32-10 block
 * ctr = {trial_lo, trial_hi, p | (c >> 2) << 12, 9 << 24}, key = seed (stream 9;
 * p < 2^12, c >> 2 < 2^10).  The word is keyed by trial, crasher and receiver
 * only: not by the schedule's order, the step (a node crashes once per trial) or
 * the launch split.  crash_reach = 0 reaches nobody, UINT32_MAX everybody, and
 * neither draws a stream-9 word.  At step s receiver c of the alive set A_s has
 * H_c = { p crashing at s : p reaches c } and draws its N-F messages from the
 * pool A_s + H_c: CRASH_TALLY's draw with m = m_s + |H_c| and the class sizes
 * counted over that pool (the m = N-F shortcut per receiver).  Everything else --
 * schedule, validation, the class of a crasher's last message, halting, outcome,
 * per-node states, the table limit -- is CRASH_PARTIAL's.  An empty schedule is
 * RANDOM_TALLY3's plan; crash_reach = 0 gives CRASH_TALLY's results bit for bit
 * and crash_reach = UINT32_MAX gives CRASH_PARTIAL's with crash_cut = m0, both on
 * this mode's kernel.  The tables are those of every m0 - j, j = 0 .. the number
 * of scheduled crashes below step 2 k_max, at every reach.  Not modelled: a reach
 * per crasher, explicitly given reach masks.  Batch API only (no network API, no
 * `sweep`). */
/* BYZ_TALLY is RANDOM_TALLY3 with Byzantine senders: faulty
 * processes that keep talking and lie, a different value to each receiver if they
 * like (equivocation).  In this mode only, faulty[i] == 2 marks node i Byzantine;
 * faulty[i] == 1 is crashed from the start, as in every mode; any other non-zero
 * value is BO_ERR_INVALID_ARGUMENT.  With f crashed and b Byzantine nodes,
 * f + b <= F (BO_ERR_FAULTY_COUNT otherwise); the rest of validation is
 * RANDOM_DELIVERY's.  The m = N - f live nodes, honest and Byzantine together,
 * carry compact indices in ascending node id, so with b = 0 every Philox key is
 * RANDOM_TALLY3's.  f + b <= F gives m >= q + b, q = N-F: m > q whenever b > 0.
 * All m live nodes send at every step (a silent node is a crash); only the
 * h = m - b honest nodes receive and run the rule.  Honest receiver c draws q
 * messages uniformly from the m senders, independently per (receiver, round,
 * phase).  What a Byzantine message says is chosen by byz_strategy and byz_one, a
 * probability in units of 2^-32 (every value valid, 0: never, UINT32_MAX:
 * certainly):
 *   BO_BYZ_RANDOM: each Byzantine message carries 1 with probability
 *     byz_one / 2^32, else 0, independently per (trial, Byzantine sender,
 *     receiver, round, phase).  At the level of counts receiver c hears
 *     B1 ~ Binomial(b, p) ones and b - B1 zeros from the Byzantine senders that
 *     could reach it: B1 = #{ j : thr[j] <= u }, thr = bo_byz_cdf(b, byz_one), u
 *     from the Philox4x32-10 block ctr = {trial_lo, trial_hi, c, (r-1) | 10 << 24},
 *     key = seed (stream 10): the R-phase takes out[1] << 32 | out[0], the P-phase
 *     out[3] << 32 | out[2] (stream 5's convention).  byz_one = 0 gives B1 = 0,
 *     UINT32_MAX gives B1 = b, and neither draws a stream-10 word.
 *   BO_BYZ_OPPOSE: at each step every Byzantine message carries the value held by
 *     fewer honest senders at that step -- 0 if H1 > H0, 1 if H0 > H1 -- the same
 *     to every receiver; on H0 == H1 the step is BO_BYZ_RANDOM's with byz_one.
 *   BO_BYZ_BALANCE, BO_BYZ_SPLIT: the Byzantine senders see the receiver's inbox
 *     before they choose (below); byz_one is not read, every value is valid.
 *   Any other strategy is BO_ERR_INVALID_ARGUMENT.
 * H0, H1, Hq are the class sizes over the honest senders at the step (a sender's
 * x at an R-step, its proposal at a P-step; decided nodes keep sending).
 * Receiver c's (c0, c1) is RANDOM_TALLY3's draw among m senders with the class
 * sizes (H0 + b - B1, H1 + B1, Hq), from its stream-5 uniform and stream-6 walk.
 * Under BO_BYZ_BALANCE and BO_BYZ_SPLIT the Byzantine messages are
 * a class of their own inside the draw, which has two stages per (receiver c,
 * round r, phase):
 *   1. (h0, h1), the honest 0s and 1s heard, is RANDOM_TALLY3's draw among m
 *      senders with the class sizes (H0, H1, Hq + b), from the same stream-5
 *      uniform and stream-6 walk; rest = q - h0 - h1 messages come from the
 *      merged class of Hq honest "?" and b Byzantine senders.
 *   2. nB ~ Hypergeometric(Hq + b, b, rest) of them are Byzantine.  Hq == 0:
 *      nB = rest; rest == 0: nB = 0; neither draws.  Otherwise the smaller
 *      sub-class is walked by RANDOM_TALLY3's selection sampling: KW = min(b, Hq)
 *      members, the Byzantine class on a tie; member i is in the inbox iff
 *      v_i < rest - (members taken so far), v_i uniform below Hq + b - i by the
 *      same multiply-shift with exact rejection, from the words .x .y .z .w of
 *      the Philox4x32-10 blocks ctr = {trial_lo, trial_hi, c | blk << 12,
 *      (r-1) | phase << 16 | 11 << 24}, blk = 0, 1, .., key = seed (stream 11).
 *      nB is the number taken if the Byzantine class was walked, else rest
 *      minus it.
 * The nB Byzantine senders then see (h0, h1); l1 of them say 1 and nB - l1 say 0,
 * (c0, c1) = (h0 + nB - l1, h1 + l1), in both phases:
 *   BO_BYZ_BALANCE: the receiver's two tallies as equal as the lies allow: with
 *     d = h0 + nB - h1 (signed), l1 = 0 if d <= 0, else min(nB, floor(d / 2)).  A
 *     liveness attack and a heuristic, not the optimal adversary.
 *   BO_BYZ_SPLIT: l1 = nB if the receiver's compact index c is odd, else 0: the
 *     classic equivocation attack on agreement.
 * Rule, coins, k and the histogram layout are RANDOM_TALLY3's.  The run halts
 * after the round in which every honest node has decided; the outcome and the
 * common value are taken over the honest nodes.  bo_run_trial_states reports a
 * Byzantine node as {killed 0, x -1, decided -1, k -1}: alive, no protocol state.
 * b = 0 is RANDOM_TALLY3's plan at every byz_one and strategy: its kernel choice
 * and its results bit for bit.  Not modelled: Byzantine nodes together with
 * crashes during the run, lies that say "?", explicit lie masks.  Batch API only
 * (no network API; `sweep --mode byz` draws its (N, F, b) diagram). */
/* BYZ_RULE_B is BYZ_TALLY with the other rule of the same paper:
 * Ben-Or's Byzantine-tolerant Protocol B, stated for N > 5t, with F as its t.
 * Who is Byzantine (faulty[i] == 2) and f + b <= F, compact indices, senders and
 * receivers, the four strategies with their draws (streams 5, 6, 10 and 11),
 * byz_one and byz_strategy in the same union words, the coin stream, halting over
 * the honest nodes, the histogram layout and the per-node states are BYZ_TALLY's,
 * word for word, and so is every validation error.  Only the rule applied to a
 * receiver's counts (c0, c1) at a step differs:
 *   R-phase: propose 0 if 2 c0 > N + F, else 1 if 2 c1 > N + F, else "?" (both
 *     cannot hold: c0 + c1 <= N - F).
 *   P-phase: v = the value with the strictly larger count (none on c0 == c1, an
 *     empty tally included).  If v exists and c_v > F: x = v, and the node has
 *     decided iff 2 c_v > N + F (sticky; x is recomputed every round).  Otherwise
 *     x is the node's coin (RANDOM_TALLY3's coin stream).
 * F is not checked against N > 5F: outside the bound the mode measures what the
 * rule does there (N <= 3F never proposes, every trial ends in bin 0..2).  For
 * N > 5F the histogram's last bin and every bin R*3 + 2 stay 0, and a unanimous
 * honest start v lands in bin[1*3 + v], under every strategy.  b = 0 is valid and
 * is NOT RANDOM_TALLY3's plan, the rule differs: it runs this mode's kernel with
 * every step wave-uniform and no stream-10 or stream-11 word, the same results
 * at every byz_one and strategy (f = F then gives m == q).  Not modelled: what
 * BYZ_TALLY does not model, Bracha's protocol.  Other threshold rules, Protocol A
 * among them, run on this mode's plan through bo_plan_create_rule (below).
 * Batch API only (no network API; `sweep --mode byzb` draws its (N, F, b) diagram). */
/* BYZ_COIN is BYZ_TALLY word for word, and BYZ_RULE_B_COIN is BYZ_RULE_B word for
 * word, with a shared coin (Rabin's, or its weak form): the word
 * that other modes call crash_window is read as coin_common, the probability, in
 * units of 2^-32, that a round's coin is common to all honest nodes (every value
 * valid, 0: never, UINT32_MAX: certainly).  For trial t and round r the common-coin
 * block is Philox4x32-10 with ctr = {trial_lo, trial_hi, 0, (r-1) | 12 << 24}, key =
 * seed (stream 12).  Round r is common iff coin_common == UINT32_MAX or out[0] <
 * coin_common; its value is out[1] & 1.  In a common round every honest node whose
 * P-phase rule takes a coin (the reference rule's tie, Protocol B's "otherwise")
 * gets x = that one bit; in any other round each such node takes its own coin from
 * RANDOM_TALLY3's coin stream, as in the parent mode.  The word depends on the
 * trial and the round only: not on the launch split and not on which nodes take a
 * coin.  coin_common == 0 draws no stream-12 word and is the parent mode's plan
 * (BYZ_TALLY's, RANDOM_TALLY3's at b = 0, BYZ_RULE_B's): its kernel choice and its
 * results bit for bit.  coin_common != 0 with b = 0 is valid in both modes and runs
 * the shared-coin kernels; BYZ_COIN at b = 0 is then the reference's crash-tolerant
 * rule under random delivery with a shared coin.  Who is Byzantine, f + b <= F, the
 * four strategies and streams 5, 6, 10 and 11, halting over the honest nodes, the
 * histogram layout, the per-node states and every validation error are the parent
 * mode's.  Not modelled: an adversary that chooses the coin values in non-common
 * rounds, or that sees the coin before it lies; a coin shared by a subset of the
 * nodes; a shared coin in the lockstep, event and crash modes.  Batch API only
 * (no network API; `sweep --mode byz|byzb --coin-common p`). */
/* SCHED_TALLY is BYZ_COIN word for word, and SCHED_RULE_B is BYZ_RULE_B_COIN word
 * for word, except for how a receiver's inbox is composed: an
 * adversarial scheduler, the asynchronous model's adversary, chooses which q = N-F
 * messages every honest receiver hears at every step, and what each Byzantine
 * sender among them says.  Who is Byzantine (faulty[i] == 2), crashed
 * (faulty[i] == 1) and f + b <= F, compact indices over the m = N - f live nodes,
 * honest nodes alone receiving, Byzantine messages that carry 0 or 1, the init and
 * coin streams, coin_common in the crash_window word (stream 12; 0: every coin is
 * local), halting over the honest nodes, the histogram layout, the per-node states
 * and every validation error are those modes'.  byz_strategy names the scheduler's
 * aim and must be BO_BYZ_BALANCE or BO_BYZ_SPLIT (anything else is
 * BO_ERR_INVALID_ARGUMENT); byz_one is not read.  With (H0, H1, Hq) the class sizes
 * over the honest senders at the step (h = H0 + H1 + Hq >= q, since f + b <= F),
 * honest receiver c is delivered exactly q messages from distinct senders, honest
 * ones carrying their true value, and counts
 *   push(v):  c_v = min(q, H_v + b), rest = q - c_v, c_{1-v} = rest - min(rest, Hq)
 *     -- the most v that any inbox allows, and then the least 1 - v;
 *   even():   hq = min(q, Hq), r = q - hq, lo = r - min(r, H1 + b),
 *     hi = min(r, H0 + b), c0 = clamp((r + (c & 1)) >> 1, lo, hi), c1 = r - c0
 *     -- "?" messages first, then the two tallies as level as the senders allow:
 *     the smallest possible larger tally.
 *   BO_BYZ_SPLIT: push(c & 1) in both phases (odd compact indices driven to 1, even
 *     ones to 0: the attack on agreement).
 *   BO_BYZ_BALANCE: even() in both phases (the attack on liveness).
 * Both counts are realisable by an inbox at every class size, push is
 * lexicographically extreme and even attains the minimum of max(c0, c1) (checked by
 * brute force over every inbox for N <= 10).  No word of streams 5, 6, 10 or 11 is
 * drawn, and the plan holds no threshold table.  b = 0 is valid in both modes and is
 * NOT another mode's plan: crash-only adversarial scheduling.  coin_common == 0 keeps
 * the mode (its local-coin kernel).  With f = F and b = 0, m == q and the scheduler has
 * no choice: SCHED_TALLY then gives RANDOM_TALLY3's histogram and states bit for bit
 * (BYZ_COIN's at coin_common != 0), SCHED_RULE_B gives BYZ_RULE_B's (BYZ_RULE_B_COIN's).
 * The two strategies are per-step greedy aims, not the provably optimal attack on
 * either rule.  Not modelled: a scheduler that holds messages back across rounds
 * (every step's messages are delivered or dropped within the step), lies that say
 * "?", an adversary that sees coins before it schedules, crashes during the run.
 * Batch API only (no network API; `sweep --mode byz|byzb --delivery adversarial`). */
enum {
  BO_MODE_LOCKSTEP = 0,
  BO_MODE_RANDOM_DELIVERY = 1,
  BO_MODE_EVENT = 2,
  BO_MODE_RANDOM_TALLY = 3,
  BO_MODE_RANDOM_TALLY3 = 4,
  BO_MODE_CRASH_TALLY = 5,
  BO_MODE_CRASH_PARTIAL = 6,
  BO_MODE_CRASH_SUBSET = 7,
  BO_MODE_BYZ_TALLY = 8,
  BO_MODE_BYZ_RULE_B = 9,
  BO_MODE_BYZ_COIN = 10,
  BO_MODE_BYZ_RULE_B_COIN = 11,
  BO_MODE_SCHED_TALLY = 12,
  BO_MODE_SCHED_RULE_B = 13
};

/* BO_MODE_BYZ_TALLY, BO_MODE_BYZ_RULE_B and their shared-coin modes, byz_strategy. */
/* (2 is not a strategy: it stays BO_ERR_INVALID_ARGUMENT, as it was before BALANCE and SPLIT existed) */
enum { BO_BYZ_RANDOM = 0, BO_BYZ_OPPOSE = 1, BO_BYZ_BALANCE = 3, BO_BYZ_SPLIT = 4 };

/* BO_MODE_CRASH_PARTIAL, crash_cut: a cut per trial and crasher, uniform on 0..m0. */
#define BO_CUT_RANDOM 0xFFFFFFFFu

/* BO_MODE_CRASH_TALLY, BO_MODE_CRASH_PARTIAL, BO_MODE_CRASH_SUBSET: most bytes of 64-bit thresholds that the tables of a
 * plan's reachable live counts may hold together (512 MiB).  The table of
 * (m', q = N-F) holds the sum over K = 0..m' of min(K, q) - max(0, q - (m' - K))
 * thresholds. */
#define BO_CRASH_TABLE_MAX_BYTES (512ull << 20)

enum { BO_INIT_RANDOM = 0, BO_INIT_FIXED = 1 };

/* Largest network simulated per trial (N <= 4096 live + faulty nodes). */
#define BO_MAX_N 4096u
/* Largest round cap. */
#define BO_MAX_K 1024u

/* NodeState (src/types.ts:1-8), as served by GET /getState (node.ts:197-199). */
typedef struct bo_node_state {
    int8_t killed;    /* 0/1 */
    int8_t x;         /* -1 null, 0, 1, 2 '?' */
    int8_t decided;   /* -1 null, 0, 1 */
    int8_t pad;
    int32_t k;        /* -1 null */
} bo_node_state;

typedef struct bo_network bo_network;

/* ---- network API: one simulated network, the reference's public surface ---- */

/* launchNetwork(N, F, initialValues, faultyList)  (src/index.ts:4-14)
 *   -> launchNodes (src/nodes/launchNodes.ts:4-44).
 * Performs the reference's two validations in its order and returns their
 * codes; on success *out owns host-side node state (node.ts:21-26):
 * faulty -> {killed:1, x:null, decided:null, k:null}; live -> {0, init, 0, 0}.
 * init values: 0, 1 or 2 ('?').  No GPU work happens here. */
int bo_network_create(uint32_t N, uint32_t F,
                      const int8_t *initial_values, uint32_t n_initial_values,
                      const uint8_t *faulty_list, uint32_t n_faulty_list,
                      bo_network **out);

/* startConsensus(N)  (src/nodes/consensus.ts:3-8) -> GET /start on every node
 * (node.ts:167-188), then the POST /message round loop (node.ts:43-163) until
 * every live node has decided or k_max rounds ran -- one HIP kernel launch on
 * the calling thread's current device, synchronous.  `seed` keys the
 * per-node coins (node.ts:111).  Nodes already stopped act as crashed.
 * Runs once per network: the reference's round inboxes (node.ts:29-30) outlive
 * a run, so a second start is not a fresh consensus and returns
 * BO_ERR_ALREADY_STARTED.  A /stop served while the kernel runs takes effect
 * after it: the node keeps its final state and is killed. */
int bo_consensus_start(bo_network *net, uint64_t seed, uint32_t k_max);

/* startConsensus(N) with GET /stop requests that land while consensus runs
 * (node.ts:191-194 served mid-round; from then on the node drops every
 * message, node.ts:45).  stop_after[i] (n_stop_after == N entries) = number
 * of POST /message deliveries, network-wide, after which node i is stopped;
 * UINT32_MAX = not stopped.  Deliveries follow BO_MODE_EVENT's seeded order
 * (trial 0 of `seed`), so a schedule is reproducible.  With every entry
 * UINT32_MAX (or stop_after NULL) this is bo_consensus_start; otherwise the
 * run is message-granular on the event-level kernel (any N <= BO_MAX_N; a
 * schedule whose entries all name killed nodes is bo_consensus_start) and the
 * per-node states are its final ones, scheduled
 * stops included (killed, x / decided / k as of the stop).  The auto-stop and
 * one-start rules of bo_consensus_start apply. */
int bo_consensus_start_sched(bo_network *net, uint64_t seed, uint32_t k_max,
                             const uint32_t *stop_after, uint32_t n_stop_after);

/* startConsensus(N) as the reference runs it (consensus.ts:3-8, node.ts:167-188):
 * GET /start answers before consensus finishes, and GET /stop / GET /getState
 * requests served while it runs land in it (node.ts:191-199, :45).  Launches
 * the event-level kernel (seeded delivery order, trial 0 of `seed`, any
 * N <= BO_MAX_N; one workgroup of 1-15 event waves and a control wave) on its
 * own HIP stream and returns.  While it runs:
 *   - bo_node_stop / bo_consensus_stop also post to a host-mapped mailbox the
 *     kernel polls (every ~20 us): a request is applied before the next
 *     delivery, and that delivery count is recorded (bo_live_stop_events);
 *   - bo_get_state / bo_get_states answer at once from a snapshot the kernel
 *     writes at its next batch boundary (tens of microseconds): every node's
 *     state as of a delivery count, with the killed flag of every /stop already
 *     served (node.ts:191-194 sets it at once);
 *   - bo_status answers from the killed flags.
 * bo_consensus_wait (blocking) or bo_consensus_poll (not) end the run and merge
 * its final states; a request the kernel did not see before it finished is
 * ordered after the run, as for bo_consensus_start.  The one-start and
 * auto-stop rules of bo_consensus_start apply; bo_network_destroy waits for a
 * live run. */
int bo_consensus_start_live(bo_network *net, uint64_t seed, uint32_t k_max);

/* Wait for a live run (bo_consensus_start_live) and merge its final states;
 * BO_OK at once when none is in flight. */
int bo_consensus_wait(bo_network *net);

/* Without blocking: *running_out = 1 while a live run is in flight; once it
 * has ended, its final states are merged (as bo_consensus_wait) and
 * *running_out = 0. */
int bo_consensus_poll(bo_network *net, int *running_out);

/* After bo_consensus_wait: for each node, the delivery count at which a live
 * run applied its GET /stop, UINT32_MAX if it applied none (n == N).  Passed as
 * bo_consensus_start_sched's stop_after on a fresh network of the same launch,
 * with the same seed, it reproduces the live run exactly (counts below
 * UINT32_MAX - 1). */
int bo_live_stop_events(const bo_network *net, uint32_t *events_out, uint32_t n);

/* stopConsensus(N)  (consensus.ts:10-15) -> GET /stop on every node (node.ts:191-194). */
int bo_consensus_stop(bo_network *net);

/* GET /stop on one node (node.ts:191-194): killed = true (and, during a live
 * run, posted to the running kernel). */
int bo_node_stop(bo_network *net, uint32_t node);

/* GET /getState (node.ts:197-199): the node's current state, answered at once
 * (during a live run: from a snapshot, see bo_get_states). */
int bo_get_state(const bo_network *net, uint32_t node, bo_node_state *out);

/* GET /getState on every node at once (__test__/tests/utils.ts:14-20), out[n],
 * n == N.  During a live run: one snapshot of the running kernel, taken at a
 * batch boundary after *events_out POST /message deliveries -- exactly oracle
 * (iii) truncated there, plus the killed flags of /stop requests served but
 * not yet applied; a snapshot taken within the last 500 us answers later
 * requests too (N concurrent GET /getState cost one).  Otherwise the
 * network's states and *events_out = UINT64_MAX.  events_out may be NULL. */
int bo_get_states(const bo_network *net, bo_node_state *out, uint32_t n, uint64_t *events_out);

/* GET /status (node.ts:33-39): returns 500 ("faulty") or 200 ("live"), or a
 * negative BO_ERR_* code. */
int bo_status(const bo_network *net, uint32_t node);

uint32_t bo_network_size(const bo_network *net);

/* server.close() for every server (benorconsensus.test.ts:14-29). */
void bo_network_destroy(bo_network *net);

/* ---- batch API: many independent trials of one network shape ---- */

typedef struct bo_trials_cfg {
    uint32_t N, F;            /* network size; fault parameter (quorum N-F, decide on > F) */
    uint32_t k_max;           /* round cap, 1..BO_MAX_K */
    uint32_t init_mode;       /* BO_INIT_RANDOM: iid Bernoulli(1/2) per live node; BO_INIT_FIXED */
    uint32_t mode;            /* BO_MODE_* */
    union {                   /* one word, the layout of the struct is that of ABI version 8 */
        uint32_t crash_cut;   /* CRASH_PARTIAL: every crasher's cut, 0..m0, or BO_CUT_RANDOM */
        uint32_t crash_reach; /* CRASH_SUBSET: the probability, in units of 2^-32, that a crasher's last message
                                 reaches a receiver (0: never, UINT32_MAX: certainly); every value is valid */
        uint32_t byz_one;     /* BYZ_TALLY, BYZ_RULE_B, BYZ_COIN, BYZ_RULE_B_COIN: the probability, in units of 2^-32, that a Byzantine message carries 1
                                 (0: never, UINT32_MAX: certainly); every value is valid.  SCHED_TALLY, SCHED_RULE_B: not read */
    };                        /* the other modes ignore it */
    uint64_t seed;            /* Philox4x32-10 key */
    const uint8_t *faulty;    /* host [N]; non-zero = faulty: exactly F set (LOCKSTEP, EVENT), at most F (RANDOM_DELIVERY, RANDOM_TALLY, RANDOM_TALLY3, CRASH_TALLY, CRASH_PARTIAL, CRASH_SUBSET);
                                 BYZ_TALLY, BYZ_RULE_B, BYZ_COIN, BYZ_RULE_B_COIN, SCHED_TALLY and SCHED_RULE_B alone read the value: 1 crashed from the start, 2 Byzantine, together at most F */
    const int8_t *init;       /* host [N]; used when init_mode == BO_INIT_FIXED */
    /* EVENT mode: GET /stop schedule.  crash_at[i] = number of deliveries
     * after which node i is stopped (UINT32_MAX = never), or, when crash_at is
     * NULL, crash_count distinct live nodes stopped at uniform delivery counts
     * in [0, crash_window), drawn per trial from Philox.
     * CRASH_TALLY, CRASH_PARTIAL and CRASH_SUBSET modes: the crash schedule in steps.  crash_at[i] = the step
     * at which node i crashes (UINT32_MAX = never; entries of faulty nodes are
     * ignored), or, when crash_at is NULL, crash_count distinct initially-live
     * nodes at uniform steps in [0, crash_window), drawn per trial.
     * The other modes ignore the three fields, except that BYZ_TALLY, BYZ_RULE_B, BYZ_COIN and
     * BYZ_RULE_B_COIN read the crash_count word as byz_strategy, and the last two the crash_window
     * word as coin_common; SCHED_TALLY and SCHED_RULE_B read both words so. */
    const uint32_t *crash_at; /* host [N] or NULL */
    union {                   /* one word, the layout of the struct is that of ABI version 8 */
        uint32_t crash_count;
        uint32_t byz_strategy; /* BYZ_TALLY, BYZ_RULE_B, BYZ_COIN, BYZ_RULE_B_COIN: a BO_BYZ_* strategy; SCHED_TALLY, SCHED_RULE_B: BO_BYZ_BALANCE or BO_BYZ_SPLIT */
    };
    union {                   /* one word, the layout of the struct is that of ABI version 8 */
        uint32_t crash_window;
        uint32_t coin_common; /* BYZ_COIN, BYZ_RULE_B_COIN, SCHED_TALLY, SCHED_RULE_B: the probability, in units of 2^-32, that a round's coin is
                                 common to all honest nodes (0: never, UINT32_MAX: certainly); every value is valid */
    };
} bo_trials_cfg;

/* Histogram length for a round cap: (k_max + 1) * 3 + 1 uint64 bins.
 *   bin[R*3 + v], 1 <= R <= k_max : every live node decided after round R, common x = v
 *                                   (v = 2: decided values differ)
 *   bin[0*3 + v]                  : not every live node decided within k_max rounds;
 *                                   v = common x, or 2 if they differ
 *   bin[(k_max+1)*3]              : trials whose decided values differ (agreement violations) */
uint32_t bo_hist_len(uint32_t k_max);

typedef struct bo_plan bo_plan;

/* Validate a trial configuration and upload its tables to the current device. */
int bo_plan_create(const bo_trials_cfg *cfg, bo_plan **out);

/* Run global trial ids [trial_begin, trial_begin + trial_count) and ADD their
 * outcomes into hist_dev (device pointer, bo_hist_len(k_max) uint64).
 * Asynchronous on `stream` (hipStream_t or NULL).  A plan owns per-plan
 * device scratch (the matrix-core kernels' deferred-trial lists, the event
 * mode's message pools), so launches of ONE plan must be issued from one host
 * thread at a time and ordered on one stream (or separated by a
 * synchronisation); concurrent launches need one plan each. */
int bo_plan_launch(bo_plan *plan, uint64_t trial_begin, uint64_t trial_count,
                   uint64_t *hist_dev, void *stream);

/* Same, blocking, host histogram (added into hist_host).  Includes bo_plan_check. */
int bo_plan_run(bo_plan *plan, uint64_t trial_begin, uint64_t trial_count, uint64_t *hist_host);

/* Synchronise the device and report device-side invariant failures of this
 * plan's launches since the last check: BO_ERR_INTERNAL when a matrix-core
 * launch deferred more trials than its segment holds (their outcomes are then
 * missing from the histogram).  No reference counterpart: call it after a
 * series of bo_plan_launch before trusting their histograms. */
int bo_plan_check(bo_plan *plan);

/* The roofline's algorithmic unit: VALU popcount words that the per-receiver
 * tallies of one live node-round need, m = live nodes, M = m - (number of "?"
 * initial values) binary votes.  LOCKSTEP / EVENT: the R-phase counts c1
 * (c0 = M - c1); the P-phase counts c1 when M is odd (no tie, so no "?"
 * proposal: c0 = m - c1) and c0, c1 otherwise -- 2 or 3 x ceil(m/32).
 * RANDOM_DELIVERY: both values in both phases, 4 x ceil(m/32).  RANDOM_TALLY,
 * RANDOM_TALLY3, CRASH_TALLY, CRASH_PARTIAL, CRASH_SUBSET, BYZ_TALLY, BYZ_RULE_B, their shared-coin modes, SCHED_TALLY and SCHED_RULE_B answer RANDOM_DELIVERY's
 * unit, the work they stand in for (the crash modes with m = the initially-live count,
 * BYZ_TALLY and BYZ_RULE_B with m = the live nodes, honest and Byzantine, as bo_plan_live_nodes reports it). */
uint64_t bo_plan_popc_words_per_node_round(const bo_plan *plan);
uint32_t bo_plan_live_nodes(const bo_plan *plan);

/* Kernel families.  BO_KERNEL_MFMA counts inboxes on the matrix cores
 * (e2m1 operands, exact f32 sums): lockstep, 64 < m <= 1024, m odd, an even
 * number of "?" initial values and m > 2F -- every trial halts in round 1.
 * Its roofline unit is receiver-sender terms, 2m per live node-round. */
enum {
  BO_KERNEL_NONE = -1, /* no live node: outcomes need no kernel */
  BO_KERNEL_BLOCKED = 0,
  BO_KERNEL_W = 1,
  BO_KERNEL_RANDOM = 2,
  BO_KERNEL_EVENT = 4,  /* event level: one lane per trial (N <= 256), one wave per trial (N > 256, live runs) */
  BO_KERNEL_LANE = 6,
  BO_KERNEL_MFMA = 7,
  BO_KERNEL_MFMA_SMALL = 8, /* packed matrix-core kernel: 2 <= m <= 32, m > F, no "?" initial value;
                              64 * min(32/m, 8) trials per wave iteration, block-diagonal e2m1 products;
                              launches of fewer than 5 * 10^5 trials run the lane kernel
                              (BENOR_SMALL_MIN_TRIALS overrides) */
  BO_KERNEL_TALLY = 9,      /* BO_MODE_RANDOM_TALLY: one wave per trial, per-receiver hypergeometric counts
                              by binary search in a table row staged in LDS; batch and per-node-state
                              launches alike, no overflow or deferral state; also what
                              BO_MODE_RANDOM_TALLY3 runs inside that mode's scope */
  BO_KERNEL_TALLY3 = 10,    /* BO_MODE_RANDOM_TALLY3 outside RANDOM_TALLY's scope (even quorum or a live "?"
                              initial value): one wave per trial, three vote classes -- one count from the
                              table, the smallest class walked by selection sampling, coins on ties */
  BO_KERNEL_TALLY_CRASH = 11, /* BO_MODE_CRASH_TALLY with a non-empty schedule: TALLY3's draw over the alive
                              set of each step -- alive, x, proposal and decided ballot planes per trial,
                              one table per reachable live count (an empty schedule runs RANDOM_TALLY3's
                              kernel choice) */
  BO_KERNEL_TALLY_PARTIAL = 12, /* BO_MODE_CRASH_PARTIAL with a non-empty schedule: TALLY_CRASH's step run once
                              per segment of receivers that hear the same crashers (the cuts of the step's
                              crashers are the boundaries), one table per pool size */
  BO_KERNEL_TALLY_SUBSET = 13, /* BO_MODE_CRASH_SUBSET with a non-empty schedule: per receiver group a reach pass
                              (which of the step's crashers each lane hears, Philox stream 9), then
                              TALLY_CRASH's wave-uniform draw for the lanes that hear none of them and one
                              per-lane draw, each lane searching the row of its own pool in global memory,
                              for the others; one table per pool size */
  BO_KERNEL_TALLY_BYZ = 14, /* BO_MODE_BYZ_TALLY with b > 0 Byzantine nodes: TALLY3's draw among all m live
                              senders for the honest receivers (a constant honest plane in place of the alive
                              plane); a step whose Byzantine messages are the same for every receiver is
                              wave-uniform with its row staged in LDS, otherwise every lane draws its own
                              Binomial count of lying 1s (Philox stream 10) and searches the row of its own
                              class sizes in global memory; one table, (m, q) (b = 0 runs RANDOM_TALLY3's
                              kernel choice) */
  BO_KERNEL_TALLY_BYZ_B = 15, /* BO_MODE_BYZ_RULE_B with an honest node, b = 0 included: TALLY_BYZ's two trial loops
                              instantiated with Protocol B's rule (thresholds at (N + F) / 2 and F + 1); the same
                              LDS layout, launch bounds, grid and state launch */
  BO_KERNEL_TALLY_BYZ_COIN = 16, /* BO_MODE_BYZ_COIN with coin_common != 0, b = 0 included: TALLY_BYZ's two trial loops
                              instantiated with the shared coin (one stream-12 block per round, drawn when an
                              honest node first takes a coin; no per-node coin in a common round) */
  BO_KERNEL_TALLY_BYZ_B_COIN = 17, /* BO_MODE_BYZ_RULE_B_COIN with coin_common != 0: TALLY_BYZ_B's with the shared coin */
  BO_KERNEL_TALLY_SCHED = 18, /* BO_MODE_SCHED_TALLY with an honest node and coin_common == 0: one wave per trial on
                              TALLY_BYZ's planes; a step's counts are the scheduler's closed form, one pair per
                              receiver parity, computed wave-uniformly from the popcounted class sizes -- no table,
                              no search, no walk; what is left per node-round is the rule's ballots and the coins */
  BO_KERNEL_TALLY_SCHED_B = 19, /* BO_MODE_SCHED_RULE_B with coin_common == 0: the same loop with Protocol B's rule */
  BO_KERNEL_TALLY_SCHED_COIN = 20, /* BO_MODE_SCHED_TALLY with coin_common != 0: the same loop with the shared coin */
  BO_KERNEL_TALLY_SCHED_B_COIN = 21 /* BO_MODE_SCHED_RULE_B with coin_common != 0 */
};

/* The kernel family bo_plan_launch runs for this plan.  (The per-node-state
 * launch behind the network API runs the W kernel for an MFMA shape and the
 * lane kernel for an MFMA_SMALL shape.) */
int bo_plan_kernel(const bo_plan *plan);

/* The same choice for a configuration, made on the host (no device needed):
 * *kernel_out = BO_KERNEL_* (BO_KERNEL_NONE for no live node).  Returns
 * bo_plan_create's validation error for an invalid cfg. */
int bo_kernel_for(const bo_trials_cfg *cfg, int *kernel_out);

/* Tests and diagnosis (no reference counterpart: SURVEY §8f #4's "first N-F arrivals", drawn as
 * oracle/benor_oracle.c oracle_delivery_mask defines them): the delivered-sender masks that the plan's
 * random-delivery kernel draws in one phase of one trial, masks_out[m][W], m = bo_plan_live_nodes and
 * W = ceil(m / 64).  Row c is the mask of the receiver with compact live index c over compact sender
 * indices -- oracle_delivery_mask(seed, trial, live_ids[c], round, phase, m, N - F, D)'s D, bits >= m
 * clear.  The read-out kernel calls the trial kernel's own sampling function (Floyd or Bernoulli +
 * fix-up, the instantiation the plan dispatches to) with the plan's own parameters and LDS layout.
 * Only for a plan whose bo_plan_kernel is BO_KERNEL_RANDOM, phase 0 (R) or 1 (P) and round 1 .. 0x7FFF
 * (the counter's round field); anything else is BO_ERR_INVALID_ARGUMENT.  Synchronous; on no hot path.
 * An added entry: the ABI version and every struct are unchanged. */
int bo_plan_delivery_masks(bo_plan *plan, uint64_t trial, uint32_t round, uint32_t phase, uint64_t *masks_out);

void bo_plan_destroy(bo_plan *plan);

/* One-shot convenience: create plan, run trial ids [trial_begin, +trial_count), destroy. */
int bo_run_trials(const bo_trials_cfg *cfg, uint64_t trial_begin, uint64_t trial_count,
                  uint64_t *hist_host);

/* Per-node final states of one trial (trial id `trial`), nodes_out[N]. */
int bo_run_trial_states(const bo_trials_cfg *cfg, uint64_t trial, bo_node_state *nodes_out,
                        uint32_t *rounds_out);

/* Row K of the RANDOM_TALLY table for (m, q): *lo_out, and its hi-lo thresholds
 * into thr_out[cap] (*n_out = their number; BO_ERR_INVALID_ARGUMENT if cap is short
 * or K > m or q > m).  Exactly what bo_plan_create uploads.  Host only, no device
 * needed.  lo = max(0, q - (m - K)), hi = min(K, q); threshold j is
 * min(2^64 - 1, floor(CDF(lo + j) * 2^64)) of Hypergeometric(m, K, q), built in
 * double; a draw u (uniform 64 bits) gives the count lo + #{ j : thr[j] <= u }. */
int bo_tally_cdf(uint32_t m, uint32_t q, uint32_t K, uint32_t *lo_out,
                 uint64_t *thr_out, uint32_t cap, uint32_t *n_out);

/* The BYZ_TALLY thresholds of Binomial(b, p), p = byz_one / 2^32: thr_out[j] =
 * min(2^64 - 1, floor(CDF(j) * 2^64)), j = 0 .. b-1, built in double (*n_out = b;
 * BO_ERR_INVALID_ARGUMENT if cap < b or b > BO_MAX_N).  Exactly what bo_plan_create
 * uploads.  Host only, no device needed.  A draw u (uniform 64 bits) gives the
 * number of Byzantine messages that carry 1, B1 = #{ j : thr[j] <= u }. */
int bo_byz_cdf(uint32_t b, uint32_t byz_one, uint64_t *thr_out, uint32_t cap, uint32_t *n_out);

/* ---- lumped API: the adversarial scheduler at the level of classes ----
 *
 * SCHED_TALLY and SCHED_RULE_B with nodes replaced by classes.  Under the adversarial
 * scheduler a step's (c0, c1) takes one value per parity of the receiver's compact index,
 * and every honest receiver of one parity applies the same rule to the same counts.  So in
 * every round a whole parity class proposes, adopts or decides the same value, or takes the
 * round's common coin, or each member takes its own local coin and the number of ones is
 * Binomial(h_pi, 1/2).  A trial is a Markov chain on (a_0, a_1, dec_0, dec_1): a_pi = the
 * honest nodes of parity pi with x = 1, dec_pi = the sticky decided flag of parity pi.  No
 * faulty[] array, no per-node state, no BO_MAX_N: N up to 2^24, one trial per lane, a cost
 * per trial-round that does not depend on N.  This is no BO_MODE_* and no BO_KERNEL_*:
 * bo_trials_cfg, the modes 0..13 and the variants 0..21 are as they were.
 *
 * A configuration: N, F, f crashed and b Byzantine nodes, byz_even of the Byzantine nodes at
 * an even compact index (compact indices: the m = N - f live nodes in ascending node id),
 * the rule (0: the reference's, SCHED_TALLY's; 1: Protocol B, SCHED_RULE_B's), the strategy
 * (BO_BYZ_BALANCE or BO_BYZ_SPLIT), coin_common, k_max, the seed and the initial values.
 * Derived: q = N - F, h_0 = ceil(m / 2) - byz_even, h_1 = floor(m / 2) - (b - byz_even),
 * h = h_0 + h_1 (>= q >= 1).
 *
 * Round r, for pi in {0, 1}:
 *   R-phase.  The honest class sizes (H0, H1, Hq): in round 1 the initial values'; later
 *     H1 = a_0 + a_1, H0 = h - H1, Hq = 0.  Parity pi's counts are SCHED_TALLY's closed form
 *     for a receiver c with c & 1 = pi -- push(pi) under SPLIT, even() under BALANCE, with
 *     (q, H0, H1, Hq, b) -- and it proposes by the rule's R-step: the reference's 0 if c0 > c1,
 *     1 if c1 > c0, else "?"; Protocol B's 0 if 2 c0 > N + F, 1 if 2 c1 > N + F, else "?".  Its
 *     h_pi members all propose alike.
 *   P-phase.  The class sizes are those of the two proposals, weighted by h_pi; the counts
 *     are the same closed forms; the rule's P-step follows (the reference's: c0 > F decides 0,
 *     else c1 > F decides 1, else the strict majority, else the coin; Protocol B's: the strict
 *     majority v with c_v > F is adopted, and decided iff 2 c_v > N + F, else the coin).  A
 *     parity that adopts or decides v gets a_pi = v h_pi, and dec_pi sticks on a deciding
 *     count.  If a parity with h_pi > 0 takes the coin, the round's stream-12 block is read
 *     exactly as BYZ_COIN reads it (coin_common == 0 draws none; common iff coin_common ==
 *     UINT32_MAX or out[0] < coin_common, the bit out[1] & 1): in a common round with bit v,
 *     a_pi = v h_pi; otherwise a_pi ~ Binomial(h_pi, 1/2), drawn as below.
 *   Halting and outcome.  The trial stops after the round in which dec_pi holds for every
 *     parity with h_pi > 0, or after k_max rounds.  K = a_0 + a_1 of the h honest nodes hold 1;
 *     the bins are those of every batch mode, over bo_hist_len(k_max).
 * Initial values: BO_INIT_RANDOM draws H1 ~ Binomial(h, 1/2), H0 = h - H1, Hq = 0;
 * BO_INIT_FIXED gives the three counts init0 + init1 + initq = h.  Only the totals matter:
 * round 1's proposals do not read a node's own x, and every x is rewritten in its P-phase.
 *
 * The Binomial(n, 1/2) draw (Philox stream 13), exact up to the rounding of 64-bit
 * thresholds.  n = the sum of 2^k over its set bits, and the draw is the sum of independent
 * B_k ~ Binomial(2^k, 1/2) over them.  The set bits are taken in ascending k; the j-th set
 * bit (j = 0, 1, ..) uses the j-th 64-bit word of the draw.  Parity pi's draw in round r reads
 * the Philox4x32-10 blocks ctr = {trial_lo, trial_hi, 16 pi + (j >> 1), r | 13 << 24}, key =
 * seed; word j is out[1] << 32 | out[0] for even j and out[3] << 32 | out[2] for odd j (stream
 * 5's convention).  n < 2^25 has at most 25 set bits: 13 blocks, below 16.  The initial draw
 * is parity 0's with n = h and r = 0.  No word is used twice, and the word of a clear bit is
 * never drawn.  From a word u: for k <= 6, B_k = popcount(u & (2^(2^k) - 1)) (the whole word
 * at k = 6); for 7 <= k <= 24, B_k = lo_k + #{ i : thr_k[i] <= u }, the table of
 * bo_binom_half_cdf.
 *
 * The law over histograms is that of SCHED_TALLY / SCHED_RULE_B for the same (N, F, f, b,
 * placement parity) with thresholds rounded at 2^-64; the random stream, and so each seed's
 * outcome, differs -- unless no local coin and no random start is drawn (fixed initial
 * values with coin_common == UINT32_MAX: stream 12 is shared, no stream-13 word is read),
 * where every trial's bins and round count are those modes'.  Not modelled: per-node
 * states, the network API, the strategies BO_BYZ_RANDOM and BO_BYZ_OPPOSE, random delivery. */
typedef struct bo_lumped_cfg {
    uint32_t N, F;            /* network size, 1..2^24; fault parameter, F < N (quorum N-F) */
    uint32_t f, b;            /* crashed from the start; Byzantine; f + b <= F */
    uint32_t byz_even;        /* the Byzantine nodes at an even compact index: <= min(b, ceil(m/2)), b - byz_even <= floor(m/2) */
    uint32_t rule;            /* 0: the reference's rule (SCHED_TALLY), 1: Protocol B (SCHED_RULE_B) */
    uint32_t strategy;        /* BO_BYZ_BALANCE or BO_BYZ_SPLIT */
    uint32_t coin_common;     /* the probability, in units of 2^-32, that a round's coin is common (0: never, UINT32_MAX: certainly) */
    uint32_t k_max;           /* round cap, 1..BO_MAX_K */
    uint32_t init_mode;       /* BO_INIT_RANDOM: H1 ~ Binomial(h, 1/2); BO_INIT_FIXED: the three counts below */
    uint32_t init0, init1, initq;   /* BO_INIT_FIXED: honest nodes that start at 0, 1 and "?"; their sum is h */
    uint32_t reserved;        /* not read */
    uint64_t seed;            /* Philox4x32-10 key */
} bo_lumped_cfg;

typedef struct bo_lumped_state {
    uint32_t a[2];            /* honest nodes of even / odd compact index with x = 1 at the end */
    uint8_t dec[2];           /* whether that parity has decided (0 for a parity without an honest node) */
    uint8_t pad[2];
    uint32_t rounds;          /* the round in which every parity had decided, 0 if k_max ran out first */
} bo_lumped_state;

/* Validate a configuration.  Host only, no device needed; the error text names what is wrong. */
int bo_lumped_check(const bo_lumped_cfg *cfg);

/* Run global trial ids [trial_begin, trial_begin + trial_count) and ADD their outcomes into
 * hist_host (bo_hist_len(k_max) uint64).  Blocking, on the current device.  A trial's outcome
 * depends on its id alone: not on the launch split, the grid or the lane that ran it. */
int bo_lumped_run(const bo_lumped_cfg *cfg, uint64_t trial_begin, uint64_t trial_count, uint64_t *hist_host);

/* The final state of one trial, from a one-trial launch. */
int bo_lumped_trial(const bo_lumped_cfg *cfg, uint64_t trial, bo_lumped_state *out);

/* The thresholds of Binomial(2^k, 1/2), 7 <= k <= 24: thr_out[i] = min(2^64 - 1,
 * floor(CDF(lo + i) * 2^64)), trimmed to the counts whose threshold is neither 0 nor
 * saturated (*lo_out = the first of them, *n_out their number; BO_ERR_INVALID_ARGUMENT if
 * cap is short or k is outside 7..24).  Built by the pmf's ratio recurrence outward from
 * the mode in long double, the lower half summed from the tail and normalised by the
 * symmetric total, the upper half its mirror image 2^64 - ceil(.).  A draw u (uniform 64
 * bits) gives the count lo + #{ i : thr[i] <= u }.  Exactly what bo_lumped_run uploads.
 * Host only, no device needed. */
int bo_binom_half_cdf(uint32_t k, uint32_t *lo_out, uint64_t *thr_out, uint32_t cap, uint32_t *n_out);

/* ---- threshold rules: Protocol A and any other rule of three words ----
 *
 * The reference's rule, Protocol B and Ben-Or's crash-tolerant Protocol A (N > 2t) are all
 * threshold rules on a receiver's counts (c0, c1): one rule of three runtime words covers
 * them.  Let v be the value with the strictly larger count (none on c0 == c1, an empty tally
 * included):
 *   R-phase: propose v iff v exists and 2 c_v > propose_gt2; otherwise propose "?".
 *   P-phase: if v exists and c_v > adopt_gt: x = v, and the node has decided iff also
 *     2 c_v > decide_gt2 (sticky; x is recomputed every round).  Otherwise x is the node's
 *     coin, under the mode's coin policy (RANDOM_TALLY3's coin stream; in a common round of a
 *     shared coin, that round's bit).
 * Presets:
 *   Protocol A (bo_rule_protocol_a)  (N, 0, 2F): propose v iff more than N / 2 of the
 *     messages heard carry v (the reference proposes the bare majority of the N - F heard);
 *     adopt the strict majority of the proposals, decide on more than F of them.  At most one
 *     value is proposed in a round by the honest nodes, whatever the scheduler delivers, so
 *     with b = 0 and N > 2F no trial ends in the last bin.  Not built for Byzantine nodes.
 *   Protocol B (bo_rule_protocol_b)  (N + F, F, N + F): BYZ_RULE_B's rule at every count.
 *   (0, 0, 2F): the reference's rule whenever N <= 3F + 1.  Beyond, a receiver can count
 *     more than F of both values (N = 3F + 2: c0 = c1 = F + 1), where the reference decides 0
 *     and this rule takes the coin; a rule that prefers 0 there is not modelled.
 * Every word is at most 2^31 - 1 and reserved is 0; anything else is
 * BO_ERR_INVALID_ARGUMENT with a text that names the word.
 *
 * The _rule entries run an existing mode with Protocol B's rule replaced by the words.
 * bo_plan_create_rule accepts cfg->mode BO_MODE_BYZ_RULE_B, BO_MODE_BYZ_RULE_B_COIN or
 * BO_MODE_SCHED_RULE_B only (any other mode: BO_ERR_INVALID_ARGUMENT); the plan is that
 * mode's plan word for word -- validation, strategies, streams and tables, coin_common
 * (mode 11 at coin_common == 0 is mode 9's plan), b = 0 valid and no other mode's plan,
 * per-node states, the histogram layout, bo_plan_launch / bo_plan_run / bo_plan_check --
 * and bo_plan_kernel reports the base plan's variant (15, 17, 19 or 21); only the rule
 * differs, and bo_plan_rule tells.  With bo_rule_protocol_b's words every histogram and
 * state is the plain plan's bit for bit, on kernel entries of their own.
 * bo_run_trial_states_rule is bo_run_trial_states for such a plan (nodes_out holds n >= N
 * entries).  The bo_lumped_*_rule entries are bo_lumped_* with the words in the place of
 * cfg->rule, which is not read.  ABI version and every struct above are unchanged. */
typedef struct bo_rule {
    uint32_t propose_gt2;     /* R-phase: propose v iff 2 c_v > propose_gt2 */
    uint32_t adopt_gt;        /* P-phase: adopt v iff c_v > adopt_gt */
    uint32_t decide_gt2;      /* ... and decide iff also 2 c_v > decide_gt2 */
    uint32_t reserved;        /* 0 */
} bo_rule;

/* The presets above (BO_ERR_INVALID_ARGUMENT if out is NULL or a word would exceed 2^31 - 1).
 * Host only, no device needed. */
int bo_rule_protocol_a(uint32_t N, uint32_t F, bo_rule *out);
int bo_rule_protocol_b(uint32_t N, uint32_t F, bo_rule *out);

int bo_plan_create_rule(const bo_trials_cfg *cfg, const bo_rule *rule, bo_plan **out);
int bo_run_trial_states_rule(const bo_trials_cfg *cfg, const bo_rule *rule, uint64_t trial, bo_node_state *nodes_out,
                             uint32_t n);
/* 1 and the rule (out may be NULL) if the plan runs a replaced rule, else 0; negative error code for a NULL plan. */
int bo_plan_rule(const bo_plan *plan, bo_rule *out);
int bo_lumped_check_rule(const bo_lumped_cfg *cfg, const bo_rule *rule);
int bo_lumped_run_rule(const bo_lumped_cfg *cfg, const bo_rule *rule, uint64_t trial_begin, uint64_t trial_count,
                       uint64_t *hist_host);
int bo_lumped_trial_rule(const bo_lumped_cfg *cfg, const bo_rule *rule, uint64_t trial, bo_lumped_state *out);

/* ---- diagnostics ---- */

/* Time the v_bcnt_u32_b32 peak microbenchmark: returns popcount words/s
 * measured on the current device over `iters` launches (0 on error). */
double bo_popc_peak(uint32_t iters);

/* Time the matrix-core peak microbenchmark (v_mfma_scale_f32_32x32x64_f8f6f4,
 * e2m1 operands, the BO_KERNEL_MFMA instruction): multiply-adds per second on
 * the current device over `iters` launches (0 on error). */
double bo_mfma_peak(uint32_t iters);

/* Message of the last error on this thread ("" if none). */
const char *bo_last_error(void);

int bo_abi_version(void);

/* Digest of the kernel sources this library was built from (16 hex digits).
 * Profiles record it, so a measured figure is only quoted for the same kernels. */
const char *bo_kernel_version(void);

#ifdef __cplusplus
}
#endif

#endif /* BENOR_H */
