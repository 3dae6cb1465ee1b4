"""Python mirror of the reference's public surface, over libbenor.so (C ABI).

The reference (viviendbk/ben-or-consensus-algorithm) exposes, in TypeScript:

    launchNetwork(N, F, initialValues, faultyList)   src/index.ts:4-14
    startConsensus(N) / stopConsensus(N)             src/nodes/consensus.ts:3-15
    GET /status, /getState on port 3000 + i          src/nodes/node.ts:33-39, :197-199
    getNodesState(N), reachedFinality(states)        __test__/tests/utils.ts:14-24

The same names, argument meanings and errors are provided here (the
JavaScript mirror for Node lives in ../js/).  As in the reference, one network
is "listening" at a time: startConsensus(N) / stopConsensus(N) / getNodesState(N)
address the network most recently launched.  Consensus itself runs as one HIP
kernel on the current device; there is no CPU fallback -- without the built
library or a gfx950 device every compute call raises.
"""
from __future__ import annotations

import ctypes
import os
import secrets
import struct
from typing import Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BENOR_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "lib", "libbenor.so")

BO_OK = 0
BO_ERR_ARRAYS_DONT_MATCH = 1
BO_ERR_FAULTY_COUNT = 2
BO_ERR_INVALID_ARGUMENT = 3
BO_ERR_NO_DEVICE = 4
BO_ERR_HIP = 5
BO_ERR_OUT_OF_RANGE = 6
BO_ERR_UNSUPPORTED = 7
BO_ERR_ALREADY_STARTED = 8
BO_MODE_LOCKSTEP = 0
BO_MODE_RANDOM_DELIVERY = 1
BO_MODE_EVENT = 2
BO_MODE_RANDOM_TALLY = 3       # random delivery at the level of counts (odd quorum, no "?" initial value)
BO_MODE_RANDOM_TALLY3 = 4      # ... any quorum, "?" allowed: three vote classes, ties and coins (a superset of mode 3)
BO_MODE_CRASH_TALLY = 5        # mode 4 with crashes during the run: crash_at[i] = node i's step (2(r-1): R-phase of
                               # round r, +1: its P-phase), or crash_count nodes at random steps below crash_window
BO_MODE_CRASH_PARTIAL = 6      # mode 5 with partial broadcasts: a crasher's last message reaches the receivers whose
                               # compact index is below its cut (crash_cut = 0..m0 for every crasher, or CUT_RANDOM)
BO_MODE_CRASH_SUBSET = 7       # mode 6 with an arbitrary subset for the prefix: a crasher's last message reaches each
                               # receiver independently with probability crash_reach / 2^32 (REACH_ALL: certainly)
BO_MODE_BYZ_TALLY = 8          # mode 4 with Byzantine senders: byzantine[i] marks node i (it sends at every step and
                               # lies, it never receives); byz_one / 2^32 is the probability that a Byzantine message
                               # carries 1, byz_strategy BYZ_RANDOM (independently per receiver), BYZ_OPPOSE, or one of
                               # the two that read the receiver's inbox and ignore byz_one, BYZ_BALANCE and BYZ_SPLIT
BO_MODE_BYZ_RULE_B = 9         # mode 8 under Ben-Or's Byzantine-tolerant rule (Protocol B, F as its t): propose v iff
                               # 2 c_v > N + F; adopt the strict majority v iff c_v > F and decide iff 2 c_v > N + F,
                               # else the coin.  Everything else, byzantine / byz_one / byz_strategy included, is mode
                               # 8's; b = 0 runs this mode's kernel (it is not mode 4's plan)
BO_MODE_BYZ_COIN = 10          # mode 8 with a shared coin: coin_common / 2^32 is the probability that a round's coin is common
                               # to all honest nodes (Philox stream 12, keyed by trial and round); in such a round
                               # every node that takes a coin gets the same bit.  0 is mode 8's plan (mode 4's at b = 0)
BO_MODE_BYZ_RULE_B_COIN = 11   # mode 9 with the same shared coin; coin_common = 0 is mode 9's plan
BO_MODE_SCHED_TALLY = 12       # mode 10 under an adversarial scheduler: the adversary, not a draw, picks the q messages each
                               # honest receiver hears at every step and what the Byzantine senders among them say;
                               # byz_strategy BYZ_SPLIT (receivers of odd index driven to 1, even ones to 0) or
                               # BYZ_BALANCE ("?" first, then the tallies as level as the senders allow); byz_one is not
                               # read; b = 0 and coin_common = 0 keep the mode (no other mode's plan); no table
BO_MODE_SCHED_RULE_B = 13      # mode 11 under the same scheduler (Protocol B's rule)
COIN_ALL = 0xFFFFFFFF          # coin_common: every round's coin is common
BYZ_RANDOM = 0                 # byz_strategy: each Byzantine message is 1 with probability byz_one / 2^32 (equivocation)
BYZ_OPPOSE = 1                 # ... every one carries the value fewer honest senders hold (byz_one's step on a tie)
BYZ_BALANCE = 3                # ... the Byzantine messages a receiver drew make its two tallies as equal as they can
BYZ_SPLIT = 4                  # ... they all say 1 to a receiver of odd compact index and 0 to one of even index
BO_BYZ_RANDOM, BO_BYZ_OPPOSE, BO_BYZ_BALANCE, BO_BYZ_SPLIT = BYZ_RANDOM, BYZ_OPPOSE, BYZ_BALANCE, BYZ_SPLIT   # include/benor.h's names
CRASH_TABLE_MAX_BYTES = 512 << 20   # modes 5, 6 and 7: thresholds of the tables of all reachable live counts, at most
CUT_RANDOM = 0xFFFFFFFF        # crash_cut: a cut per trial and crasher, uniform on 0..m0 (Philox stream 8)
REACH_ALL = 0xFFFFFFFF         # crash_reach: every crasher reaches every receiver (no Philox stream 9 word is drawn)
NEVER = 0xFFFFFFFF             # crash_at entry: never stopped / never crashes
BO_INIT_RANDOM = 0
BO_INIT_FIXED = 1
BO_KERNEL_NONE = -1
BO_KERNEL_BLOCKED = 0
BO_KERNEL_W = 1
BO_KERNEL_RANDOM = 2
BO_KERNEL_EVENT = 4
BO_KERNEL_LANE = 6
BO_KERNEL_MFMA = 7
BO_KERNEL_MFMA_SMALL = 8
BO_KERNEL_TALLY = 9
BO_KERNEL_TALLY3 = 10
BO_KERNEL_TALLY_CRASH = 11
BO_KERNEL_TALLY_PARTIAL = 12
BO_KERNEL_TALLY_SUBSET = 13
BO_KERNEL_TALLY_BYZ = 14
BO_KERNEL_TALLY_BYZ_B = 15
BO_KERNEL_TALLY_BYZ_COIN = 16
BO_KERNEL_TALLY_BYZ_B_COIN = 17
BO_KERNEL_TALLY_SCHED = 18
BO_KERNEL_TALLY_SCHED_B = 19
BO_KERNEL_TALLY_SCHED_COIN = 20
BO_KERNEL_TALLY_SCHED_B_COIN = 21
KERNEL_NAMES = {BO_KERNEL_NONE: "none", BO_KERNEL_BLOCKED: "blocked popcount", BO_KERNEL_W: "W popcount",
                BO_KERNEL_RANDOM: "random delivery", BO_KERNEL_EVENT: "event level", BO_KERNEL_LANE: "lane",
                BO_KERNEL_MFMA: "matrix core (e2m1 MFMA)", BO_KERNEL_MFMA_SMALL: "packed matrix core (e2m1 MFMA, m <= 32)",
                BO_KERNEL_TALLY: "count-level random delivery (hypergeometric tallies)",
                BO_KERNEL_TALLY3: "count-level random delivery, three vote classes (hypergeometric tally + walk)",
                BO_KERNEL_TALLY_CRASH: "count-level random delivery with crashes during the run (a table per live count)",
                BO_KERNEL_TALLY_PARTIAL: "count-level random delivery with crashes cutting a broadcast short "
                                         "(a segment of receivers per cut)",
                BO_KERNEL_TALLY_SUBSET: "count-level random delivery with crashes whose last broadcast reaches a random "
                                        "subset (a reach pass per group, per-lane draws for the receivers it reaches)",
                BO_KERNEL_TALLY_BYZ: "count-level random delivery with Byzantine senders (an honest plane, wave-uniform "
                                     "steps from a staged row, per-lane Binomial lies and draws otherwise)",
                BO_KERNEL_TALLY_BYZ_B: "count-level random delivery with Byzantine senders under Ben-Or's Byzantine-"
                                       "tolerant rule (the same two trial loops with thresholds at (N + F) / 2 and F + 1)",
                BO_KERNEL_TALLY_BYZ_COIN: "count-level random delivery with Byzantine senders and a shared coin (the same "
                                          "two trial loops, one wave-uniform coin block per round)",
                BO_KERNEL_TALLY_BYZ_B_COIN: "count-level random delivery with Byzantine senders under Ben-Or's Byzantine-"
                                            "tolerant rule with a shared coin",
                BO_KERNEL_TALLY_SCHED: "count-level delivery under an adversarial scheduler (closed-form counts per "
                                       "receiver parity: no table, no search, no walk)",
                BO_KERNEL_TALLY_SCHED_B: "count-level delivery under an adversarial scheduler, Ben-Or's Byzantine-tolerant rule",
                BO_KERNEL_TALLY_SCHED_COIN: "count-level delivery under an adversarial scheduler with a shared coin",
                BO_KERNEL_TALLY_SCHED_B_COIN: "count-level delivery under an adversarial scheduler, Ben-Or's Byzantine-"
                                              "tolerant rule with a shared coin"}
BO_MAX_N = 4096
BO_MAX_K = 1024

# Environment knobs libbenor reads (csrc/benor_runtime.cpp kKnobs):
# none is needed in production; each forces a choice the planner makes itself.
# bench.py refuses to report while any is set.
KNOBS = {
    "BENOR_NO_MFMA": "validation", "BENOR_NO_MFMA_BIG": "validation", "BENOR_BIG_FORM": "validation",
    "BENOR_COOP_BW": "validation", "BENOR_SMALL_MIN_TRIALS": "validation", "BENOR_BLOCKS_PER_CU": "tuning",
    "BENOR_EVENT_LANES_PER_CU": "tuning", "BENOR_TEST_DEFER_SEG_CAP": "test", "BENOR_TIMELINE": "diagnostic",
    "BENOR_EVENT_FORM": "validation", "BENOR_LIVE_WAVES": "tuning", "BENOR_EVENT_STATS": "diagnostic",
    "BENOR_MFMA_PAIR": "validation", "BENOR_MFMA_DYNAMIC": "validation", "BENOR_MFMA_CHUNK": "tuning",
    "BENOR_MFMA_STRIP": "validation",
}

BASE_NODE_PORT = 3000          # src/config.ts:1 (kept for the HTTP-shaped helpers)
DEFAULT_K_MAX = 64             # round cap; the reference runs until /stop

# Symbols the C ABI exports (include/benor.h); checked by tests.
EXPORTED_SYMBOLS = (
    "bo_network_create", "bo_consensus_start", "bo_consensus_stop", "bo_node_stop",
    "bo_get_state", "bo_status", "bo_network_size", "bo_network_destroy", "bo_hist_len",
    "bo_plan_create", "bo_plan_launch", "bo_plan_run", "bo_plan_popc_words_per_node_round",
    "bo_plan_live_nodes", "bo_plan_destroy", "bo_run_trials", "bo_run_trial_states",
    "bo_popc_peak", "bo_last_error", "bo_abi_version", "bo_kernel_version", "bo_plan_kernel", "bo_kernel_for",
    "bo_mfma_peak", "bo_consensus_start_sched", "bo_plan_check",
    "bo_consensus_start_live", "bo_consensus_wait", "bo_live_stop_events", "bo_get_states", "bo_consensus_poll",
    "bo_tally_cdf", "bo_byz_cdf",
    "bo_lumped_check", "bo_lumped_run", "bo_lumped_trial", "bo_binom_half_cdf",
    "bo_rule_protocol_a", "bo_rule_protocol_b", "bo_plan_create_rule", "bo_run_trial_states_rule", "bo_plan_rule",
    "bo_lumped_check_rule", "bo_lumped_run_rule", "bo_lumped_trial_rule",
    "bo_plan_delivery_masks",
)


class Error(Exception):
    """The reference's `new Error(message)` (launchNodes.ts:11,13)."""


class AlreadyStartedError(RuntimeError):
    """libbenor error 8: a second start on one network (its inboxes persist, node.ts:29-30)."""


class NodeStateC(ctypes.Structure):
    _fields_ = [("killed", ctypes.c_int8), ("x", ctypes.c_int8), ("decided", ctypes.c_int8),
                ("pad", ctypes.c_int8), ("k", ctypes.c_int32)]


class TrialsCfgC(ctypes.Structure):
    _fields_ = [("N", ctypes.c_uint32), ("F", ctypes.c_uint32), ("k_max", ctypes.c_uint32),
                ("init_mode", ctypes.c_uint32), ("mode", ctypes.c_uint32), ("crash_cut", ctypes.c_uint32),
                ("seed", ctypes.c_uint64), ("faulty", ctypes.POINTER(ctypes.c_uint8)),
                ("init", ctypes.POINTER(ctypes.c_int8)), ("crash_at", ctypes.POINTER(ctypes.c_uint32)),
                ("crash_count", ctypes.c_uint32), ("crash_window", ctypes.c_uint32)]


class LumpedCfgC(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("N", "F", "f", "b", "byz_even", "rule", "strategy", "coin_common", "k_max",
                                               "init_mode", "init0", "init1", "initq", "reserved")] + \
               [("seed", ctypes.c_uint64)]


class LumpedStateC(ctypes.Structure):
    _fields_ = [("a", ctypes.c_uint32 * 2), ("dec", ctypes.c_uint8 * 2), ("pad", ctypes.c_uint8 * 2),
                ("rounds", ctypes.c_uint32)]


class Rule(ctypes.Structure):
    """bo_rule: a threshold rule on a receiver's counts (c0, c1), three words (include/benor.h).
    With v the value of the strictly larger count: propose v iff 2 c_v > propose_gt2; adopt v iff c_v > adopt_gt and
    decide iff also 2 c_v > decide_gt2, else the coin.  The library validates the words."""
    _fields_ = [("propose_gt2", ctypes.c_uint32), ("adopt_gt", ctypes.c_uint32), ("decide_gt2", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]

    @property
    def words(self) -> tuple:
        return (int(self.propose_gt2), int(self.adopt_gt), int(self.decide_gt2))

    def __eq__(self, other):
        return isinstance(other, Rule) and self.words == other.words and self.reserved == other.reserved

    def __hash__(self):
        return hash((self.words, int(self.reserved)))

    def __repr__(self):
        return "Rule(propose_gt2=%d, adopt_gt=%d, decide_gt2=%d)" % self.words


def _rule(thresholds) -> Rule:
    """thresholds=: a Rule, or its three words (propose_gt2, adopt_gt, decide_gt2)."""
    if isinstance(thresholds, Rule):
        return thresholds
    words = tuple(thresholds)
    if len(words) != 3:
        raise ValueError("thresholds is a benor.Rule or its three words (propose_gt2, adopt_gt, decide_gt2)")
    for name, v in zip(("propose_gt2", "adopt_gt", "decide_gt2"), words):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 0xFFFFFFFF:
            raise ValueError(f"{name} is an unsigned 32-bit word, got {v!r}")
    return Rule(*words, 0)


def rule_check(thresholds) -> Rule:
    """The library's validation of a rule's words, without a plan (bo_lumped_check_rule on a one-node
    configuration, whose own words are valid; host only).  Returns the Rule."""
    rule = _rule(thresholds)
    one = LumpedCfgC(N=1, F=0, strategy=BYZ_BALANCE, k_max=1)
    _check(lib().bo_lumped_check_rule(ctypes.byref(one), ctypes.byref(rule)))
    return rule


def rule_protocol_a(N: int, F: int) -> Rule:
    """Ben-Or's crash-tolerant Protocol A (N > 2F) as a threshold rule: (N, 0, 2F) (bo_rule_protocol_a; host only)."""
    r = Rule()
    _check(lib().bo_rule_protocol_a(N, F, ctypes.byref(r)))
    return r


def rule_protocol_b(N: int, F: int) -> Rule:
    """Protocol B, BO_MODE_BYZ_RULE_B's rule, as a threshold rule: (N + F, F, N + F) (bo_rule_protocol_b; host only)."""
    r = Rule()
    _check(lib().bo_rule_protocol_b(N, F, ctypes.byref(r)))
    return r


def _crash_array(N, crash_at):
    if crash_at is None:
        return None
    return (ctypes.c_uint32 * max(1, N))(*[NEVER if v is None else int(v) for v in crash_at])


_lib = None


def lib() -> ctypes.CDLL:
    """Load libbenor.so; raises if it was not built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libbenor.so not built at {LIB_PATH}: run __graft_entry__.build()")
    L = ctypes.CDLL(LIB_PATH)
    P = ctypes.POINTER
    # int8 initial values and uint8 faulty flags, passed as bytes
    L.bo_network_create.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32,
                                    ctypes.c_char_p, ctypes.c_uint32, P(ctypes.c_void_p)]
    L.bo_consensus_start.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]
    L.bo_consensus_start_sched.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, P(ctypes.c_uint32),
                                           ctypes.c_uint32]
    L.bo_consensus_start_live.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]
    L.bo_consensus_wait.argtypes = [ctypes.c_void_p]
    L.bo_live_stop_events.argtypes = [ctypes.c_void_p, P(ctypes.c_uint32), ctypes.c_uint32]
    L.bo_consensus_stop.argtypes = [ctypes.c_void_p]
    L.bo_node_stop.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    L.bo_get_state.argtypes = [ctypes.c_void_p, ctypes.c_uint32, P(NodeStateC)]
    L.bo_get_states.argtypes = [ctypes.c_void_p, P(NodeStateC), ctypes.c_uint32, P(ctypes.c_uint64)]
    L.bo_consensus_poll.argtypes = [ctypes.c_void_p, P(ctypes.c_int)]
    L.bo_status.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    L.bo_network_size.argtypes = [ctypes.c_void_p]
    L.bo_network_size.restype = ctypes.c_uint32
    L.bo_network_destroy.argtypes = [ctypes.c_void_p]
    L.bo_network_destroy.restype = None
    L.bo_hist_len.argtypes = [ctypes.c_uint32]
    L.bo_hist_len.restype = ctypes.c_uint32
    L.bo_plan_create.argtypes = [P(TrialsCfgC), P(ctypes.c_void_p)]
    L.bo_plan_launch.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                 ctypes.c_void_p]
    L.bo_plan_run.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, P(ctypes.c_uint64)]
    L.bo_plan_check.argtypes = [ctypes.c_void_p]
    L.bo_plan_popc_words_per_node_round.argtypes = [ctypes.c_void_p]
    L.bo_plan_popc_words_per_node_round.restype = ctypes.c_uint64
    L.bo_plan_live_nodes.argtypes = [ctypes.c_void_p]
    L.bo_plan_live_nodes.restype = ctypes.c_uint32
    L.bo_plan_destroy.argtypes = [ctypes.c_void_p]
    L.bo_plan_destroy.restype = None
    L.bo_run_trials.argtypes = [P(TrialsCfgC), ctypes.c_uint64, ctypes.c_uint64, P(ctypes.c_uint64)]
    L.bo_run_trial_states.argtypes = [P(TrialsCfgC), ctypes.c_uint64, P(NodeStateC), P(ctypes.c_uint32)]
    L.bo_popc_peak.argtypes = [ctypes.c_uint32]
    L.bo_popc_peak.restype = ctypes.c_double
    L.bo_mfma_peak.argtypes = [ctypes.c_uint32]
    L.bo_mfma_peak.restype = ctypes.c_double
    L.bo_plan_kernel.argtypes = [ctypes.c_void_p]
    L.bo_plan_kernel.restype = ctypes.c_int
    L.bo_kernel_for.argtypes = [P(TrialsCfgC), P(ctypes.c_int)]
    L.bo_tally_cdf.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, P(ctypes.c_uint32),
                               P(ctypes.c_uint64), ctypes.c_uint32, P(ctypes.c_uint32)]
    L.bo_byz_cdf.argtypes = [ctypes.c_uint32, ctypes.c_uint32, P(ctypes.c_uint64), ctypes.c_uint32, P(ctypes.c_uint32)]
    L.bo_lumped_check.argtypes = [P(LumpedCfgC)]
    L.bo_lumped_run.argtypes = [P(LumpedCfgC), ctypes.c_uint64, ctypes.c_uint64, P(ctypes.c_uint64)]
    L.bo_lumped_trial.argtypes = [P(LumpedCfgC), ctypes.c_uint64, P(LumpedStateC)]
    L.bo_binom_half_cdf.argtypes = [ctypes.c_uint32, P(ctypes.c_uint32), P(ctypes.c_uint64), ctypes.c_uint32,
                                    P(ctypes.c_uint32)]
    L.bo_rule_protocol_a.argtypes = [ctypes.c_uint32, ctypes.c_uint32, P(Rule)]
    L.bo_rule_protocol_b.argtypes = [ctypes.c_uint32, ctypes.c_uint32, P(Rule)]
    L.bo_plan_create_rule.argtypes = [P(TrialsCfgC), P(Rule), P(ctypes.c_void_p)]
    L.bo_run_trial_states_rule.argtypes = [P(TrialsCfgC), P(Rule), ctypes.c_uint64, P(NodeStateC), ctypes.c_uint32]
    L.bo_plan_rule.argtypes = [ctypes.c_void_p, P(Rule)]
    L.bo_plan_rule.restype = ctypes.c_int
    L.bo_lumped_check_rule.argtypes = [P(LumpedCfgC), P(Rule)]
    L.bo_lumped_run_rule.argtypes = [P(LumpedCfgC), P(Rule), ctypes.c_uint64, ctypes.c_uint64, P(ctypes.c_uint64)]
    L.bo_lumped_trial_rule.argtypes = [P(LumpedCfgC), P(Rule), ctypes.c_uint64, P(LumpedStateC)]
    L.bo_plan_delivery_masks.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                         P(ctypes.c_uint64)]
    L.bo_last_error.restype = ctypes.c_char_p
    L.bo_abi_version.restype = ctypes.c_int
    L.bo_kernel_version.restype = ctypes.c_char_p
    _lib = L
    return L


def last_error() -> str:
    return lib().bo_last_error().decode()


def _check(rc: int) -> None:
    if rc != BO_OK:
        msg = last_error()
        if rc in (BO_ERR_ARRAYS_DONT_MATCH, BO_ERR_FAULTY_COUNT):
            raise Error(msg)
        if rc == BO_ERR_ALREADY_STARTED:
            raise AlreadyStartedError(f"libbenor error {rc}: {msg}")
        raise RuntimeError(f"libbenor error {rc}: {msg}")


_VAL = {0: 0, 1: 1, "?": 2}
_UNVAL = {-1: None, 0: 0, 1: 1, 2: "?"}


def _state_dict(s: NodeStateC) -> dict:
    """NodeState (src/types.ts:1-8)."""
    return {"killed": bool(s.killed), "x": _UNVAL[s.x],
            "decided": None if s.decided < 0 else bool(s.decided),
            "k": None if s.k < 0 else int(s.k)}


_REC = struct.Struct("bbbbi")                     # bo_node_state


def _state_dicts(arr, n: int) -> list[dict]:
    """n NodeState dicts from a bo_node_state array: a network's states repeat
    (a few distinct records at any N), so each distinct 8-byte record is
    decoded once and copied."""
    raw = memoryview(arr).cast("B").cast("Q")[:n]
    tab = {}
    for v in set(raw):
        kl, x, dec, _, k = _REC.unpack(v.to_bytes(8, "little"))
        tab[v] = {"killed": kl != 0, "x": _UNVAL[x], "decided": None if dec < 0 else dec != 0,
                  "k": None if k < 0 else k}
    return [tab[v].copy() for v in raw]


class Node:
    """Stands in for one of the `http.Server` objects launchNetwork returns:
    the caller may close() it (benorconsensus.test.ts:14-29); the node's
    routes are getState() / status()."""
    __slots__ = ("_net", "node_id")

    def __init__(self, net: "Network", node_id: int):
        self._net, self.node_id = net, node_id

    @property
    def port(self) -> int:
        return BASE_NODE_PORT + self.node_id

    def close(self, cb=None):
        if cb is not None:
            cb()

    def closeAllConnections(self):
        return None

    def getState(self) -> dict:
        return self._net.get_state(self.node_id)

    def status(self) -> tuple[int, str]:
        return self._net.status(self.node_id)


class Network:
    """Owns one bo_network handle (host-side node state)."""

    def __init__(self, N: int, F: int, initialValues: Sequence, faultyList: Sequence[bool]):
        L = lib()
        n_init, n_f = len(initialValues), len(faultyList)
        init = bytes(_VAL.get(v, -2) & 0xFF for v in initialValues) or b"\0"     # int8 values
        fl = bytes(v is True for v in faultyList) or b"\0"
        h = ctypes.c_void_p()
        _check(L.bo_network_create(N, F, init, n_init, fl, n_f, ctypes.byref(h)))
        self._h = h
        self.N, self.F = N, F

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.bo_network_destroy(h)
            self._h = None

    def start(self, seed: int | None = None, k_max: int = DEFAULT_K_MAX, stop_after=None) -> None:
        """stop_after: GET /stop requests that land during the run -- {node: deliveries} or a
        length-N sequence (None = not stopped); deliveries = POST /message handled network-wide
        before the stop (bo_consensus_start_sched: the event-level kernels, N <= 4096)."""
        if seed is None:
            seed = secrets.randbits(64)        # the reference's coin is Math.random()
        if not stop_after:
            _check(lib().bo_consensus_start(self._h, seed, k_max))
            return
        if not isinstance(stop_after, dict) and len(stop_after) != self.N:
            raise ValueError(f"stop_after: a sequence must have N = {self.N} entries, got {len(stop_after)}")
        sched = [None] * self.N
        for i, v in (stop_after.items() if isinstance(stop_after, dict) else enumerate(stop_after)):
            if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < self.N:
                raise ValueError(f"stop_after: node {i!r} is not a node id in [0, {self.N})")
            if v is not None and (isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < NEVER):
                raise ValueError(f"stop_after[{i}]: {v!r} is not a delivery count (uint32 < 2^32 - 1) or None")
            sched[i] = v
        arr = _crash_array(self.N, sched)
        _check(lib().bo_consensus_start_sched(self._h, seed, k_max, arr, self.N))

    def start_live(self, seed: int | None = None, k_max: int = DEFAULT_K_MAX) -> None:
        """GET /start as the reference serves it (node.ts:167-188): launch the
        event-level kernel and return; stop() / stop_node() then land in the
        running kernel (bo_consensus_start_live) and wait() ends the run."""
        if seed is None:
            seed = secrets.randbits(64)
        _check(lib().bo_consensus_start_live(self._h, seed, k_max))

    def wait(self) -> None:
        """End of a live run: its final states replace the pre-run ones (no-op otherwise)."""
        _check(lib().bo_consensus_wait(self._h))

    def live_stop_events(self) -> list:
        """After wait(): per node, the delivery count at which the live run applied its
        /stop (None = none) -- as stop_after on a fresh network with the same seed it
        reproduces the run."""
        out = (ctypes.c_uint32 * max(1, self.N))()
        _check(lib().bo_live_stop_events(self._h, out, self.N))
        return [None if v == NEVER else int(v) for v in out[:self.N]]

    def stop(self) -> None:
        _check(lib().bo_consensus_stop(self._h))

    def stop_node(self, i: int) -> None:
        _check(lib().bo_node_stop(self._h, i))

    def poll(self) -> bool:
        """True while a live run is in flight; once it has ended its final states
        are merged (bo_consensus_poll, no blocking)."""
        r = ctypes.c_int(0)
        _check(lib().bo_consensus_poll(self._h, ctypes.byref(r)))
        return bool(r.value)

    def get_state(self, i: int) -> dict:
        """GET /getState (node.ts:197-199): at once, from a snapshot during a live run."""
        s = NodeStateC()
        _check(lib().bo_get_state(self._h, i, ctypes.byref(s)))
        return _state_dict(s)

    def get_states_at(self) -> tuple[list, int | None]:
        """Every node's state at once (bo_get_states) and, during a live run, the
        delivery count the snapshot reflects (None otherwise)."""
        st = (NodeStateC * max(1, self.N))()
        ev = ctypes.c_uint64(0)
        _check(lib().bo_get_states(self._h, st, self.N, ctypes.byref(ev)))
        return _state_dicts(st, self.N), (None if ev.value == 2 ** 64 - 1 else int(ev.value))

    def get_states(self) -> list[dict]:
        return self.get_states_at()[0]

    def status(self, i: int) -> tuple[int, str]:
        """GET /status (node.ts:33-39): (500, "faulty") or (200, "live")."""
        code = lib().bo_status(self._h, i)
        if code < 0:
            _check(-code)
        return (500, "faulty") if code == 500 else (200, "live")


_current: Network | None = None


def launchNetwork(N: int, F: int, initialValues: Sequence, faultyList: Sequence[bool]) -> list[Node]:
    """src/index.ts:4-14 -> launchNodes.ts:4-44.  Raises Error("Arrays don't
    match") / Error("faultyList doesnt have F faulties") like the reference."""
    global _current
    net = Network(N, F, initialValues, faultyList)
    _current = net
    return [Node(net, i) for i in range(N)]


def _net(N: int) -> Network:
    if _current is None or _current.N != N:
        raise RuntimeError(f"no launched network of size {N}")
    return _current


def startConsensus(N: int, seed: int | None = None, k_max: int = DEFAULT_K_MAX, stop_after=None,
                   strict: bool = False, live: bool | None = None, sync: bool = False) -> None:
    """src/nodes/consensus.ts:3-8: GET /start on every node.  As the
    reference's, it returns once the round loop (node.ts:43-163) is launched
    on the GPU, before consensus finishes (Network.start_live): stopConsensus /
    a node's stop land in the running kernel, getNodesState / getNodeState
    answer at once with the running network's states (a snapshot), and
    waitConsensus(N) waits for the end.  sync=True (or live=False) returns after the run (every live node
    decided, or k_max rounds; Network.start).  stop_after: a mid-run GET /stop
    schedule given up front (Network.start; returns after the run).  A second
    start on a network returns as the reference's does (every GET /start
    answers 200) but runs nothing: its inboxes persist (node.ts:29-30), so no
    fresh consensus can follow; strict=True raises instead."""
    if N == 0:
        return
    if live and stop_after:
        raise ValueError("stop_after and live are exclusive: a live run takes /stop as it comes")
    if live and sync:
        raise ValueError("live and sync are exclusive")
    if live is False:
        sync = True                      # an explicit non-live start is the run-to-completion form
    try:
        if not stop_after and not sync:
            _net(N).start_live(seed, k_max)
        else:
            _net(N).start(seed, k_max, stop_after)
    except AlreadyStartedError:
        if strict:
            raise


def stopConsensus(N: int) -> None:
    """src/nodes/consensus.ts:10-15: GET /stop on every node."""
    if N == 0:
        return
    _net(N).stop()


def getNodeState(nodeId: int) -> dict:
    """__test__/tests/utils.ts:4-12 (GET /getState, node.ts:197-199): answers at
    once -- during a live run, with the running network's state."""
    if _current is None:
        raise RuntimeError("no launched network")
    return _current.get_state(nodeId)


def getNodesState(N: int) -> list[dict]:
    """__test__/tests/utils.ts:14-20: every node's state at once (one snapshot of
    a running network, bo_get_states).  Callers poll it until reachedFinality, as
    the reference's tests do (benorconsensus.test.ts:153-160)."""
    return _net(N).get_states()


def waitConsensus(N: int) -> None:
    """The end of the network's live run (no-op otherwise): its final states."""
    if N == 0:
        return
    _net(N).wait()


def getStatus(nodeId: int) -> tuple[int, str]:
    if _current is None:
        raise RuntimeError("no launched network")
    return _current.status(nodeId)


def reachedFinality(states: Sequence[dict]) -> bool:
    """__test__/tests/utils.ts:22-24."""
    return all(s["decided"] is not False for s in states)


# ------------------------------------------------------------------ batches
def hist_len(k_max: int) -> int:
    return (k_max + 1) * 3 + 1


def _cut_word(crash_cut, crash_reach):
    """The configuration word that mode 6 reads as crash_cut and mode 7 as crash_reach."""
    if crash_reach is None:
        return crash_cut
    if crash_cut:
        raise ValueError("crash_cut and crash_reach name the same configuration word: give one")
    if not 0 <= crash_reach <= REACH_ALL:
        raise ValueError("crash_reach is a probability in units of 2**-32: 0 .. 2**32 - 1")
    return crash_reach


def reach_word(p: float) -> int:
    """crash_reach of a probability in [0, 1]: 1.0 is REACH_ALL, otherwise floor(p * 2**32)."""
    if not 0.0 <= p <= 1.0:
        raise ValueError("a reach probability lies in [0, 1]")
    return REACH_ALL if p >= 1.0 else int(p * 2.0 ** 32)


_SCHED_MODES = (BO_MODE_SCHED_TALLY, BO_MODE_SCHED_RULE_B)
_BYZ_MODES = (BO_MODE_BYZ_TALLY, BO_MODE_BYZ_RULE_B, BO_MODE_BYZ_COIN, BO_MODE_BYZ_RULE_B_COIN) + _SCHED_MODES


def _byz_words(mode, crash_cut, crash_count, byzantine, byz_one, byz_strategy):
    """Modes 8 to 13 read the crash_cut word as byz_one and the crash_count word as byz_strategy."""
    if byzantine is None and byz_one is None and byz_strategy is None:
        return crash_cut, crash_count
    if mode not in _BYZ_MODES:
        raise ValueError("byzantine, byz_one and byz_strategy need mode=BO_MODE_BYZ_TALLY or BO_MODE_BYZ_RULE_B "
                         "(or their shared-coin modes)")
    if crash_cut or crash_count:
        raise ValueError("byz_one / byz_strategy name the configuration words of crash_cut / crash_count: give one")
    byz_one = 0 if byz_one is None else byz_one
    if not 0 <= byz_one <= 0xFFFFFFFF:
        raise ValueError("byz_one is a probability in units of 2**-32: 0 .. 2**32 - 1")
    return byz_one, (BYZ_RANDOM if byz_strategy is None else byz_strategy)


def _coin_word(mode, crash_window, coin_common):
    """Modes 10 to 13 read the crash_window word as coin_common."""
    if coin_common is None:
        return crash_window
    if mode not in (BO_MODE_BYZ_COIN, BO_MODE_BYZ_RULE_B_COIN) + _SCHED_MODES:
        raise ValueError("coin_common needs mode=BO_MODE_BYZ_COIN or BO_MODE_BYZ_RULE_B_COIN")
    if crash_window:
        raise ValueError("coin_common names the configuration word of crash_window: give one")
    if not 0 <= coin_common <= 0xFFFFFFFF:
        raise ValueError("coin_common is a probability in units of 2**-32: 0 .. 2**32 - 1")
    return coin_common


def _faulty_array(N, faulty, byzantine, mode):
    """The faulty bytes: 1 for a faulty node, and in modes 8 to 13 2 for a Byzantine one (an int entry of
    `faulty` goes through as it is there, so that the library's validation can be reached)."""
    raw = mode in _BYZ_MODES
    fl = [v if raw and type(v) is int else (1 if v else 0) for v in faulty]
    if byzantine is not None:
        if len(byzantine) != len(fl):
            raise ValueError("byzantine holds one flag per node")
        for i, v in enumerate(byzantine):
            if v and fl[i]:
                raise ValueError(f"node {i} is both faulty and Byzantine")
            if v:
                fl[i] = 2
    return (ctypes.c_uint8 * max(1, N))(*fl)


def _trials_cfg(N, F, faulty=None, *, seed=0, k_max=DEFAULT_K_MAX, initial_values=None, mode=BO_MODE_LOCKSTEP,
                crash_at=None, crash_count=0, crash_window=0, crash_cut=0, crash_reach=None, byzantine=None,
                byz_one=None, byz_strategy=None, coin_common=None):
    """bo_trials_cfg for a shape, and the ctypes arrays it points into."""
    crash_window = _coin_word(mode, crash_window, coin_common)
    crash_cut = _cut_word(crash_cut, crash_reach)
    crash_cut, crash_count = _byz_words(mode, crash_cut, crash_count, byzantine, byz_one, byz_strategy)
    if faulty is None:                       # start.ts:7-18 placement: the first F nodes
        faulty = [i < F for i in range(N)]
    fl = _faulty_array(N, faulty, byzantine, mode)
    if initial_values is None:
        init = (ctypes.c_int8 * max(1, N))()
        init_mode = BO_INIT_RANDOM
    else:
        init = (ctypes.c_int8 * max(1, N))(*[_VAL[v] for v in initial_values])
        init_mode = BO_INIT_FIXED
    crash = _crash_array(N, crash_at)
    cfg = TrialsCfgC(N, F, k_max, init_mode, mode, crash_cut, seed,
                     ctypes.cast(fl, ctypes.POINTER(ctypes.c_uint8)),
                     ctypes.cast(init, ctypes.POINTER(ctypes.c_int8)),
                     ctypes.cast(crash, ctypes.POINTER(ctypes.c_uint32)) if crash else None,
                     crash_count, crash_window)
    return cfg, (fl, init, crash)


def kernel_for(N: int, F: int, faulty: Sequence[bool] | None = None, **kw) -> int:
    """The kernel family a TrialsPlan of this shape runs (bo_kernel_for; host only)."""
    cfg, _keep = _trials_cfg(N, F, faulty, **kw)
    k = ctypes.c_int()
    _check(lib().bo_kernel_for(ctypes.byref(cfg), ctypes.byref(k)))
    return k.value


class TrialsPlan:
    """Many independent trials of one (N, F, faulty) network shape on the
    current device (bo_plan_*)."""

    def __init__(self, N: int, F: int, faulty: Sequence[bool] | None = None, *, seed: int = 0,
                 k_max: int = DEFAULT_K_MAX, initial_values: Sequence | None = None,
                 mode: int = BO_MODE_LOCKSTEP, crash_at: Sequence | None = None, crash_count: int = 0,
                 crash_window: int = 0, crash_cut: int = 0, crash_reach: int | None = None,
                 byzantine: Sequence[bool] | None = None, byz_one: int | None = None,
                 byz_strategy: int | None = None, coin_common: int | None = None, thresholds=None):
        """thresholds: a benor.Rule (or its three words) that replaces Protocol B's rule on a plan of mode 9, 11 or
        13 (bo_plan_create_rule): rule_protocol_a(N, F) runs Ben-Or's Protocol A there."""
        self.N, self.F, self.k_max, self.seed = N, F, k_max, seed
        self.mode = mode
        self._cfg, self._keep = _trials_cfg(N, F, faulty, seed=seed, k_max=k_max, initial_values=initial_values,
                                            mode=mode, crash_at=crash_at, crash_count=crash_count,
                                            crash_window=crash_window, crash_cut=crash_cut, crash_reach=crash_reach,
                                            byzantine=byzantine, byz_one=byz_one, byz_strategy=byz_strategy,
                                            coin_common=coin_common)
        h = ctypes.c_void_p()
        if thresholds is None:
            _check(lib().bo_plan_create(ctypes.byref(self._cfg), ctypes.byref(h)))
        else:
            rule = _rule(thresholds)
            _check(lib().bo_plan_create_rule(ctypes.byref(self._cfg), ctypes.byref(rule), ctypes.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.bo_plan_destroy(h)
            self._h = None

    @property
    def live_nodes(self) -> int:
        return lib().bo_plan_live_nodes(self._h)

    @property
    def popc_words_per_node_round(self) -> int:
        return lib().bo_plan_popc_words_per_node_round(self._h)

    @property
    def kernel(self) -> int:
        """BO_KERNEL_* family of this plan's batch launches (bo_plan_kernel)."""
        return lib().bo_plan_kernel(self._h)

    @property
    def rule(self) -> Rule | None:
        """The threshold rule that replaces the plan's own (bo_plan_rule), or None."""
        r = Rule()
        rc = lib().bo_plan_rule(self._h, ctypes.byref(r))
        if rc < 0:
            _check(-rc)
        return r if rc else None

    @property
    def hist_len(self) -> int:
        return hist_len(self.k_max)

    def launch(self, trial_begin: int, trial_count: int, hist_dev_ptr: int, stream_ptr: int = 0) -> None:
        """Asynchronous; adds into the device histogram at hist_dev_ptr."""
        _check(lib().bo_plan_launch(self._h, trial_begin, trial_count, ctypes.c_void_p(hist_dev_ptr),
                                    ctypes.c_void_p(stream_ptr)))

    def check(self) -> None:
        """bo_plan_check: synchronise and raise when a launch of this plan broke a
        device-side invariant (its histogram is then incomplete)."""
        _check(lib().bo_plan_check(self._h))

    def run(self, trial_begin: int, trial_count: int):
        import numpy as np

        h = np.zeros(self.hist_len, dtype=np.uint64)
        _check(lib().bo_plan_run(self._h, trial_begin, trial_count,
                                 h.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return h

    def delivery_masks(self, trial: int, round: int, phase: int):
        """The delivered-sender masks the plan's random-delivery kernel draws in one phase of one trial
        (bo_plan_delivery_masks; tests and diagnosis): an [m, ceil(m / 64)] uint64 array, row c the mask of the
        receiver with compact live index c over compact sender indices."""
        import numpy as np

        m = self.live_nodes
        out = np.zeros((m, (m + 63) // 64), dtype=np.uint64)
        _check(lib().bo_plan_delivery_masks(self._h, trial, round, phase,
                                            out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out


def run_trial_states(N: int, F: int, faulty: Sequence[bool], *, seed: int = 0, trial: int = 0,
                     k_max: int = DEFAULT_K_MAX, initial_values: Sequence | None = None,
                     mode: int = BO_MODE_LOCKSTEP, crash_at: Sequence | None = None, crash_count: int = 0,
                     crash_window: int = 0, crash_cut: int = 0, crash_reach: int | None = None,
                     byzantine: Sequence[bool] | None = None, byz_one: int | None = None,
                     byz_strategy: int | None = None, coin_common: int | None = None, thresholds=None):
    """Per-node final states of one trial: (rounds, [NodeState dict] * N).  thresholds: as TrialsPlan's
    (bo_run_trial_states_rule; the rounds are then read off the states: k - 1 of the honest nodes if all of them
    have decided, else 0)."""
    crash_window = _coin_word(mode, crash_window, coin_common)
    crash_cut = _cut_word(crash_cut, crash_reach)
    crash_cut, crash_count = _byz_words(mode, crash_cut, crash_count, byzantine, byz_one, byz_strategy)
    fl = _faulty_array(N, faulty, byzantine, mode)
    if initial_values is None:
        init = (ctypes.c_int8 * max(1, N))()
        init_mode = BO_INIT_RANDOM
    else:
        init = (ctypes.c_int8 * max(1, N))(*[_VAL[v] for v in initial_values])
        init_mode = BO_INIT_FIXED
    ca = _crash_array(N, crash_at)
    cfg = TrialsCfgC(N, F, k_max, init_mode, mode, crash_cut, seed,
                     ctypes.cast(fl, ctypes.POINTER(ctypes.c_uint8)),
                     ctypes.cast(init, ctypes.POINTER(ctypes.c_int8)),
                     ctypes.cast(ca, ctypes.POINTER(ctypes.c_uint32)) if ca else None, crash_count, crash_window)
    st = (NodeStateC * max(1, N))()
    if thresholds is not None:
        rule = _rule(thresholds)
        _check(lib().bo_run_trial_states_rule(ctypes.byref(cfg), ctypes.byref(rule), trial, st, N))
        states = [_state_dict(st[i]) for i in range(N)]
        ran = [s for s in states if s["k"] is not None]          # the honest nodes
        return (ran[0]["k"] - 1 if ran and all(s["decided"] for s in ran) else 0), states
    rounds = ctypes.c_uint32(0)
    _check(lib().bo_run_trial_states(ctypes.byref(cfg), trial, st, ctypes.byref(rounds)))
    return int(rounds.value), [_state_dict(st[i]) for i in range(N)]


def tally_cdf(m: int, q: int, K: int) -> tuple[int, list[int]]:
    """Row K of the BO_MODE_RANDOM_TALLY table for (m, q) (bo_tally_cdf; host only):
    (lo, thresholds).  With K of m senders holding a 1, a 64-bit draw u gives the
    receiver's count of 1s among its q arrivals as lo + #{j : thresholds[j] <= u}."""
    cap = max(1, min(K, q))
    thr = (ctypes.c_uint64 * cap)()
    lo, n = ctypes.c_uint32(), ctypes.c_uint32()
    _check(lib().bo_tally_cdf(m, q, K, ctypes.byref(lo), thr, cap, ctypes.byref(n)))
    return int(lo.value), [int(v) for v in thr[:n.value]]


def byz_cdf(b: int, byz_one: int) -> list[int]:
    """The b thresholds of Binomial(b, byz_one / 2**32) that BO_MODE_BYZ_TALLY searches (bo_byz_cdf;
    host only): a 64-bit draw u gives the number of Byzantine messages that carry 1 as
    #{j : thresholds[j] <= u}."""
    thr = (ctypes.c_uint64 * max(1, b))()
    n = ctypes.c_uint32()
    _check(lib().bo_byz_cdf(b, byz_one, thr, b, ctypes.byref(n)))
    return [int(v) for v in thr[:n.value]]


# ------------------------------------------------------------------ the lumped (class-level) chain
LUMPED_MAX_N = 1 << 24


def byz_even(faulty: Sequence, byzantine: Sequence | None = None) -> int:
    """The Byzantine nodes at an even compact index, as bo_lumped_cfg.byz_even counts them: compact indices number
    the live nodes in ascending node id.  `faulty` marks the crashed nodes (an int entry 2 a Byzantine one, as modes
    8 to 13 read it), `byzantine` the Byzantine ones: a mode-12 configuration maps to its lumped one through
    f = the crashed, b = the Byzantine, and this."""
    n, c = 0, 0
    for i, v in enumerate(faulty):
        byz = (type(v) is int and v == 2) or (byzantine is not None and bool(byzantine[i]))
        if v and not byz:
            continue                                # crashed: no compact index
        if byz and c % 2 == 0:
            n += 1
        c += 1
    return n


class LumpedPlan:
    """Many independent trials of the adversarial scheduler's class-level chain (bo_lumped_*):
    modes 12 and 13 with nodes replaced by the two receiver parities, N up to 2**24.  rule 0 is mode 12's, 1 mode 13's;
    byz_strategy BYZ_BALANCE or BYZ_SPLIT; initial_values None (random) or the counts (init0, init1, initq) of the
    honest nodes that start at 0, 1 and "?".  Validation needs no device."""

    def __init__(self, N: int, F: int, *, f: int = 0, b: int = 0, byz_even: int = 0, rule: int = 0,
                 byz_strategy: int = BYZ_BALANCE, coin_common: int = 0, seed: int = 0, k_max: int = DEFAULT_K_MAX,
                 initial_values: Sequence[int] | None = None, thresholds=None):
        """thresholds: a benor.Rule (or its three words) in the place of `rule`, which is then not read
        (bo_lumped_*_rule)."""
        words = dict(N=N, F=F, f=f, b=b, byz_even=byz_even, rule=rule, strategy=byz_strategy, coin_common=coin_common,
                     k_max=k_max)
        init = (0, 0, 0) if initial_values is None else tuple(initial_values)
        if len(init) != 3:
            raise ValueError("initial_values holds three counts: the honest nodes that start at 0, 1 and '?'")
        words.update(init0=init[0], init1=init[1], initq=init[2])
        for name, v in words.items():
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 0xFFFFFFFF:
                raise ValueError(f"{name} is an unsigned 32-bit word, got {v!r}")
        if not 0 <= seed < 1 << 64:
            raise ValueError("seed is an unsigned 64-bit word")
        self.N, self.F, self.k_max, self.seed = N, F, k_max, seed
        self._cfg = LumpedCfgC(init_mode=BO_INIT_RANDOM if initial_values is None else BO_INIT_FIXED, reserved=0,
                               seed=seed, **words)
        self.rule = None if thresholds is None else _rule(thresholds)
        if self.rule is None:
            _check(lib().bo_lumped_check(ctypes.byref(self._cfg)))
        else:
            _check(lib().bo_lumped_check_rule(ctypes.byref(self._cfg), ctypes.byref(self.rule)))

    @property
    def hist_len(self) -> int:
        return hist_len(self.k_max)

    def run(self, trial_begin: int, trial_count: int):
        import numpy as np

        h = np.zeros(self.hist_len, dtype=np.uint64)
        hp = h.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        if self.rule is None:
            _check(lib().bo_lumped_run(ctypes.byref(self._cfg), trial_begin, trial_count, hp))
        else:
            _check(lib().bo_lumped_run_rule(ctypes.byref(self._cfg), ctypes.byref(self.rule), trial_begin, trial_count, hp))
        return h

    def trial(self, trial: int) -> dict:
        """One trial's final state: {"a": (a_0, a_1), "dec": (dec_0, dec_1), "rounds": R or 0}."""
        st = LumpedStateC()
        if self.rule is None:
            _check(lib().bo_lumped_trial(ctypes.byref(self._cfg), trial, ctypes.byref(st)))
        else:
            _check(lib().bo_lumped_trial_rule(ctypes.byref(self._cfg), ctypes.byref(self.rule), trial, ctypes.byref(st)))
        return {"a": (int(st.a[0]), int(st.a[1])), "dec": (bool(st.dec[0]), bool(st.dec[1])), "rounds": int(st.rounds)}


def lumped_trials(N: int, F: int, trial_begin: int, trial_count: int, **kw):
    """The histogram of trials [trial_begin, trial_begin + trial_count) of a LumpedPlan(N, F, **kw)."""
    return LumpedPlan(N, F, **kw).run(trial_begin, trial_count)


def lumped_trial(N: int, F: int, trial: int, **kw) -> dict:
    """LumpedPlan(N, F, **kw).trial(trial)."""
    return LumpedPlan(N, F, **kw).trial(trial)


def binom_half_cdf(k: int) -> tuple[int, list[int]]:
    """The thresholds of Binomial(2**k, 1/2), 7 <= k <= 24, that the lumped chain searches (bo_binom_half_cdf; host
    only): (lo, thresholds).  A 64-bit draw u gives the count lo + #{j : thresholds[j] <= u}."""
    cap = 1 << 16                                   # k = 24 holds about 37 000: 9.1 standard deviations either side
    thr = (ctypes.c_uint64 * cap)()
    lo, n = ctypes.c_uint32(), ctypes.c_uint32()
    _check(lib().bo_binom_half_cdf(k, ctypes.byref(lo), thr, cap, ctypes.byref(n)))
    return int(lo.value), list(thr[:n.value])


def kernel_version() -> str:
    """Digest of the kernel sources libbenor.so was built from."""
    return lib().bo_kernel_version().decode()


def popc_peak(iters: int = 20) -> float:
    return float(lib().bo_popc_peak(iters))


def mfma_peak(iters: int = 10) -> float:
    """Measured e2m1 32x32x64 MFMA multiply-adds per second (bo_mfma_peak)."""
    return float(lib().bo_mfma_peak(iters))
