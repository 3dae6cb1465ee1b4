// Type declarations for the JavaScript mirror (index.js).  The reference's
// types are src/types.ts:1-8; the signatures mirror src/index.ts:4-14 and
// src/nodes/consensus.ts:3-15.

export type Value = 0 | 1 | "?";

export type NodeState = {
  killed: boolean;
  x: Value | null;
  decided: boolean | null;
  k: number | null;
};

export declare const BASE_NODE_PORT: number;
export declare const DEFAULT_K_MAX: number;

/** Stand-in for the reference's http.Server per node. */
export interface NodeServer {
  readonly nodeId: number;
  readonly port: number;
  close(cb?: () => void): NodeServer;
  closeAllConnections(): void;
}

/** Rejects with Error("Arrays don't match") / Error("faultyList doesnt have F faulties"). */
export declare function launchNetwork(
  N: number,
  F: number,
  initialValues: Value[],
  faultyList: boolean[]
): Promise<NodeServer[]>;

export interface StartOptions {
  /** Philox key for the per-node coins (default: random, like Math.random()). */
  seed?: bigint | number;
  /** Round cap (default 64). */
  kMax?: number;
  /** GET /stop requests landing mid-run (node.ts:191-194): per node, the number of
   * POST /message deliveries (network-wide, seeded order) after which it is stopped;
   * an array of N entries (null = never) or {nodeId: deliveries}.  Event-level kernels,
   * N <= 4096.  Resolves at the end of the run. */
  stopAfter?: (number | null)[] | { [nodeId: number]: number };
  /** Reject a second start on one network (libbenor error 8) instead of resolving as a no-op. */
  strict?: boolean;
  /** Resolve once the run has finished (every live node decided, or kMax rounds); a stop
   * sent meanwhile is ordered after the run.  Default: resolve once the kernel is launched,
   * as the reference's startConsensus does (consensus.ts:3-8). */
  sync?: boolean;
  /** The default (launch, resolve, let stops land in the running kernel); exclusive with
   * stopAfter and sync. */
  live?: boolean;
}

/** Resolves once the round loop is launched (before consensus finishes, like GET /start);
 * stopNode / stopConsensus then land in the running kernel, getNodesState / getNodeState answer
 * at once with a snapshot of the running network (GET /getState, node.ts:197-199), and
 * waitConsensus waits for the end of the run.  {sync: true}: resolves after the run. */
export declare function startConsensus(N: number, options?: StartOptions): Promise<void>;
export declare function stopConsensus(N: number): Promise<void>;
export declare function stopNode(nodeId: number): Promise<void>;
export declare function getNodeState(nodeId: number): Promise<NodeState>;
export declare function getNodesState(N: number): Promise<NodeState[]>;
/** getNodesState with the delivery count a live run's snapshot reflects (null when no run is in
 * flight): the states are oracle (iii) truncated before that many POST /message deliveries. */
export declare function getNodesStateAt(N: number): Promise<{ states: NodeState[]; events: number | null }>;
export declare function getNodeStatus(nodeId: number): Promise<{ status: 200 | 500; body: "live" | "faulty" }>;
export declare function reachedFinality(states: NodeState[]): boolean;
export declare function delay(ms: number): Promise<void>;
/** End of a run started by the default startConsensus; resolves at once otherwise. */
export declare function waitConsensus(N: number): Promise<void>;
/** After a run started by the default startConsensus: per node, the delivery count at which its /stop landed (null = none);
 * as stopAfter on a fresh network with the same seed it reproduces the run. */
export declare function liveStopEvents(N: number): Promise<(number | null)[]>;

export interface TrialsConfig {
  N: number;
  F: number;
  /** default: the first F nodes are crash-faulty */
  faultyList?: boolean[];
  /** default: iid Bernoulli(1/2) per live node */
  initialValues?: Value[];
  seed?: bigint | number;
  kMax?: number;
  trialBegin?: bigint | number;
  trialCount?: bigint | number;
  /** 0 lockstep (default), 1 random delivery (f <= F), 2 event level (N <= 4096),
   *  3 random delivery at the level of counts (MODE_RANDOM_TALLY: f <= F, N - F odd, no "?" initial value),
   *  4 the same for any quorum and with "?" initial values (MODE_RANDOM_TALLY3: f <= F; three vote classes,
   *    ties and coins; equal to mode 3 bit for bit wherever mode 3 is defined),
   *  5 mode 4 with crashes during the run (MODE_CRASH_TALLY: clean crashes at step boundaries, step 2(r-1) =
   *    the R-phase of round r, step 2(r-1)+1 = its P-phase; f + scheduled crashes <= F; an empty schedule is
   *    mode 4 bit for bit),
   *  6 mode 5 with partial broadcasts (MODE_CRASH_PARTIAL: a crasher's last message reaches the initially-live
   *    nodes whose index, in ascending node id, is below its cut; crashCut = 0 is mode 5 bit for bit),
   *  7 mode 6 with an arbitrary subset for the prefix (MODE_CRASH_SUBSET: a crasher's last message reaches each
   *    receiver independently with probability crashReach / 2^32; crashReach = 0 is mode 5 and REACH_ALL is
   *    mode 6 with a full cut, bit for bit),
   *  8 mode 4 with Byzantine senders (MODE_BYZ_TALLY: the nodes of byzantineList send at every step and lie,
   *    they never receive; crashed + Byzantine <= F; without a Byzantine node it is mode 4 bit for bit),
   *  9 mode 8 under Ben-Or's Byzantine-tolerant rule (MODE_BYZ_RULE_B: Protocol B with F as its t -- propose v
   *    iff 2 c_v > N + F, adopt the strict majority v iff c_v > F and decide iff 2 c_v > N + F, else the coin;
   *    byzantineList, byzOne and byzStrategy as in mode 8; without a Byzantine node it still runs this rule),
   *  10, 11 modes 8 and 9 with a shared coin (MODE_BYZ_COIN, MODE_BYZ_RULE_B_COIN: in a common round every honest
   *    node that takes a coin gets the same bit; coinCommon = 0 is mode 8 or 9 bit for bit),
   *  12, 13 modes 10 and 11 under an adversarial scheduler (MODE_SCHED_TALLY, MODE_SCHED_RULE_B: the adversary, not
   *    a draw, picks the N - F messages each honest receiver hears at every step and what the Byzantine senders
   *    among them say; byzStrategy BYZ_BALANCE or BYZ_SPLIT, byzOne is not read, no Byzantine node is needed) */
  mode?: 0 | 1 | 2 | 3 | 4 | 5 | 6 | 7 | 8 | 9 | 10 | 11 | 12 | 13;
  /** event mode: deliveries after which node i is stopped (null = never);
   *  MODE_CRASH_TALLY, MODE_CRASH_PARTIAL, MODE_CRASH_SUBSET: the step at which node i crashes (null = never) */
  crashAt?: (number | null)[];
  /** event mode, random schedule: stop crashCount live nodes at uniform delivery counts in [0, crashWindow);
   *  MODE_CRASH_TALLY: crashCount initially-live nodes crash at uniform steps in [0, crashWindow), per trial */
  crashCount?: number;
  crashWindow?: number;
  /** MODE_CRASH_PARTIAL: every crasher's cut, 0 .. the initially-live count, or CUT_RANDOM (uniform per trial
   *  and crasher); default 0 */
  crashCut?: number;
  /** MODE_CRASH_SUBSET: the probability, in units of 2^-32, that a crasher's last message reaches a receiver
   *  (0 .. REACH_ALL = 2^32 - 1: certainly); it fills the word that crashCut fills, so give one of the two */
  crashReach?: number;
  /** MODE_BYZ_TALLY, MODE_BYZ_RULE_B: true marks node i Byzantine (a node of faultyList is crashed and may not be in both) */
  byzantineList?: boolean[];
  /** MODE_BYZ_TALLY, MODE_BYZ_RULE_B: the probability, in units of 2^-32, that a Byzantine message carries 1, independently per
   *  trial, sender, receiver, round and phase (0 .. 2^32 - 1: certainly); it fills the word that crashCut fills */
  byzOne?: number;
  /** MODE_BYZ_TALLY, MODE_BYZ_RULE_B: BYZ_RANDOM (default; each message by byzOne), BYZ_OPPOSE (every message carries the value
   *  fewer honest senders hold at the step, byzOne's step on a tie), BYZ_BALANCE (the Byzantine messages in a
   *  receiver's inbox make its two tallies as equal as they can) or BYZ_SPLIT (they say 1 to a receiver of odd
   *  compact index, 0 to one of even index); the last two do not read byzOne.  It fills the word that crashCount
   *  fills */
  byzStrategy?: 0 | 1 | 3 | 4;
  /** MODE_BYZ_COIN, MODE_BYZ_RULE_B_COIN, MODE_SCHED_TALLY, MODE_SCHED_RULE_B: the probability, in units of 2^-32, that a round's coin is common to all
   *  honest nodes (0 .. COIN_ALL = 2^32 - 1: certainly), per trial and round; it fills the word that crashWindow fills */
  coinCommon?: number;
}

/** TrialsConfig.mode values (include/benor.h BO_MODE_*). */
export declare const MODE_LOCKSTEP: 0;
export declare const MODE_RANDOM_DELIVERY: 1;
export declare const MODE_EVENT: 2;
export declare const MODE_RANDOM_TALLY: 3;
export declare const MODE_RANDOM_TALLY3: 4;
export declare const MODE_CRASH_TALLY: 5;
export declare const MODE_CRASH_PARTIAL: 6;
/** TrialsConfig.crashCut: a cut per trial and crasher (include/benor.h BO_CUT_RANDOM). */
export declare const CUT_RANDOM: 4294967295;
export declare const MODE_CRASH_SUBSET: 7;
/** TrialsConfig.crashReach: every crasher reaches every receiver (include/benor.h, crash_reach = UINT32_MAX). */
export declare const REACH_ALL: 4294967295;
export declare const MODE_BYZ_TALLY: 8;
export declare const MODE_BYZ_RULE_B: 9;
export declare const MODE_BYZ_COIN: 10;
export declare const MODE_BYZ_RULE_B_COIN: 11;
export declare const MODE_SCHED_TALLY: 12;
export declare const MODE_SCHED_RULE_B: 13;
export declare const COIN_ALL: 4294967295;
/** TrialsConfig.byzStrategy (include/benor.h BO_BYZ_RANDOM, BO_BYZ_OPPOSE, BO_BYZ_BALANCE, BO_BYZ_SPLIT). */
export declare const BYZ_RANDOM: 0;
export declare const BYZ_OPPOSE: 1;
export declare const BYZ_BALANCE: 3;
export declare const BYZ_SPLIT: 4;

/** Outcome histogram, (kMax + 1) * 3 + 1 bins (include/benor.h). */
export declare function runTrials(cfg: TrialsConfig): Promise<BigUint64Array>;
