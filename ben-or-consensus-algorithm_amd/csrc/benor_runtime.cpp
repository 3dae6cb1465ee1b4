// benor_runtime.cpp -- C ABI (include/benor.h) over the gfx950 kernels.
//
// Host-side mirror of the reference's network layer:
//   launchNetwork / launchNodes   src/index.ts:4-14, src/nodes/launchNodes.ts:4-44
//   startConsensus / stopConsensus src/nodes/consensus.ts:3-15
//   GET /status, /start, /stop, /getState   src/nodes/node.ts:33-39, :167-199
// The POST /message round loop (node.ts:43-163) runs on the device
// (benor_kernels.hip).  There is no CPU fallback: without a gfx950 device
// every compute entry point returns BO_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <algorithm>
#include <utility>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <thread>
#include <chrono>
#include <cmath>
#include <vector>

#include "benor.h"
#include "benor_internal.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

int hip_fail(hipError_t e, const char *what) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return BO_ERR_HIP;
}

#define HIP_TRY(expr)                                  \
  do {                                                 \
    hipError_t e_ = (expr);                            \
    if (e_ != hipSuccess) return hip_fail(e_, #expr);  \
  } while (0)

// The product runs only on a gfx950 device.
int check_device(int *dev_out) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(BO_ERR_NO_DEVICE, "no HIP device visible (libbenor has no CPU fallback)");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(BO_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", libbenor targets gfx950");
  if (dev_out) *dev_out = dev;
  return BO_OK;
}

__global__ void add_bin_kernel(unsigned long long *hist, uint32_t bin, unsigned long long n) {
  if (threadIdx.x == 0 && blockIdx.x == 0) hist[bin] += n;
}

}  // namespace

namespace benor {
// Every environment knob the library reads.  Production needs none: each
// forces a choice the planner makes by itself (DESIGN.md §6 "knobs").
//   validation: run another product kernel or form on the same trials, so
//     tests can check each against the others and the oracle;
//   tuning: grid shape only (every test checks that the histogram does not
//     depend on it);
//   test: provoke an error path;  diagnostic: instrumented launches.
struct KnobSpec {
  const char *name, *kind;
};
constexpr KnobSpec kKnobs[] = {
    {"BENOR_NO_MFMA", "validation"},            // "1": popcount kernels instead of the matrix-core ones
    {"BENOR_NO_MFMA_BIG", "validation"},        // "1": popcount kernels for m > 1024
    {"BENOR_MFMA_PAIR", "validation"},          // "0": KIND 0 matrix-core kernel, one receiver tile per accumulator
    {"BENOR_MFMA_DYNAMIC", "validation"},       // "0" / "1": KIND 0 matrix-core kernel, static stride / claimed chunks
    {"BENOR_MFMA_STRIP", "validation"},         // "0" / "1": its last receiver tile of <= 16 live rows in the 32-row shape / as a 16-row strip from W = 5
    {"BENOR_MFMA_CHUNK", "tuning"},            // its dynamic form: groups per claim (1..64)
    {"BENOR_BIG_FORM", "validation"},           // "wave" / "coop": big-network matrix-core form
    {"BENOR_COOP_BW", "validation"},            // 4 / 8: waves per cooperative workgroup
    {"BENOR_SMALL_MIN_TRIALS", "validation"},   // packed matrix-core kernel from this launch size
    {"BENOR_BLOCKS_PER_CU", "tuning"},          // workgroups per CU (grid)
    {"BENOR_EVENT_LANES_PER_CU", "tuning"},     // event level, N <= 256: lanes per CU
    {"BENOR_EVENT_FORM", "validation"},         // "wg": batch event plans on the workgroup-batched kernel
    {"BENOR_LIVE_WAVES", "tuning"},             // 1 / 3 / 7 / 15: event waves of the workgroup-batched kernel
    {"BENOR_EVENT_STATS", "diagnostic"},        // workgroup-batched kernel: batch counters and cycle split to a file
    {"BENOR_TEST_DEFER_SEG_CAP", "test"},       // deferral segment capacity below the sizing rule
    {"BENOR_TIMELINE", "diagnostic"},           // packed and KIND 0 matrix-core kernels: per-wave stamps to a file
};

const char *knob(const char *name) {
  for (const KnobSpec &k : kKnobs)
    if (std::strcmp(k.name, name) == 0) return std::getenv(name);
  std::fprintf(stderr, "libbenor: knob %s is not registered in kKnobs\n", name);
  std::abort();
}

uint32_t knob_u32(const char *name, uint32_t dflt) {
  const char *v = knob(name);
  return v && *v ? (uint32_t)std::strtoul(v, nullptr, 10) : dflt;
}

bool knob_is(const char *name, const char *value) {
  const char *v = knob(name);
  return v && std::strcmp(v, value) == 0;
}
}  // namespace benor

// One simulated network.  `mu` guards the node states: bo_consensus_start may
// run on a worker thread (the N-API addon's napi_async_work) while the caller's
// thread serves /stop, /getState and /status.  The kernel runs without the
// lock; its results are merged under it.
struct bo_live;
struct bo_network {
  uint32_t N = 0, F = 0;
  std::vector<bo_node_state> st;
  std::vector<uint8_t> faulty;
  bool started = false;     // GET /start was served (node.ts:167-188); inboxes persist after it
  bool in_flight = false;   // a start's kernel is running
  std::shared_ptr<bo_live> live;   // a live run (bo_consensus_start_live) not yet finalized
  int live_rc = 0;          // the result of the last live run finalized
  std::vector<uint32_t> stop_events;   // its /stop delivery counts, after the run
  mutable std::mutex mu;
  std::mutex wait_mu;       // serialises the end of a live run (live_finalize)
  std::mutex snap_mu;       // one GET /getState snapshot request in flight at a time
};

struct bo_plan {
  benor::KParams kp{};
  bo_trials_cfg cfg{};
  std::vector<uint32_t> live_ids;
  uint32_t *d_live = nullptr;
  uint4 *d_init = nullptr;
  int8_t *d_init_x = nullptr;      // event mode
  uint32_t *d_crash = nullptr;     // event mode
  uint32_t *d_scratch = nullptr;   // event mode
  uint32_t *d_defer = nullptr;     // matrix-core KIND > 0: deferred-trial list, its length, per-wave segments
  uint64_t defer_words = 0;
  uint32_t *d_flag = nullptr;      // KParams::overflow (bo_plan_check)
  uint32_t *d_claim = nullptr;     // KParams::mfma_claim: the claim words of the matrix-core kernel's dynamic form
  uint64_t *d_stops = nullptr;     // event level, N > 256: sorted /stop schedule
  unsigned char *d_tally = nullptr;   // RANDOM_TALLY: u32 row offsets [m + 2] (padded to 8 bytes), u64 thresholds;
                                      // CRASH_TALLY: directory, row offsets, explicit schedule list, thresholds
  int device = 0;
  bo_plan() = default;
  bo_plan(const bo_plan &) = delete;
  bo_plan &operator=(const bo_plan &) = delete;
  // (run_states_lockstep's plan on the stack views a scratch buffer: its d_* are null, and a state launch never
  // defers, so d_defer stays null too)
  ~bo_plan() {
    for (void *d : {(void *)d_live, (void *)d_init, (void *)d_init_x, (void *)d_crash, (void *)d_scratch, (void *)d_defer,
                    (void *)d_flag, (void *)d_claim, (void *)d_stops, (void *)d_tally})
      if (d) (void)hipFree(d);
  }
};

namespace {
// A device buffer of `count` T, freed at the end of its scope.
template <typename T>
struct DeviceBuf {
  T *d = nullptr;
  DeviceBuf() = default;
  DeviceBuf(const DeviceBuf &) = delete;
  DeviceBuf &operator=(const DeviceBuf &) = delete;
  ~DeviceBuf() { if (d) (void)hipFree(d); }
  hipError_t alloc(size_t count) { return hipMalloc(&d, sizeof(T) * count); }
};

// The peak probes' clock: one warm-up launch, then `iters` launches between two events on the null stream.
template <typename Launch>
float timed_launches_ms(uint32_t iters, Launch launch) {
  hipEvent_t a, b;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  launch();
  (void)hipEventRecord(a, nullptr);
  for (uint32_t i = 0; i < iters; ++i) launch();
  (void)hipEventRecord(b, nullptr);
  (void)hipEventSynchronize(b);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, a, b);
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return ms;
}

// The resources of one single-trial event-level run, kept for the next one
// (r05: the default startConsensus is a live run, and a network of the
// reference's size spent 0.8 ms of its 0.83 ms creating a stream, pinning a
// mailbox and allocating and freeing ten device buffers).  A slot is one
// device's stream, a host-mapped mailbox for BO_MAX_N nodes (GET /stop
// requests, their landing points, GET /getState snapshots) and one device
// buffer that grows to the largest run it served.  Slots are handed out under
// a lock and returned when their run ends; a buffer above kSlotKeepBytes is
// freed on return (a process that once ran a large network does not keep its
// message pool), and a slot whose run failed is destroyed, not reused.
struct LiveSlot {
  int device = -1;
  hipStream_t s = nullptr;
  uint32_t *box = nullptr;             // host-mapped mailbox (benor::kLiveReq .. kLiveBoxWords layout)
  uint32_t *dbox = nullptr;            // its device address
  unsigned char *d = nullptr;          // flag | states | hist | rounds | live ids | init x | stops | pool
  size_t bytes = 0;
  // pinned host copy of the buffer's head: the upload reads it, and the
  // result head (flag | states | hist | rounds) is copied back into it right
  // behind the kernel, so the end of a run is one stream synchronisation
  unsigned char *hp = nullptr;
  size_t hp_bytes = 0;
};
constexpr size_t kSlotKeepBytes = 64u << 20;
std::mutex g_slots_mu;
std::vector<LiveSlot *> g_free_slots;

// Where the run's results sit in the slot's buffer.
struct WgRun {
  size_t o_st = 0, o_r = 0;            // states [N], round word (the head read back ends after it)
  size_t o_stats = 0;                  // BENOR_EVENT_STATS counters (24 u64, after the round word)
  uint32_t N = 0, F = 0;
};
}  // namespace

// A live run (bo_consensus_start_live): the workgroup-batched event kernel
// (benor_event_live.hip) runs on its slot's stream while the caller serves
// /stop, /getState and /status; GET /stop requests and /getState snapshot
// requests reach the running kernel through the slot's mailbox.  Shared by the
// network and by every caller that reads its mailbox (snapshots), so the slot
// goes back to the pool only when the last of them is done.
struct bo_live {
  LiveSlot *slot = nullptr;
  WgRun run;
  std::vector<uint32_t> active;        // the nodes that run
  bool failed = false;                 // the run's stream reported an error: the slot is not reused
  // the last /getState snapshot (under bo_network::snap_mu): the kernel's
  // words of the active nodes, its delivery count and when it was served
  std::vector<uint32_t> snap_words;
  uint64_t snap_e = 0;
  std::chrono::steady_clock::time_point snap_t{};
  bool snap_ok = false;
  ~bo_live();
};

namespace {
// Post GET /stop requests to a live run (caller holds net->mu): the nodes'
// request bits (one OR per 32-node word), then the sequence word.  The
// kernel's control wave applies the bits it reads in the poll after the one
// that saw the new sequence, so one call's requests land together.
void live_post(bo_live *lr, const uint32_t *ids, uint32_t n) {
  uint32_t *box = lr->slot->box;
  uint32_t words[BO_MAX_N / 32] = {};
  for (uint32_t j = 0; j < n; ++j) words[ids[j] >> 5] |= 1u << (ids[j] & 31u);
  for (uint32_t w = 0; w < BO_MAX_N / 32; ++w)
    if (words[w]) __atomic_fetch_or(&box[benor::kLiveReq + w], words[w], __ATOMIC_RELAXED);
  __atomic_fetch_add(&box[0], 1u, __ATOMIC_RELEASE);
}
}  // namespace

extern "C" {

const char *bo_last_error(void) { return g_err.c_str(); }
int bo_abi_version(void) { return BENOR_ABI_VERSION; }
#ifndef BENOR_KERNEL_SHA
#define BENOR_KERNEL_SHA "unknown"
#endif
const char *bo_kernel_version(void) { return BENOR_KERNEL_SHA; }
uint32_t bo_hist_len(uint32_t k_max) { return (k_max + 1u) * 3u + 1u; }

// ------------------------------------------------------------ network API
int bo_network_create(uint32_t N, uint32_t F, const int8_t *init, uint32_t n_init,
                      const uint8_t *faulty, uint32_t n_faulty, bo_network **out) {
  if (!out) return fail(BO_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  // launchNodes.ts:10-11
  if (n_init != n_faulty || N != n_init) return fail(BO_ERR_ARRAYS_DONT_MATCH, "Arrays don't match");
  if (N > 0 && (!init || !faulty)) return fail(BO_ERR_INVALID_ARGUMENT, "initial_values / faulty_list is NULL");
  uint32_t cnt = 0;
  for (uint32_t i = 0; i < n_faulty; ++i) cnt += faulty[i] ? 1u : 0u;
  // launchNodes.ts:12-13
  if (cnt != F) return fail(BO_ERR_FAULTY_COUNT, "faultyList doesnt have F faulties");
  if (N > BO_MAX_N) return fail(BO_ERR_UNSUPPORTED, "N exceeds BO_MAX_N");
  for (uint32_t i = 0; i < N; ++i)
    if (init[i] < 0 || init[i] > 2) return fail(BO_ERR_INVALID_ARGUMENT, "initial value must be 0, 1 or '?'(2)");
  auto *net = new bo_network();
  net->N = N;
  net->F = F;
  net->st.resize(N);
  net->faulty.assign(faulty, faulty + N);
  for (uint32_t i = 0; i < N; ++i) {   // node.ts:21-26
    const bool f = faulty[i] != 0;
    net->st[i].killed = f ? 1 : 0;
    net->st[i].x = f ? -1 : init[i];
    net->st[i].decided = f ? -1 : 0;
    net->st[i].pad = 0;
    net->st[i].k = f ? -1 : 0;
  }
  *out = net;
  return BO_OK;
}

uint32_t bo_network_size(const bo_network *net) { return net ? net->N : 0u; }

void bo_network_destroy(bo_network *net) {
  if (!net) return;
  (void)bo_consensus_wait(net);   // a live run still holds device buffers
  delete net;
}

int bo_status(const bo_network *net, uint32_t i) {   // node.ts:33-39
  if (!net) return -fail(BO_ERR_INVALID_ARGUMENT, "net is NULL");
  if (i >= net->N) return -fail(BO_ERR_OUT_OF_RANGE, "node index out of range");
  std::lock_guard<std::mutex> g(net->mu);
  return net->st[i].killed ? 500 : 200;
}

namespace {
int get_states_impl(bo_network *net, bo_node_state *out, uint64_t *events_out);
}  // namespace

// GET /getState answers at once with the node's current state (node.ts:197-199):
// during a live run, from a snapshot the kernel takes at its next batch
// boundary (bo_get_states).
int bo_get_state(const bo_network *net, uint32_t i, bo_node_state *out) {   // node.ts:197-199
  if (!net || !out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  if (i >= net->N) return fail(BO_ERR_OUT_OF_RANGE, "node index out of range");
  {
    std::lock_guard<std::mutex> g(net->mu);
    if (!net->live) {
      *out = net->st[i];
      return net->live_rc;
    }
  }
  std::vector<bo_node_state> all(net->N);
  const int rc = get_states_impl(const_cast<bo_network *>(net), all.data(), nullptr);
  *out = all[i];
  return rc;
}

int bo_node_stop(bo_network *net, uint32_t i) {   // node.ts:191-194
  if (!net) return fail(BO_ERR_INVALID_ARGUMENT, "net is NULL");
  if (i >= net->N) return fail(BO_ERR_OUT_OF_RANGE, "node index out of range");
  std::lock_guard<std::mutex> g(net->mu);
  net->st[i].killed = 1;
  if (net->live) live_post(net->live.get(), &i, 1u);
  return BO_OK;
}

int bo_consensus_stop(bo_network *net) {   // consensus.ts:10-15
  if (!net) return fail(BO_ERR_INVALID_ARGUMENT, "net is NULL");
  std::lock_guard<std::mutex> g(net->mu);
  for (auto &s : net->st) s.killed = 1;
  if (net->live) {
    std::vector<uint32_t> all(net->N);
    for (uint32_t i = 0; i < net->N; ++i) all[i] = i;
    live_post(net->live.get(), all.data(), net->N);
  }
  return BO_OK;
}

int bo_consensus_start(bo_network *net, uint64_t seed, uint32_t k_max) {   // consensus.ts:3-8
  return bo_consensus_start_sched(net, seed, k_max, nullptr, 0u);
}

namespace {
// What a GET /start (node.ts:167-188) runs: the nodes not killed, their x, and
// their /stop schedule entries.  `launch` is false when nothing needs a kernel.
struct StartPlan {
  std::vector<uint8_t> crashed;
  std::vector<int8_t> x;
  std::vector<uint32_t> active, sched;
  bool scheduled = false;   // a /stop lands on a node that runs (entries of killed nodes are moot)
  bool launch = false;
};

int start_prologue(bo_network *net, uint32_t k_max, const uint32_t *stop_after, uint32_t n_stop_after,
                   StartPlan &sp) {
  if (!net) return fail(BO_ERR_INVALID_ARGUMENT, "net is NULL");
  if (k_max < 1 || k_max > BO_MAX_K) return fail(BO_ERR_INVALID_ARGUMENT, "k_max out of range");
  const uint32_t N = net->N;
  if (stop_after && n_stop_after != N) return fail(BO_ERR_INVALID_ARGUMENT, "stop schedule must have N entries");
  sp.crashed.assign(N, 0);
  sp.x.assign(N, 0);
  sp.sched.assign(N, 0xFFFFFFFFu);
  std::lock_guard<std::mutex> g(net->mu);
  // The reference's per-node inboxes (node.ts:29-30) live as long as the
  // server: a second GET /start pushes round-1 messages onto inboxes that
  // already hold them, and every push past N-F re-triggers the tally
  // (node.ts:47-52).  That is not a fresh consensus, so it is refused.
  if (net->started)
    return fail(BO_ERR_ALREADY_STARTED, net->in_flight
                ? "consensus is already running on this network"
                : "consensus already started on this network: node inboxes persist across /start "
                  "(node.ts:29-30), launch a new network to run again");
  // Nodes that run: not killed (faulty from launch, or stopped).  They send
  // and receive; killed nodes do neither (node.ts:45, :171).
  for (uint32_t i = 0; i < N; ++i) {
    sp.crashed[i] = net->st[i].killed ? 1 : 0;
    sp.x[i] = net->st[i].killed ? 0 : net->st[i].x;
    if (!net->st[i].killed) {
      sp.active.push_back(i);
      if (stop_after) sp.sched[i] = stop_after[i];
    }
  }
  for (uint32_t i : sp.active) sp.scheduled = sp.scheduled || sp.sched[i] != 0xFFFFFFFFu;
  if (sp.active.empty()) { net->started = true; return BO_OK; }
  const int64_t quorum = (int64_t)N - (int64_t)net->F;
  // Fewer running senders than the quorum: no R-phase ever triggers
  // (node.ts:52), every running node stays at k = 1, undecided.
  if ((int64_t)sp.active.size() < quorum) {
    for (uint32_t i : sp.active) net->st[i].k = 1;   // node.ts:172
    net->started = true;
    return BO_OK;
  }
  int dev = 0;
  const int rc = check_device(&dev);
  if (rc) return rc;
  net->started = true;
  net->in_flight = true;
  sp.launch = true;
  return BO_OK;
}

bo_trials_cfg start_cfg(const bo_network *net, uint64_t seed, uint32_t k_max, StartPlan &sp, int mode) {
  bo_trials_cfg cfg{};
  cfg.N = net->N;
  cfg.F = net->F;
  cfg.k_max = k_max;
  cfg.init_mode = BO_INIT_FIXED;
  cfg.mode = mode;
  cfg.seed = seed;
  cfg.faulty = sp.crashed.data();
  cfg.init = sp.x.data();
  cfg.crash_at = sp.scheduled ? sp.sched.data() : nullptr;
  return cfg;
}

// The run's final states into the network (caller holds net->mu).  A /stop
// the run applied is part of it (the kernel's killed flag); one served while
// the kernel ran but not applied by it is ordered after it: the node keeps its
// final x / decided / k and stays killed.
void merge_states(bo_network *net, const std::vector<uint32_t> &active, const std::vector<bo_node_state> &states) {
  const uint32_t N = net->N;
  for (uint32_t i : active) {
    const int8_t killed = net->st[i].killed;
    net->st[i] = states[i];
    net->st[i].killed = (int8_t)(killed | states[i].killed);
  }
  // The reference's auto-stop (node.ts:116-145): after its P-phase a node asks
  // every node's /getState and, when every answer has `decided` truthy, sends
  // /stop to all of them.  A faulty node answers decided: null (node.ts:24)
  // and a node stopped before the run answers false, so it fires only when
  // every node of the network decided -- then every node ends killed.
  bool all_decided = true;
  for (uint32_t i = 0; i < N; ++i) all_decided = all_decided && net->st[i].decided == 1;
  if (all_decided)
    for (uint32_t i = 0; i < N; ++i) net->st[i].killed = 1;
}
}  // namespace

namespace {
int run_sched_wg(const bo_trials_cfg *cfg, std::vector<bo_node_state> &states);
}  // namespace

// startConsensus with GET /stop requests landing during the run (node.ts:191-194
// served while the round loop is in flight).  Without a schedule: the lockstep
// round loop (every running node hears every running node).  With
// one: the event-level kernel, delivery by delivery in the seeded order, each
// scheduled /stop applied after its node's delivery count (oracle (iii)).
int bo_consensus_start_sched(bo_network *net, uint64_t seed, uint32_t k_max, const uint32_t *stop_after,
                             uint32_t n_stop_after) {
  StartPlan sp;
  int rc = start_prologue(net, k_max, stop_after, n_stop_after, sp);
  if (rc || !sp.launch) return rc;
  // Launch-time validation is already done; here the crashed set is the
  // killed set, which has exactly N - quorum = F members at this point.
  const bo_trials_cfg cfg = start_cfg(net, seed, k_max, sp, sp.scheduled ? BO_MODE_EVENT : BO_MODE_LOCKSTEP);
  std::vector<bo_node_state> states(net->N);
  uint32_t rounds = 0;
  // a schedule: one trial of the workgroup-batched event kernel; none: the
  // lockstep round loop
  rc = sp.scheduled ? run_sched_wg(&cfg, states) : bo_run_trial_states(&cfg, 0, states.data(), &rounds);
  std::lock_guard<std::mutex> g(net->mu);
  net->in_flight = false;
  if (rc) {
    net->started = false;          // nothing ran: the start may be retried
    return rc;
  }
  merge_states(net, sp.active, states);
  return BO_OK;
}

// ------------------------------------------------ RANDOM_TALLY table (host)
// Row K of the threshold table of Hypergeometric(m, K, q), the count of 1s in
// a uniform q-subset of m senders of which K hold a 1: support [lo, hi],
// lo = max(0, q - (m - K)), hi = min(K, q), and hi - lo thresholds
// T[j] = min(2^64 - 1, floor(CDF(lo + j) * 2^64)) appended to `thr`.  In double:
// weights by the ratio recurrence pmf(c + 1) / pmf(c) =
// (K - c)(q - c) / ((c + 1)(m - K - q + c + 1)) outward from the mode (weight 1,
// so nothing overflows and the far tails underflow harmlessly), then running
// sums over their total.  The sums never decrease, so neither do the
// thresholds.
static uint32_t tally_row(uint32_t m, uint32_t q, uint32_t K, std::vector<uint64_t> &thr, std::vector<double> &w) {
  const uint32_t lo = K + q > m ? K + q - m : 0u, hi = K < q ? K : q, n = hi - lo;
  if (n == 0u) return lo;
  uint32_t mode = (uint32_t)(((uint64_t)q + 1u) * ((uint64_t)K + 1u) / ((uint64_t)m + 2u));
  mode = mode < lo ? lo : (mode > hi ? hi : mode);
  w.assign(n + 1u, 0.0);
  auto ratio = [&](uint32_t c) {                 // pmf(c + 1) / pmf(c), lo <= c < hi
    return ((double)(K - c) * (double)(q - c)) / ((double)(c + 1u) * (double)(m - K - q + c + 1u));
  };
  w[mode - lo] = 1.0;
  for (uint32_t c = mode; c < hi; ++c) w[c + 1u - lo] = w[c - lo] * ratio(c);
  for (uint32_t c = mode; c > lo; --c) w[c - 1u - lo] = w[c - lo] / ratio(c - 1u);
  double total = 0.0;
  for (uint32_t i = 0; i <= n; ++i) total += w[i];
  double run = 0.0;
  for (uint32_t j = 0; j < n; ++j) {
    run += w[j];
    const double t = std::ldexp(run / total, 64);
    thr.push_back(t >= 18446744073709551616.0 ? ~0ull : (uint64_t)t);
  }
  return lo;
}

int bo_tally_cdf(uint32_t m, uint32_t q, uint32_t K, uint32_t *lo_out, uint64_t *thr_out, uint32_t cap,
                 uint32_t *n_out) {
  if (!lo_out || !n_out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  if (K > m || q > m) return fail(BO_ERR_INVALID_ARGUMENT, "bo_tally_cdf needs K <= m and q <= m");
  const uint32_t n = (K < q ? K : q) - (K + q > m ? K + q - m : 0u);   // hi - lo: checked before the row is built
  if (n > cap || (n && !thr_out)) return fail(BO_ERR_INVALID_ARGUMENT, "bo_tally_cdf: thr_out is too short for the row");
  std::vector<uint64_t> thr;
  std::vector<double> w;
  const uint32_t lo = tally_row(m, q, K, thr, w);
  *lo_out = lo;
  *n_out = (uint32_t)thr.size();
  if (!thr.empty()) std::memcpy(thr_out, thr.data(), sizeof(uint64_t) * thr.size());
  return BO_OK;
}

// ------------------------------------------------- BYZ_TALLY thresholds (host)
// The b thresholds of Binomial(b, p), p = one / 2^32 (exact in double, as 1 - p is):
// T[j] = min(2^64 - 1, floor(CDF(j) * 2^64)), j = 0..b-1.  tally_row's construction:
// weights by the ratio recurrence pmf(j + 1) / pmf(j) = (b - j) p / ((j + 1)(1 - p))
// outward from the mode (weight 1), then running sums over their total.
static void byz_row(uint32_t b, uint32_t one, std::vector<uint64_t> &thr) {
  thr.clear();
  if (b == 0u) return;
  const double p = std::ldexp((double)one, -32), np = 1.0 - p;
  uint32_t mode = (uint32_t)(((uint64_t)b + 1u) * one >> 32);   // floor((b + 1) p) <= b
  std::vector<double> w(b + 1u, 0.0);
  auto ratio = [&](uint32_t j) { return ((double)(b - j) * p) / ((double)(j + 1u) * np); };   // 0 <= j < b
  w[mode] = 1.0;
  for (uint32_t j = mode; j < b; ++j) w[j + 1u] = w[j] * ratio(j);
  for (uint32_t j = mode; j > 0u; --j) w[j - 1u] = w[j] / ratio(j - 1u);   // mode > 0 only if p > 0
  double total = 0.0;
  for (uint32_t j = 0; j <= b; ++j) total += w[j];
  double run = 0.0;
  for (uint32_t j = 0; j < b; ++j) {
    run += w[j];
    const double t = std::ldexp(run / total, 64);
    thr.push_back(t >= 18446744073709551616.0 ? ~0ull : (uint64_t)t);
  }
}

int bo_byz_cdf(uint32_t b, uint32_t byz_one, uint64_t *thr_out, uint32_t cap, uint32_t *n_out) {
  if (!n_out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  if (b > BO_MAX_N) return fail(BO_ERR_INVALID_ARGUMENT, "bo_byz_cdf needs b <= 4096");
  if (b > cap || (b && !thr_out)) return fail(BO_ERR_INVALID_ARGUMENT, "bo_byz_cdf: thr_out is too short for b thresholds");
  std::vector<uint64_t> thr;
  byz_row(b, byz_one, thr);
  *n_out = b;
  if (b) std::memcpy(thr_out, thr.data(), sizeof(uint64_t) * b);
  return BO_OK;
}

// ------------------------------------------ Binomial(2^k, 1/2) thresholds (host)
// The lumped API's table of one k (include/benor.h).  n = 2^k, mode n / 2.  Weights by
// the ratio recurrence pmf(x - 1) / pmf(x) = x / (n - x + 1) downward from the mode
// (weight 1) over the window W = ceil(5 sqrt(n)) below it -- by Hoeffding the mass
// beyond is under 2^-72 of the total, less than one unit of a threshold.  The law is
// symmetric, so the total is twice the sum below the mode plus the mode's weight; the
// lower half's running sums start at the far tail (small terms first), and the upper
// half is the mirror image: CDF(x) = 1 - CDF(n - 1 - x), thr = 2^64 - ceil(.).  lgamma
// is not used: at n = 2^24 it leaves eight digits.
static void binom_half_row(uint32_t k, uint32_t &lo, std::vector<uint64_t> &thr) {
  const uint32_t n = 1u << k, mode = n >> 1;
  uint32_t W = (uint32_t)std::ceil(5.0 * std::sqrt((double)n)) + 1u;
  if (W > mode) W = mode;
  std::vector<long double> w(W + 1u);              // w[d]: the weight of x = mode - d
  w[0] = 1.0L;
  for (uint32_t d = 1; d <= W; ++d) {
    const uint32_t x = mode - d + 1u;              // pmf(x - 1) = pmf(x) * x / (n - x + 1)
    w[d] = w[d - 1u] * (long double)x / (long double)(n - x + 1u);
  }
  long double below = 0.0L;
  for (uint32_t d = W; d >= 1u; --d) below += w[d];
  const long double total = 2.0L * below + w[0];
  std::vector<long double> cdf(W);                 // cdf[i] = CDF(mode - W + i), i < W: x below the mode
  long double run = 0.0L;
  for (uint32_t i = 0; i < W; ++i) {
    run += w[W - i];
    cdf[i] = run / total;
  }
  thr.clear();
  lo = 0u;
  bool any = false;
  for (uint32_t i = 0; i < W; ++i) {               // the lower half: floor(CDF 2^64) < 2^63
    const uint64_t t = (uint64_t)std::floor(std::ldexp(cdf[i], 64));
    if (!any && t == 0u) continue;
    if (!any) lo = mode - W + i, any = true;
    thr.push_back(t);
  }
  if (!any) lo = mode;
  for (uint32_t i = W; i-- > 0u;) {                // x = n - 1 - (mode - W + i) = mode, mode + 1, ..
    const uint64_t c = (uint64_t)std::ceil(std::ldexp(cdf[i], 64));
    if (c <= 1u) break;                            // saturated from here on
    thr.push_back(0u - c);
  }
}

int bo_binom_half_cdf(uint32_t k, uint32_t *lo_out, uint64_t *thr_out, uint32_t cap, uint32_t *n_out) {
  if (!lo_out || !n_out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  if (k < benor::lumped::kTableMinK || k > benor::lumped::kTableMaxK)
    return fail(BO_ERR_INVALID_ARGUMENT, "bo_binom_half_cdf needs 7 <= k <= 24");
  uint32_t lo = 0;
  std::vector<uint64_t> thr;
  binom_half_row(k, lo, thr);
  if (thr.size() > cap || !thr_out) return fail(BO_ERR_INVALID_ARGUMENT, "bo_binom_half_cdf: thr_out is too short for the table");
  *lo_out = lo;
  *n_out = (uint32_t)thr.size();
  std::memcpy(thr_out, thr.data(), sizeof(uint64_t) * thr.size());
  return BO_OK;
}

// ------------------------------------------------------------- lumped API
// The adversarial scheduler at the level of classes (include/benor.h):
// validation is benor_lumped.h's, the kernel benor_lumped.hip's.  The tables of every
// k are built once per process and uploaded once per device; they are never freed
// (about 1 MB; freeing device memory while the process exits can race the runtime's teardown).
namespace {
struct LumpedTables {
  std::vector<uint64_t> thr;
  std::vector<uint32_t> dir;                       // off[kTables + 1], then lo[kTables]
};

const LumpedTables *lumped_tables() {
  static const LumpedTables tables = [] {
    LumpedTables t;
    std::vector<uint32_t> off{0u}, lo;
    std::vector<uint64_t> row;
    for (uint32_t k = benor::lumped::kTableMinK; k <= benor::lumped::kTableMaxK; ++k) {
      uint32_t l = 0;
      binom_half_row(k, l, row);
      t.thr.insert(t.thr.end(), row.begin(), row.end());
      off.push_back((uint32_t)t.thr.size());
      lo.push_back(l);
    }
    t.dir = off;
    t.dir.insert(t.dir.end(), lo.begin(), lo.end());
    return t;
  }();
  return &tables;
}

struct LumpedDevice {
  int device;
  unsigned char *d;                                // thr, then dir
};
std::mutex g_lumped_mu;
std::vector<LumpedDevice> g_lumped_dev;

int lumped_device_tables(int dev, benor::lumped::TableDir &out) {
  const LumpedTables &t = *lumped_tables();
  const size_t thr_bytes = sizeof(uint64_t) * t.thr.size(), dir_bytes = sizeof(uint32_t) * t.dir.size();
  std::lock_guard<std::mutex> lock(g_lumped_mu);
  unsigned char *d = nullptr;
  for (const LumpedDevice &e : g_lumped_dev)
    if (e.device == dev) d = e.d;
  if (!d) {
    HIP_TRY(hipMalloc(&d, thr_bytes + dir_bytes));
    hipError_t e = hipMemcpy(d, t.thr.data(), thr_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + thr_bytes, t.dir.data(), dir_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return hip_fail(e, "lumped tables upload");
    }
    g_lumped_dev.push_back({dev, d});
  }
  out.thr = reinterpret_cast<const uint64_t *>(d);
  out.off = reinterpret_cast<const uint32_t *>(d + thr_bytes);
  out.lo = out.off + benor::lumped::kTables + 1u;
  return BO_OK;
}

// A threshold rule's words (benor_rule.h).
int rule_check(const bo_rule *rule) {
  if (!rule) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  const char *msg = "";
  const int rc = benor::rule::check(*rule, &msg);
  return rc ? fail(rc, msg) : BO_OK;
}

// `rule`: NULL for the configuration's own rule (cfg->rule), else the threshold rule that replaces it.
int lumped_check(const bo_lumped_cfg *cfg, const bo_rule *rule = nullptr) {
  if (!cfg) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  const char *msg = "";
  const int rc = benor::lumped::check(*cfg, &msg, rule == nullptr);
  if (rc) return fail(rc, msg);
  return rule ? rule_check(rule) : BO_OK;
}

// Trials [begin, begin + count) added into hist (host); `state`: the one trial's final state.
int lumped_launch(const bo_lumped_cfg *cfg, const bo_rule *rule, uint64_t begin, uint64_t count, uint64_t *hist,
                  bo_lumped_state *state) {
  int rc = lumped_check(cfg, rule);
  if (rc) return rc;
  if (!hist && !state) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  if (count == 0u) return BO_OK;
  int dev = 0;
  rc = check_device(&dev);
  if (rc) return rc;
  benor::LumpedParams p;
  std::memset(&p, 0, sizeof p);
  p.s = benor::lumped::shape_of(*cfg);
  p.rule = rule ? benor::lumped::RuleT::kRule : cfg->rule;
  if (rule) p.thresholds = *rule;
  p.coin_common = cfg->coin_common, p.k_max = cfg->k_max, p.hist_len = bo_hist_len(cfg->k_max);
  p.init_mode = cfg->init_mode, p.init0 = cfg->init0, p.init1 = cfg->init1;
  p.seed = cfg->seed;
  rc = lumped_device_tables(dev, p.tables);
  if (rc) return rc;
  const uint32_t H = p.hist_len;
  const size_t o_state = sizeof(uint64_t) * H;
  unsigned char *d = nullptr;
  HIP_TRY(hipMalloc(&d, o_state + sizeof(bo_lumped_state)));
  p.hist = reinterpret_cast<unsigned long long *>(d);
  p.state_out = state ? reinterpret_cast<bo_lumped_state *>(d + o_state) : nullptr;
  hipError_t e = hipMemset(d, 0, o_state + sizeof(bo_lumped_state));
  int cus = 0;
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  int per_cu = (int)benor::knob_u32("BENOR_BLOCKS_PER_CU", 0u);
  if (per_cu < 1) per_cu = benor::lumped_blocks_per_cu(p);
  if (per_cu < 1) per_cu = 8;
  for (uint64_t done = 0; e == hipSuccess && done < count; done += benor::kMaxTrialsPerLaunch) {
    p.trial_begin = begin + done;
    p.trial_count = std::min<uint64_t>(count - done, benor::kMaxTrialsPerLaunch);
    const uint64_t want = (p.trial_count + benor::kLumpedBlock - 1u) / benor::kLumpedBlock;
    const int grid = (int)std::min<uint64_t>(want, (uint64_t)std::max(1, cus) * per_cu);
    e = benor::launch_lumped(p, grid, nullptr);
  }
  std::vector<uint64_t> h(H);
  bo_lumped_state st;
  if (e == hipSuccess) e = hipMemcpy(h.data(), d, o_state, hipMemcpyDeviceToHost);
  if (e == hipSuccess && state) e = hipMemcpy(&st, d + o_state, sizeof st, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return hip_fail(e, "bo_lumped_run");
  if (hist)
    for (uint32_t i = 0; i < H; ++i) hist[i] += h[i];
  if (state) *state = st;
  return BO_OK;
}
}  // namespace

int bo_lumped_check(const bo_lumped_cfg *cfg) { return lumped_check(cfg); }

int bo_lumped_run(const bo_lumped_cfg *cfg, uint64_t trial_begin, uint64_t trial_count, uint64_t *hist_host) {
  if (!hist_host) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  return lumped_launch(cfg, nullptr, trial_begin, trial_count, hist_host, nullptr);
}

int bo_lumped_trial(const bo_lumped_cfg *cfg, uint64_t trial, bo_lumped_state *out) {
  if (!out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  return lumped_launch(cfg, nullptr, trial, 1, nullptr, out);
}

// ... with a threshold rule in the place of cfg->rule, which is not read
int bo_lumped_check_rule(const bo_lumped_cfg *cfg, const bo_rule *rule) {
  if (!rule) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  return lumped_check(cfg, rule);
}

int bo_lumped_run_rule(const bo_lumped_cfg *cfg, const bo_rule *rule, uint64_t trial_begin, uint64_t trial_count,
                       uint64_t *hist_host) {
  if (!rule || !hist_host) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  return lumped_launch(cfg, rule, trial_begin, trial_count, hist_host, nullptr);
}

int bo_lumped_trial_rule(const bo_lumped_cfg *cfg, const bo_rule *rule, uint64_t trial, bo_lumped_state *out) {
  if (!rule || !out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  return lumped_launch(cfg, rule, trial, 1, nullptr, out);
}

// The presets (benor_rule.h).
static int rule_preset(bool b, uint32_t N, uint32_t F, bo_rule *out) {
  if (!out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  if (!benor::rule::preset_fits(N, F))
    return fail(BO_ERR_INVALID_ARGUMENT, "bo_rule: N + F and 2 F must be at most 2^31 - 1");
  *out = b ? benor::rule::protocol_b(N, F) : benor::rule::protocol_a(N, F);
  return BO_OK;
}
int bo_rule_protocol_a(uint32_t N, uint32_t F, bo_rule *out) { return rule_preset(false, N, F, out); }
int bo_rule_protocol_b(uint32_t N, uint32_t F, bo_rule *out) { return rule_preset(true, N, F, out); }

// -------------------------------------------------------------- batch API
// Validation and kernel planning of a trial configuration, host only: the
// live-node map, the fixed-init plane and the KParams shape (no device fields).
// Which words a mode reads and which family it belongs to: benor_modes.h.
// plan_host is the common part; a family's own checks and plan are entered on
// its traits flag (check_ / plan_crash_family, check_ / plan_byz_family: the
// checks run where they always did, so the first error of a configuration is
// the one it was).
using benor::ModeTraits;
using benor::mode_traits;

// The crash family, host side of a non-empty schedule: the explicit list
// (step << 12 | compact index, ascending, steps below 2 k_max: no run reaches a
// later one) and, per number of crashes so far d = 0 .. kp.cr_n, whether the
// live count m0 - d is reachable and so needs a table.
struct CrashSchedule {
  std::vector<uint32_t> list;
  std::vector<uint8_t> reach;
};
// What a plan uploads besides the live map and the init plane: the schedule, and the Byzantine
// family's honest plane, bit c of word c / 64 set for an honest compact index c.
struct PlanTables {
  CrashSchedule crash;
  std::vector<uint64_t> honest;
};

// Thresholds of the table of (m, q): sum over K = 0..m of min(K, q) - max(0, q - (m - K)).
static uint64_t tally_table_len(uint32_t m, uint32_t q) {
  uint64_t n = 0;
  for (uint32_t K = 0; K <= m; ++K) n += (K < q ? K : q) - (K + q > m ? K + q - m : 0u);
  return n;
}

// The Byzantine family alone reads the value of a faulty entry: 1 crashed from the start, 2 Byzantine
// (live: it sends); every other mode reads non-zero as faulty.  Under an adversarial scheduler the
// strategy names the scheduler's aim.
static int check_byz_family(const bo_trials_cfg *cfg, const ModeTraits &mode) {
  for (uint32_t i = 0; i < cfg->N; ++i)
    if (cfg->faulty[i] > 2u)
      return fail(BO_ERR_INVALID_ARGUMENT, std::string(mode.name) + ": a faulty entry is 0, 1 (crashed) or 2 (Byzantine)");
  const bool inbox = cfg->byz_strategy == BO_BYZ_BALANCE || cfg->byz_strategy == BO_BYZ_SPLIT;
  if (!inbox && cfg->byz_strategy != BO_BYZ_RANDOM && cfg->byz_strategy != BO_BYZ_OPPOSE)
    return fail(BO_ERR_INVALID_ARGUMENT,
                "byz_strategy must be BO_BYZ_RANDOM, BO_BYZ_OPPOSE, BO_BYZ_BALANCE or BO_BYZ_SPLIT");
  if (mode.is(benor::kModeSched) && !inbox)
    return fail(BO_ERR_INVALID_ARGUMENT,
                "byz_strategy must be BO_BYZ_BALANCE or BO_BYZ_SPLIT under an adversarial scheduler "
                "(BO_MODE_SCHED_TALLY, BO_MODE_SCHED_RULE_B)");
  return BO_OK;
}

// Crashes during the run: with the f initially faulty nodes at most F, so every step has a quorum of
// live senders.  n_crash: the nodes scheduled; random: crash_count of them drawn per trial.
static int check_crash_family(const bo_trials_cfg *cfg, const ModeTraits &mode, const std::vector<uint32_t> &live,
                              uint32_t f, uint64_t &n_crash, bool &random) {
  const uint32_t m = (uint32_t)live.size();
  if (cfg->crash_at) {
    for (uint32_t c = 0; c < m; ++c) n_crash += cfg->crash_at[live[c]] != 0xFFFFFFFFu ? 1u : 0u;
  } else if (cfg->crash_count > 0) {
    if (cfg->crash_window < 1) return fail(BO_ERR_INVALID_ARGUMENT, "crash_count > 0 needs crash_window >= 1");
    n_crash = cfg->crash_count;
    random = true;
  }
  if ((uint64_t)f + n_crash > cfg->F)
    return fail(BO_ERR_FAULTY_COUNT, std::string(mode.name) + " needs at most F nodes faulty or scheduled to crash");
  // Partial broadcasts: a cut counts initially-live receivers
  // (BO_MODE_CRASH_SUBSET reads the word as crash_reach, a probability in units of 2^-32: every value is one)
  if (cfg->mode == BO_MODE_CRASH_PARTIAL && cfg->crash_cut != BO_CUT_RANDOM && cfg->crash_cut > m)
    return fail(BO_ERR_INVALID_ARGUMENT, "crash_cut must be at most the initially-live count N - f, or BO_CUT_RANDOM");
  return BO_OK;
}

// A crash-family plan with a non-empty schedule: the list, the reachable live counts, the table limit.
static int plan_crash_family(const bo_trials_cfg *cfg, const std::vector<uint32_t> &live, uint64_t n_crash, bool random,
                             benor::KParams &kp, CrashSchedule &cs) {
  const uint32_t m = kp.m;
  cs.list.clear();
  kp.cr_random = random ? 1u : 0u;
  kp.cr_cut = kp.mode == BO_MODE_CRASH_PARTIAL ? cfg->crash_cut : 0u;
  if (kp.mode == BO_MODE_CRASH_SUBSET) kp.cr_reach = cfg->crash_reach;
  if (random) {
    kp.cr_n = (uint32_t)n_crash;
    cs.reach.assign(kp.cr_n + 1u, 1);            // every m0 - j, j = 0 .. crash_count
  } else {
    for (uint32_t c = 0; c < m; ++c) {
      const uint32_t s = cfg->crash_at[live[c]];
      if (s != 0xFFFFFFFFu && (uint64_t)s < 2ull * cfg->k_max) cs.list.push_back(s << 12 | c);
    }
    std::sort(cs.list.begin(), cs.list.end());
    kp.cr_n = (uint32_t)cs.list.size();
    cs.reach.assign(kp.cr_n + 1u, 0);            // m0 minus the cumulative crashes at each distinct step
    cs.reach[0] = 1;
    for (uint32_t i = 0; i < kp.cr_n; ++i)
      if (i + 1u == kp.cr_n || (cs.list[i + 1u] >> 12) != (cs.list[i] >> 12)) cs.reach[i + 1u] = 1;
    // Partial broadcasts: a receiver's pool is the alive set and the step's crashers that reach
    // it.  A fixed cut gives all of them or none, live counts of the set above; random cuts
    // any number of them, so every m0 - j
    if (kp.mode == BO_MODE_CRASH_PARTIAL && kp.cr_cut == BO_CUT_RANDOM) cs.reach.assign(kp.cr_n + 1u, 1);
    // A random subset: any number of a step's crashers may reach a receiver, every m0 - j (at reach
    // 0 and UINT32_MAX too: one rule for the mode)
    if (kp.mode == BO_MODE_CRASH_SUBSET) cs.reach.assign(kp.cr_n + 1u, 1);
  }
  uint64_t bytes = 0;
  for (uint32_t d = 0; d <= kp.cr_n; ++d)
    if (cs.reach[d]) bytes += 8ull * tally_table_len(m - d, kp.q);
  if (bytes > BO_CRASH_TABLE_MAX_BYTES)
    return fail(BO_ERR_UNSUPPORTED,
                std::string(mode_traits(kp.mode)->name) + ": the threshold tables of the reachable " +
                    (kp.mode == BO_MODE_CRASH_TALLY ? "live counts" : "pool sizes") +
                    " exceed the 512 MiB limit (BO_CRASH_TABLE_MAX_BYTES): schedule fewer crashes");
  return BO_OK;
}

// A Byzantine-family plan: the strategy words and the honest plane.
static void plan_byz_family(const bo_trials_cfg *cfg, const std::vector<uint32_t> &live, uint32_t nbyz,
                            benor::KParams &kp, std::vector<uint64_t> *honest) {
  kp.byz_n = nbyz;
  kp.byz_strategy = cfg->byz_strategy;
  kp.byz_one = cfg->byz_one;
  if (!honest) return;
  honest->assign(kp.W, 0ull);
  for (uint32_t c = 0; c < kp.m; ++c)
    if (cfg->faulty[live[c]] == 0u) (*honest)[c >> 6] |= 1ull << (c & 63u);
}

static int plan_host(const bo_trials_cfg *cfg, std::vector<uint32_t> &live, std::vector<uint4> &plane,
                     benor::KParams &kp, bool live_run = false, PlanTables *tables = nullptr) {
  if (!cfg) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  if (cfg->N < 1 || cfg->N > BO_MAX_N) return fail(BO_ERR_UNSUPPORTED, "N must be in [1, 4096]");
  if (cfg->k_max < 1 || cfg->k_max > BO_MAX_K) return fail(BO_ERR_INVALID_ARGUMENT, "k_max must be in [1, 1024]");
  const ModeTraits *mode = mode_traits(cfg->mode);
  if (!mode) return fail(BO_ERR_UNSUPPORTED, "unknown delivery mode");
  const bool byz_mode = mode->is(benor::kModeByz), coin_mode = mode->is(benor::kModeCoin);
  if (cfg->init_mode != BO_INIT_RANDOM && cfg->init_mode != BO_INIT_FIXED)
    return fail(BO_ERR_INVALID_ARGUMENT, "unknown init_mode");
  if (!cfg->faulty) return fail(BO_ERR_INVALID_ARGUMENT, "faulty is NULL");
  if (cfg->init_mode == BO_INIT_FIXED && !cfg->init) return fail(BO_ERR_INVALID_ARGUMENT, "init is NULL");
  if (byz_mode) {
    const int rc = check_byz_family(cfg, *mode);
    if (rc) return rc;
  }
  const auto crashed = [&](uint32_t i) { return byz_mode ? cfg->faulty[i] == 1u : cfg->faulty[i] != 0u; };
  uint32_t f = 0, nbyz = 0;
  for (uint32_t i = 0; i < cfg->N; ++i) {
    f += crashed(i) ? 1u : 0u;
    nbyz += byz_mode && cfg->faulty[i] == 2u ? 1u : 0u;
  }
  // Lockstep = the reference's admissible inputs: exactly F crash faults
  // (launchNodes.ts:12-13).  Random delivery admits f <= F.
  if (!mode->is(benor::kModeRandom) && f != cfg->F)
    return fail(BO_ERR_FAULTY_COUNT, "faultyList doesnt have F faulties");
  if (mode->is(benor::kModeRandom) && f > cfg->F)
    return fail(BO_ERR_FAULTY_COUNT, "random delivery needs at most F crash-faulty nodes");
  if (f + nbyz > cfg->F)
    return fail(BO_ERR_FAULTY_COUNT, std::string(mode->name) + " needs at most F nodes crashed or Byzantine");
  live.clear();
  for (uint32_t i = 0; i < cfg->N; ++i)
    if (!crashed(i)) live.push_back(i);
  const uint32_t m = (uint32_t)live.size();
  uint64_t n_crash = 0;
  bool crash_random = false;
  if (mode->is(benor::kModeCrash)) {
    const int rc = check_crash_family(cfg, *mode, live, f, n_crash, crash_random);
    if (rc) return rc;
  }
  kp = benor::KParams{};
  kp.N = cfg->N;
  kp.F = cfg->F;
  kp.m = m;
  kp.W = (m + 63u) / 64u;
  kp.k_max = cfg->k_max;
  kp.init_mode = cfg->init_mode;
  kp.seed = cfg->seed;
  kp.mode = cfg->mode;
  // A shared-coin plan whose rounds are never common is its parent mode's plan (under a scheduler: its own);
  // otherwise it carries the word.
  if (coin_mode && cfg->coin_common == 0u) kp.mode = mode->coin_parent;
  if (coin_mode) kp.coin_common = cfg->coin_common;
  kp.q = cfg->N - cfg->F;
  kp.crash_count = byz_mode ? 0u : cfg->crash_count;      // (the Byzantine family: the word is byz_strategy)
  kp.crash_window = coin_mode ? 0u : cfg->crash_window;   // (the shared-coin modes: the word is coin_common)
  if (cfg->mode == BO_MODE_EVENT && !cfg->crash_at && cfg->crash_count > 0 && cfg->crash_window > 0)
    kp.ev_rstops = std::min<uint32_t>(cfg->crash_count, m);   // per-trial random /stop schedule
  kp.live = live_run && cfg->mode == BO_MODE_EVENT ? 1u : 0u;
  for (uint32_t i = 0; i < cfg->N && i < 4u * 64u; ++i)
    if (cfg->faulty[i]) kp.faulty_mask[i >> 6] |= 1ull << (i & 63u);
  if (m == 0 || m == nbyz) {                        // no live node, or (N = F only) no honest one: bin[2], no kernel
    kp.m = 0;
    kp.W = 0;
    kp.hist_len = bo_hist_len(cfg->k_max);
    return BO_OK;
  }
  plane.assign(kp.W, make_uint4(0, 0, 0, 0));
  if (cfg->init_mode == BO_INIT_FIXED) {
    uint32_t n0 = 0, n1 = 0;
    for (uint32_t c = 0; c < m; ++c) {
      const int8_t v = cfg->init[live[c]];
      if (v < 0 || v > 2) return fail(BO_ERR_INVALID_ARGUMENT, "initial value must be 0, 1 or '?'(2)");
      const uint32_t w = c >> 6, b = c & 63u;
      uint32_t *r = reinterpret_cast<uint32_t *>(&plane[w]);
      if (v == 0) { r[b >> 5] |= 1u << (b & 31u); ++n0; }
      if (v == 1) { r[2 + (b >> 5)] |= 1u << (b & 31u); ++n1; }
      if (v == 2) ++kp.init_q;
    }
    kp.init_tie = n0 == n1 ? 1u : 0u;
  }
  // Count-level random delivery draws two-category counts: every vote binary
  // and no tally tie, i.e. an odd quorum and no "?" initial value.
  if (cfg->mode == BO_MODE_RANDOM_TALLY && !(kp.q & 1u))
    return fail(BO_ERR_UNSUPPORTED, "BO_MODE_RANDOM_TALLY needs an odd quorum N - F: use BO_MODE_RANDOM_DELIVERY");
  if (cfg->mode == BO_MODE_RANDOM_TALLY && kp.init_q)
    return fail(BO_ERR_UNSUPPORTED, "BO_MODE_RANDOM_TALLY takes no \"?\" initial value: use BO_MODE_RANDOM_DELIVERY");
  // The demotions, in this order (the order decides the plan; a shared-coin mode became its parent
  // above).  A crash-family plan with an empty schedule is the three-valued mode's plan,
  if (mode->is(benor::kModeCrash) && n_crash == 0) kp.mode = BO_MODE_RANDOM_TALLY3;
  // ... and so is a BO_MODE_BYZ_TALLY plan without a Byzantine node, at every byz_one and strategy
  // (the other rule keeps its plan: the rule differs; a shared coin keeps its plan at b = 0: mode 4
  // has no such coin; so does a scheduler)
  if (kp.mode == BO_MODE_BYZ_TALLY && nbyz == 0) kp.mode = BO_MODE_RANDOM_TALLY3;
  if (mode_traits(kp.mode)->is(benor::kModeByz)) plan_byz_family(cfg, live, nbyz, kp, tables ? &tables->honest : nullptr);
  // The three-valued mode is a superset of the two-valued one: inside that scope it is that mode's
  // plan (its kernel, its results bit for bit); outside, benor_tally3.hip.
  if (kp.mode == BO_MODE_RANDOM_TALLY3 && (kp.q & 1u) && !kp.init_q) kp.mode = BO_MODE_RANDOM_TALLY;
  if (mode_traits(kp.mode)->is(benor::kModeCrash)) {
    CrashSchedule local;
    const int rc = plan_crash_family(cfg, live, n_crash, crash_random, kp, tables ? tables->crash : local);
    if (rc) return rc;
  }
  benor::plan_geometry(kp);   // after init_q: the kernel choice depends on the round-1 vote parity
  // The workgroup-batched event kernel holds a random /stop schedule's keys in LDS, 8 bytes a stop: at N near
  // BO_MAX_N some 1600 of them pass the device's limit, and the launch would fail in hipFuncSetAttribute.  Only a
  // batch plan under BENOR_EVENT_FORM=wg gets there (a live run and a network start carry no crash_count, and
  // without the knob such a plan runs the wave-per-trial kernel, whose keys are in global memory): refused here,
  // not rerouted, since the knob exists to put a plan on this kernel.
  if (kp.variant == benor::kVarEventWave && kp.ev_wg && !benor::event_wg_lds_fits(kp))
    return fail(BO_ERR_UNSUPPORTED,
                "event level on the workgroup-batched kernel (BENOR_EVENT_FORM=wg): " + std::to_string(kp.lds_bytes) +
                    " bytes of LDS exceed the device's " + std::to_string(benor::kEventWgLdsLimit) +
                    " (N = " + std::to_string(kp.N) + ", " + std::to_string(kp.ev_rstops) +
                    " random stops at 8 bytes each): schedule fewer stops or run without the knob");
  return BO_OK;
}

// BO_KERNEL_* of a plan: its variant, except the wave-per-trial event kernel
// (kVarEventWave: N > 256 or a live run), which is the event-level family too.
static int kernel_family(const benor::KParams &kp) {
  if (kp.m == 0) return BO_KERNEL_NONE;
  return kp.variant == benor::kVarEventWave ? BO_KERNEL_EVENT : (int)kp.variant;
}

int bo_kernel_for(const bo_trials_cfg *cfg, int *kernel_out) {
  if (!kernel_out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  std::vector<uint32_t> live;
  std::vector<uint4> plane;
  benor::KParams kp;
  const int rc = plan_host(cfg, live, plane, kp);
  if (rc) return rc;
  *kernel_out = kernel_family(kp);
  return BO_OK;
}

// A count-level plan's device tables: one buffer of sections, each at the next 8-byte-aligned offset in
// the order they are added (the kernels rely on the order and the alignment).  add: `bytes` from `src`,
// the section at least `min_bytes` long; it returns the section's offset.  upload allocates once and
// copies every non-empty section from where it lies (the crash family's tables may reach 512 MiB: no
// second host copy).
struct TableUpload {
  struct Section {
    const void *src;
    size_t bytes, offset;
  };
  std::vector<Section> sections;
  size_t total = 0;
  size_t add(const void *src, size_t bytes, size_t min_bytes = 0u) {
    sections.push_back({src, bytes, total});
    total += (std::max(bytes, min_bytes) + 7u) & ~size_t(7);
    return sections.back().offset;
  }
  hipError_t upload(unsigned char **dev) const {
    hipError_t e = hipMalloc(dev, total);
    for (const Section &s : sections)
      if (e == hipSuccess && s.bytes) e = hipMemcpy(*dev + s.offset, s.src, s.bytes, hipMemcpyHostToDevice);
    return e;
  }
};

// A threshold rule replaces Protocol B's rule on the plans of the three modes that run it; the
// plan is otherwise the mode's own, word for word.  Host only: the argument errors need no device.
static int check_rule_base(const bo_trials_cfg *cfg, const bo_rule *rule) {
  if (!cfg || !rule) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  if (cfg->mode != BO_MODE_BYZ_RULE_B && cfg->mode != BO_MODE_BYZ_RULE_B_COIN && cfg->mode != BO_MODE_SCHED_RULE_B)
    return fail(BO_ERR_INVALID_ARGUMENT,
                "a threshold rule needs mode BO_MODE_BYZ_RULE_B, BO_MODE_BYZ_RULE_B_COIN or BO_MODE_SCHED_RULE_B "
                "(the plan whose rule it replaces)");
  return rule_check(rule);
}

// ---- What plan_create_impl uploads besides the live map and the init plane, family by family.  Each allocates
// into the plan's d_* members, which the plan's destructor frees whatever happens after, and points pl->kp there.

// Event level: the initial values, the /stop schedule, the scratch of as many trials as run at once.
static int upload_event(bo_plan *pl, const bo_trials_cfg *cfg, bool live_run) {
  benor::KParams &kp = pl->kp;
  std::vector<int8_t> ix(cfg->N, 0);
  if (cfg->init_mode == BO_INIT_FIXED)
    for (uint32_t i = 0; i < cfg->N; ++i) ix[i] = cfg->init[i];
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, pl->device);
  const uint64_t slot = (uint64_t)kp.ev_stride * 4u;   // scratch bytes of a trial
  const bool wave = kp.variant == benor::kVarEventWave;
  std::vector<uint64_t> stops;
  if (wave) {
    // one wave per trial, each with a pool of ev_cap messages: as many
    // concurrent trials as CUs, within ~4 GiB of pools
    if (cfg->crash_at)
      for (uint32_t i = 0; i < cfg->N; ++i)
        if (cfg->crash_at[i] != 0xFFFFFFFFu) stops.push_back(((uint64_t)cfg->crash_at[i] << 12) | i);
    std::sort(stops.begin(), stops.end());
    kp.ev_lanes = std::max<uint64_t>(1u, std::min<uint64_t>((uint64_t)cus, (4ull << 30) / slot));
    if (live_run) kp.ev_lanes = 1u;                // a live run is one trial
  } else {
    // scratch: one slice per lane, at most ~4 GiB
    // Lanes per CU: the mode is bound by the latency of per-lane scratch
    // accesses, so fewer lanes whose slices stay cache-resident beat full
    // occupancy: 512 per CU for slices up to 4 KiB (N <= 12), else 256
    // (tools/ev_sweep.sh, BENOR_EVENT_LANES_PER_CU overrides).
    uint64_t per_cu = benor::knob_u32("BENOR_EVENT_LANES_PER_CU", slot <= 4096u ? 512u : 256u);
    if (per_cu < 256u) per_cu = 256u;
    uint64_t lanes = (uint64_t)cus * per_cu;
    const uint64_t fit = (4ull << 30) / slot;
    if (fit < lanes) lanes = fit;
    lanes = lanes / 256u * 256u;
    if (lanes < 256u) lanes = 256u;
    kp.ev_lanes = lanes;
  }
  hipError_t e = hipMalloc(&pl->d_init_x, cfg->N);
  if (e == hipSuccess) e = hipMemcpy(pl->d_init_x, ix.data(), cfg->N, hipMemcpyHostToDevice);
  if (e == hipSuccess && !stops.empty()) {         // one wave per trial: the sorted /stop schedule
    e = hipMalloc(&pl->d_stops, sizeof(uint64_t) * stops.size());
    if (e == hipSuccess)
      e = hipMemcpy(pl->d_stops, stops.data(), sizeof(uint64_t) * stops.size(), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess && !wave && cfg->crash_at) {   // one lane per trial: crash_at as it is
    e = hipMalloc(&pl->d_crash, sizeof(uint32_t) * cfg->N);
    if (e == hipSuccess) e = hipMemcpy(pl->d_crash, cfg->crash_at, sizeof(uint32_t) * cfg->N, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipMalloc(&pl->d_scratch, kp.ev_lanes * slot);
  if (e != hipSuccess) return hip_fail(e, "event-mode scratch");
  kp.init_x = pl->d_init_x;
  kp.ev_stops = pl->d_stops;
  kp.ev_nstops = (uint32_t)stops.size();
  kp.crash_at = pl->d_crash;
  kp.scratch = pl->d_scratch;
  return BO_OK;
}

// The count-level plans of one table: the two- and three-valued modes, the Byzantine family with its additions,
// and the adversarial scheduler, which has the honest plane and no table.
static int upload_count_level(bo_plan *pl, const PlanTables &tables) {
  benor::KParams &kp = pl->kp;
  const uint32_t m = kp.m;
  if (benor::variant_sched(kp.variant)) {
    // An adversarial scheduler: the honest plane alone -- the scheduler's counts are a closed form
    TableUpload up;
    const size_t o_plane = up.add(tables.honest.data(), sizeof(uint64_t) * tables.honest.size());
    const hipError_t e = up.upload(&pl->d_tally);
    if (e != hipSuccess) return hip_fail(e, "honest plane upload");
    kp.byz_plane = reinterpret_cast<const unsigned long long *>(pl->d_tally + o_plane);
    return BO_OK;
  }
  // The two- and three-valued modes and the Byzantine family: the whole table HG(m, K, q), K = 0..m: at most
  // ~3.7 * 10^6 thresholds (30 MB) at m = 4096
  std::vector<uint32_t> off(m + 2u, 0u);
  std::vector<uint64_t> thr;
  std::vector<double> w;
  for (uint32_t K = 0; K <= m; ++K) {
    off[K] = (uint32_t)thr.size();
    (void)tally_row(m, kp.q, K, thr, w);
  }
  off[m + 1u] = (uint32_t)thr.size();
  // ... and, with Byzantine senders, the Binomial thresholds and the honest plane behind it
  const bool byz = benor::variant_byz(kp.variant);
  std::vector<uint64_t> lie;
  if (byz && !benor::byz_heard(kp)) byz_row(kp.byz_n, kp.byz_one, lie);   // (BALANCE, SPLIT, b = 0: no thresholds)
  TableUpload up;
  const size_t o_off = up.add(off.data(), sizeof(uint32_t) * off.size());
  const size_t o_thr = up.add(thr.data(), sizeof(uint64_t) * thr.size(), sizeof(uint64_t));
  const size_t o_lie = up.add(lie.data(), sizeof(uint64_t) * lie.size());
  const size_t o_plane = up.add(tables.honest.data(), byz ? sizeof(uint64_t) * tables.honest.size() : 0u);
  const hipError_t e = up.upload(&pl->d_tally);
  if (e != hipSuccess) return hip_fail(e, "tally table upload");
  kp.tally_off = reinterpret_cast<const uint32_t *>(pl->d_tally + o_off);
  kp.tally_thr = reinterpret_cast<const unsigned long long *>(pl->d_tally + o_thr);
  if (byz) {
    if (!lie.empty()) kp.byz_thr = reinterpret_cast<const unsigned long long *>(pl->d_tally + o_lie);
    kp.byz_plane = reinterpret_cast<const unsigned long long *>(pl->d_tally + o_plane);
  }
  return BO_OK;
}

// The crash family: one table per reachable live count (pool size), and their directory
static int upload_crash(bo_plan *pl, const PlanTables &tables) {
  benor::KParams &kp = pl->kp;
  const CrashSchedule &crash = tables.crash;
  std::vector<benor::CrashDir> dir(kp.cr_n + 1u);
  std::vector<uint32_t> off;
  std::vector<uint64_t> thr;
  std::vector<double> w;
  for (uint32_t d = 0; d <= kp.cr_n; ++d) {
    if (!crash.reach[d]) {       // never read: the entry of the next larger live count (d = 0 is reachable)
      dir[d] = dir[d - 1u];
      continue;
    }
    const uint32_t md = kp.m - d;
    dir[d].thr_base = thr.size();
    dir[d].off_base = (uint32_t)off.size();
    dir[d].pad = 0u;
    const size_t base = thr.size();
    for (uint32_t K = 0; K <= md; ++K) {
      off.push_back((uint32_t)(thr.size() - base));
      (void)tally_row(md, kp.q, K, thr, w);
    }
    off.push_back((uint32_t)(thr.size() - base));   // the md + 2nd offset: the last row's end
  }
  TableUpload up;
  const size_t o_dir = up.add(dir.data(), sizeof(benor::CrashDir) * dir.size());
  const size_t o_off = up.add(off.data(), sizeof(uint32_t) * off.size());
  const size_t o_list = up.add(crash.list.data(), sizeof(uint32_t) * crash.list.size());
  const size_t o_thr = up.add(thr.data(), sizeof(uint64_t) * thr.size(), sizeof(uint64_t));
  const hipError_t e = up.upload(&pl->d_tally);
  if (e != hipSuccess) return hip_fail(e, "crash tally table upload");
  kp.cr_dir = reinterpret_cast<const benor::CrashDir *>(pl->d_tally + o_dir);
  kp.tally_off = reinterpret_cast<const uint32_t *>(pl->d_tally + o_off);
  kp.cr_list = crash.list.empty() ? nullptr : reinterpret_cast<const uint32_t *>(pl->d_tally + o_list);
  kp.tally_thr = reinterpret_cast<const unsigned long long *>(pl->d_tally + o_thr);
  return BO_OK;
}

// `rule`: NULL, or the threshold rule that replaces the plan's own (checked by check_rule_base).
static int plan_create_impl(const bo_trials_cfg *cfg, bo_plan **out, bool live_run, const bo_rule *rule = nullptr) {
  if (!cfg || !out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  *out = nullptr;
  std::vector<uint32_t> live;
  std::vector<uint4> plane;
  benor::KParams kp0;
  PlanTables tables;
  int rc = plan_host(cfg, live, plane, kp0, live_run, &tables);
  if (rc) return rc;
  if (rule) kp0.rule_on = 1u, kp0.rule = *rule;     // (the variant, the geometry and the tables are the base plan's)
  int dev = 0;
  rc = check_device(&dev);
  if (rc) return rc;

  auto pl = std::make_unique<bo_plan>();            // an error return below frees what was allocated so far
  pl->cfg = *cfg;
  pl->cfg.faulty = nullptr;
  pl->cfg.init = nullptr;
  pl->cfg.crash_at = nullptr;
  pl->device = dev;
  pl->live_ids = live;
  pl->kp = kp0;
  benor::KParams &kp = pl->kp;
  const uint32_t m = kp.m;
  hipError_t e = hipMalloc(&pl->d_flag, sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemset(pl->d_flag, 0, sizeof(uint32_t));
  if (e != hipSuccess) return hip_fail(e, "plan flag");
  if (benor::mfma_sure_batch(kp.variant, kp.G, kp.W, false)) {   // (the plan-level form: a plan has no node_out)
    // benor.h orders a plan's launches on one stream, and every launch leaves
    // the words 0 (benor_mfma_sched.h): one pair per plan, zeroed once
    e = hipMalloc(&pl->d_claim, sizeof(uint32_t) * benor::sched::kWords);
    if (e == hipSuccess) e = hipMemset(pl->d_claim, 0, sizeof(uint32_t) * benor::sched::kWords);
    if (e != hipSuccess) return hip_fail(e, "plan claim words");
    kp.mfma_claim = pl->d_claim;
  }
  if (m > 0) {
    e = hipMalloc(&pl->d_live, sizeof(uint32_t) * m);
    if (e == hipSuccess) e = hipMalloc(&pl->d_init, sizeof(uint4) * kp.W);
    if (e == hipSuccess) e = hipMemcpy(pl->d_live, pl->live_ids.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(pl->d_init, plane.data(), sizeof(uint4) * kp.W, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "plan upload");
    kp.live_ids = pl->d_live;
    kp.init_plane = pl->d_init;
    if (cfg->mode == BO_MODE_EVENT) rc = upload_event(pl.get(), cfg, live_run);
    else if (benor::variant_crash(kp.variant)) rc = upload_crash(pl.get(), tables);
    else if (benor::variant_count_level(kp.variant)) rc = upload_count_level(pl.get(), tables);
    if (rc) return rc;
  }
  *out = pl.release();
  return BO_OK;
}

int bo_plan_create(const bo_trials_cfg *cfg, bo_plan **out) { return plan_create_impl(cfg, out, false); }

int bo_plan_create_rule(const bo_trials_cfg *cfg, const bo_rule *rule, bo_plan **out) {
  if (!out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  *out = nullptr;
  const int rc = check_rule_base(cfg, rule);
  return rc ? rc : plan_create_impl(cfg, out, false, rule);
}

int bo_plan_rule(const bo_plan *pl, bo_rule *out) {
  if (!pl) return -BO_ERR_INVALID_ARGUMENT;
  if (!pl->kp.rule_on) return 0;
  if (out) *out = pl->kp.rule;
  return 1;
}

void bo_plan_destroy(bo_plan *pl) { delete pl; }

uint32_t bo_plan_live_nodes(const bo_plan *pl) { return pl ? pl->kp.m : 0u; }

int bo_plan_kernel(const bo_plan *pl) {
  if (!pl) return -BO_ERR_INVALID_ARGUMENT;
  return kernel_family(pl->kp);
}

// Tests and diagnosis: what the plan's random-delivery kernel draws for one (trial, round, phase), read out by a
// kernel that calls the trial kernel's own device function with the plan's own parameters (benor_internal.h
// launch_delivery_masks).  Synchronous, on the null stream; no histogram, no flag.
int bo_plan_delivery_masks(bo_plan *pl, uint64_t trial, uint32_t round, uint32_t phase, uint64_t *masks_out) {
  if (!pl || !masks_out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  if (pl->kp.m == 0u || pl->kp.variant != benor::kVarRandom)
    return fail(BO_ERR_INVALID_ARGUMENT, "bo_plan_delivery_masks: the plan's kernel is not BO_KERNEL_RANDOM");
  if (phase > 1u || round == 0u || round > 0x7FFFu)
    return fail(BO_ERR_INVALID_ARGUMENT, "bo_plan_delivery_masks: phase is 0 or 1 and round 1 .. 0x7FFF");
  benor::KParams kp = pl->kp;
  kp.trial_begin = trial;
  kp.trial_count = 1;
  const size_t words = (size_t)kp.m * kp.W;
  int cur = 0;
  HIP_TRY(hipGetDevice(&cur));
  if (cur != pl->device) HIP_TRY(hipSetDevice(pl->device));
  hipError_t e;
  {
    DeviceBuf<unsigned long long> d;
    e = d.alloc(words);
    if (e == hipSuccess) e = hipMemset(d.d, 0, sizeof(unsigned long long) * words);
    if (e == hipSuccess) e = benor::launch_delivery_masks(kp, round, phase, d.d, nullptr);
    if (e == hipSuccess) e = hipMemcpy(masks_out, d.d, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost);
  }
  if (cur != pl->device) (void)hipSetDevice(cur);
  if (e != hipSuccess) return hip_fail(e, "bo_plan_delivery_masks");
  return BO_OK;
}

// Lockstep: the R-phase needs c1 only (c0 = M - c1, M binary votes,
// node.ts:52,56-62).  The P-phase needs c0 and c1 (node.ts:92-98) unless M
// is odd: then no R-phase count can tie, no proposal is "?" (node.ts:63-69),
// and c0 = m - c1.  So 2 counts of ceil(m/32) words for odd M (the bench's
// m = 683), 3 for even M (round-1 parity: M = m - init_q).  Random delivery
// counts both values in both phases: 4 (the count-level modes answer the same
// unit: the work they stand in for).
uint64_t bo_plan_popc_words_per_node_round(const bo_plan *pl) {
  if (!pl) return 0;
  const bool random = mode_traits(pl->kp.mode)->is(benor::kModeRandom);
  const uint64_t counts = random ? 4ull : ((pl->kp.m - pl->kp.init_q) & 1u) ? 2ull : 3ull;
  return counts * ((pl->kp.m + 31ull) / 32ull);
}

// Diagnostics (BENOR_TIMELINE=<file>): the packed matrix-core kernel stamps
// each wave's phases, the KIND 0 matrix-core kernel each wave's entry and last
// group, with its group count and its XCC, SE and CU ids (kernel=mfma in the
// header line); one CSV line per wave is appended to the file
// (tools/timeline_report.py).  Synchronous; not for timing the launch itself.
static hipError_t launch_with_timeline(benor::KParams kp, int grid, hipStream_t s, const char *path) {
  const size_t words = (size_t)grid * benor::kWavesPerBlock * benor::kTimelineWords;
  DeviceBuf<unsigned long long> d;
  hipError_t e = d.alloc(words);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(d.d, 0, words * sizeof(unsigned long long), s);
  kp.timeline = d.d;
  if (e == hipSuccess) e = benor::launch_lockstep(kp, grid, s);
  std::vector<unsigned long long> h(words);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipMemcpy(h.data(), d.d, words * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  if (FILE *f = std::fopen(path, "a")) {
    std::fprintf(f, "# launch m=%u trials=%llu grid=%d waves=%d", kp.m, (unsigned long long)kp.trial_count, grid,
                 grid * benor::kWavesPerBlock);
    if (kp.variant == benor::kVarMfma) std::fprintf(f, " kernel=mfma chunk=%u strip=%d", kp.mfma_chunk, benor::mfma_strip_form(kp) ? 1 : 0);
    std::fprintf(f, "\n");
    for (size_t w = 0; w < (size_t)grid * benor::kWavesPerBlock; ++w) {
      const unsigned long long *t = h.data() + w * benor::kTimelineWords;
      std::fprintf(f, "%zu", w);
      for (uint32_t i = 0; i < 11u; ++i) std::fprintf(f, ",%llu", t[i]);
      std::fprintf(f, "\n");
    }
    std::fclose(f);
  }
  return hipSuccess;
}

static int plan_launch_impl(bo_plan *pl, uint64_t trial_begin, uint64_t trial_count, uint64_t *hist_dev,
                            bo_node_state *node_out, uint32_t *rounds_out, hipStream_t s) {
  if (trial_count == 0) return BO_OK;
  benor::KParams kp = pl->kp;
  if (kp.m == 0) {   // no live node: every trial lands in bin (0, 2)
    hipLaunchKernelGGL(add_bin_kernel, dim3(1), dim3(64), 0, s,
                       reinterpret_cast<unsigned long long *>(hist_dev), 2u, (unsigned long long)trial_count);
    HIP_TRY(hipGetLastError());
    return BO_OK;
  }
  kp.hist = reinterpret_cast<unsigned long long *>(hist_dev);
  kp.overflow = pl->d_flag;
  kp.node_out = node_out;
  kp.rounds_out = rounds_out;
  if (benor::mfma_defers(kp)) {
    // Matrix-core round 1 with deferral (benor_mfma.h, KIND > 0): per chunk of
    // at most kDeferChunk trials, the matrix-core launch records the trials
    // that do not halt in round 1, and the W kernel runs exactly those from
    // round 1 (trial-list mode; the list length is read on the device, so
    // the two launches queue back to back with no host sync).
    const uint64_t cap = std::min<uint64_t>(trial_count, benor::kDeferChunk);
    kp.trial_count = cap;
    const int grid = benor::lockstep_grid(kp, pl->device);
    // Continuation passes: a trial that tied in round 1 starts round 2 from its
    // round-1 coins, so the matrix cores run rounds 2 .. kMfmaContRounds of the
    // deferred trials too, each pass deferring its own ties; whatever is left
    // goes to the popcount kernel, which re-runs it from round 1.
    const uint32_t last_round = std::min<uint32_t>(benor::kMfmaContRounds, kp.k_max - 1u);
    // A pass's list holds the previous round's ties only: in lockstep every
    // receiver hears the whole x plane, so a round without an R-phase tie
    // makes every receiver propose and then decide the majority (m > F, KIND 1
    // and 2 alike), and random starts tie with q(m) <= 10 % at m > 64.  So pass
    // r runs on grid >> 2(r - 1) workgroups: a full-size grid gives most waves
    // a single group, and every workgroup that works pays its serialised
    // deferral atomic and histogram flush (~12 ns each; N=256 F=0:
    // round 2 took 31 us for ~5 us of products).  The cooperative form's grid
    // is already one workgroup per group.
    const bool shrink = !benor::mfma_big_coop(kp);
    auto pass_grid = [&](uint32_t r) {
      if (!shrink || r < 2u) return grid;
      const int g = grid >> (2u * (r - 1u));
      return std::max(g, std::min(grid, 64));
    };
    // Deferral segments: a launch of u owners (waves, or workgroups of the
    // cooperative form) gives each at most ceil(groups / u) 32-trial groups,
    // so its segments hold that many trials each; the region is sized for the
    // largest u * cap over the chunk's launches (the per-launch cap is passed
    // in KParams::defer_seg_cap).
    const uint64_t groups = (cap + 31u) / 32u;
    auto seg_cap_of = [&](uint64_t units) { return (groups + units - 1u) / units * 32u; };
    uint64_t seg_words = 0;
    for (uint32_t r = 1u; r <= std::max<uint32_t>(last_round, 1u); ++r) {
      benor::KParams kr = kp;
      kr.cont_round = r >= 2u ? r : 0u;
      const uint64_t u = benor::defer_units(kr, pass_grid(r));
      seg_words = std::max<uint64_t>(seg_words, u * seg_cap_of(u));
    }
    const uint64_t words = 2u * cap + 64u + seg_words;                  // two lists, three lengths, segments
    // Test knob: a smaller segment capacity than the sizing rule's, so that a
    // GPU test can see the overflow reported (tests/test_mfma.py).
    const uint32_t test_seg_cap = benor::knob_u32("BENOR_TEST_DEFER_SEG_CAP", 0u);
    if (pl->defer_words < words) {
      if (pl->d_defer) (void)hipFree(pl->d_defer);
      pl->d_defer = nullptr;
      pl->defer_words = 0;
      HIP_TRY(hipMalloc(&pl->d_defer, sizeof(uint32_t) * words));
      pl->defer_words = words;
    }
    uint32_t *const lens = pl->d_defer + cap;                           // pass r's output length: lens[16 (r - 1)]
    uint32_t *const segs = lens + 64u;
    uint32_t *const lists[2] = {pl->d_defer, segs + seg_words};         // pass r writes lists[(r - 1) & 1]
    for (uint64_t done = 0; done < trial_count;) {
      const uint64_t n = std::min<uint64_t>(trial_count - done, cap);
      HIP_TRY(hipMemsetAsync(lens, 0, sizeof(uint32_t) * 16u * std::max<uint32_t>(last_round, 1u), s));   // every pass's length
      kp.trial_begin = trial_begin + done;
      kp.trial_count = n;
      kp.defer_seg = segs;
      uint32_t r_last = 1u;
      for (uint32_t r = 1u; r <= std::max<uint32_t>(last_round, 1u); ++r) {
        benor::KParams kc = kp;
        const int g = pass_grid(r);
        kc.cont_round = r >= 2u ? r : 0u;
        if (r >= 2u) {
          kc.trial_list = lists[(r - 2u) & 1u];
          kc.trial_list_len = lens + 16u * (r - 2u);
        }
        kc.defer_list = lists[(r - 1u) & 1u];
        kc.defer_len = lens + 16u * (r - 1u);
        kc.defer_seg_cap = (uint32_t)seg_cap_of(benor::defer_units(kc, g));
        if (test_seg_cap) kc.defer_seg_cap = std::min<uint32_t>(kc.defer_seg_cap, test_seg_cap);
        HIP_TRY(benor::launch_lockstep(kc, g, s));
        r_last = r;
      }
      benor::KParams kw = benor::base_kernel(kp);   // W kernel (W <= 32) or blocked kernel
      kw.defer_list = kw.defer_len = kw.defer_seg = nullptr;
      kw.trial_list = lists[(r_last - 1u) & 1u];
      kw.trial_list_len = lens + 16u * (r_last - 1u);
      HIP_TRY(benor::launch_lockstep(kw, benor::lockstep_grid(kw, pl->device), s));
      done += n;
    }
    return BO_OK;
  }
  // Launches of at most 2^31 trials: the kernels index trials within a launch in 32 bits.
  for (uint64_t done = 0; done < trial_count;) {
    const uint64_t n = std::min<uint64_t>(trial_count - done, benor::kMaxTrialsPerLaunch);
    kp.trial_begin = trial_begin + done;
    kp.trial_count = n;
    kp.mfma_chunk = benor::mfma_chunk(kp, pl->device);   // KIND 0 matrix-core launch: static (0) or dynamic
    const int grid = benor::lockstep_grid(kp, pl->device);
    const bool stamps = kp.variant == benor::kVarMfmaSmall || benor::mfma_sure_batch(kp);
    const char *tl_path = stamps ? benor::knob("BENOR_TIMELINE") : nullptr;
    if (tl_path) {
      HIP_TRY(launch_with_timeline(kp, grid, s, tl_path));
    } else {
      HIP_TRY(benor::launch_lockstep(kp, grid, s));
    }
    done += n;
  }
  return BO_OK;
}

int bo_plan_launch(bo_plan *pl, uint64_t trial_begin, uint64_t trial_count, uint64_t *hist_dev, void *stream) {
  if (!pl || !hist_dev) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  return plan_launch_impl(pl, trial_begin, trial_count, hist_dev, nullptr, nullptr,
                          reinterpret_cast<hipStream_t>(stream));
}

namespace {
int plan_flag_read(bo_plan *pl, hipStream_t s, uint32_t &v);
int plan_flag_error(uint32_t v);
}  // namespace

int bo_plan_run(bo_plan *pl, uint64_t trial_begin, uint64_t trial_count, uint64_t *hist_host) {
  if (!pl || !hist_host) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  const uint32_t H = bo_hist_len(pl->cfg.k_max);
  DeviceBuf<uint64_t> d;
  hipError_t e = d.alloc(H);
  if (e != hipSuccess) return hip_fail(e, "hipMalloc(&d, sizeof(uint64_t) * H)");
  e = hipMemset(d.d, 0, sizeof(uint64_t) * H);
  int rc = BO_OK;
  if (e == hipSuccess) rc = plan_launch_impl(pl, trial_begin, trial_count, d.d, nullptr, nullptr, nullptr);
  std::vector<uint64_t> h(H);
  if (e == hipSuccess && rc == BO_OK) e = hipMemcpy(h.data(), d.d, sizeof(uint64_t) * H, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(e, "bo_plan_run");
  if (rc) return rc;
  uint32_t flag = 0;
  rc = plan_flag_read(pl, nullptr, flag);   // the launches went to the null stream
  if (!rc) rc = plan_flag_error(flag);
  if (rc) return rc;
  for (uint32_t i = 0; i < H; ++i) hist_host[i] += h[i];
  return BO_OK;
}

namespace {
// The plan's invariant flag, read with a copy ordered on `s` (the stream its
// launches went to) on the plan's device: waits for that stream only, not for
// other plans', torch's or a live run's work (bo_plan_run, bo_consensus_wait).
// Cleared when set.
int plan_flag_read(bo_plan *pl, hipStream_t s, uint32_t &v) {
  v = 0;
  if (!pl->d_flag) return BO_OK;
  int cur = 0;
  HIP_TRY(hipGetDevice(&cur));
  if (cur != pl->device) HIP_TRY(hipSetDevice(pl->device));
  hipError_t e = hipMemcpyAsync(&v, pl->d_flag, sizeof v, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess && v) e = hipMemsetAsync(pl->d_flag, 0, sizeof v, s);
  if (e == hipSuccess && v) e = hipStreamSynchronize(s);
  if (cur != pl->device) (void)hipSetDevice(cur);
  if (e != hipSuccess) return hip_fail(e, "plan flag read");
  return BO_OK;
}

int plan_flag_error(uint32_t v) {
  if (!v) return BO_OK;
  if (v & 1u)
    return fail(BO_ERR_INTERNAL, "a matrix-core launch deferred more trials than its segment holds: "
                                 "its histogram is incomplete (deferral segment sizing)");
  if (v & benor::sched::kInvariantBit)
    return fail(BO_ERR_INTERNAL, "a matrix-core launch ended with its claim counter off: "
                                 "groups were skipped or run twice (benor_mfma_sched.h)");
  return fail(BO_ERR_INTERNAL, "an event-level message pool filled up: the affected trials stopped early");
}
}  // namespace

// Standalone check after bo_plan_launch on streams the library does not know:
// the whole plan device is synchronised first.
int bo_plan_check(bo_plan *pl) {
  if (!pl) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  if (!pl->d_flag) return BO_OK;
  int cur = 0;
  HIP_TRY(hipGetDevice(&cur));
  if (cur != pl->device) HIP_TRY(hipSetDevice(pl->device));
  const hipError_t e = hipDeviceSynchronize();
  if (cur != pl->device) (void)hipSetDevice(cur);
  if (e != hipSuccess) return hip_fail(e, "bo_plan_check");
  uint32_t v = 0;
  const int rc = plan_flag_read(pl, nullptr, v);
  return rc ? rc : plan_flag_error(v);
}

int bo_run_trials(const bo_trials_cfg *cfg, uint64_t trial_begin, uint64_t trial_count, uint64_t *hist_host) {
  bo_plan *pl = nullptr;
  int rc = bo_plan_create(cfg, &pl);
  if (rc) return rc;
  rc = bo_plan_run(pl, trial_begin, trial_count, hist_host);
  bo_plan_destroy(pl);
  return rc;
}

// One trial with per-node state in lockstep mode (the network API's
// /start, consensus.ts:3-8): every device operand -- live ids, initial planes,
// node states, histogram, round count -- goes into one per-thread device buffer
// that persists between calls, with one upload and one read-back.  A network of
// the reference's size is then a few tens of microseconds, not the ten
// allocations and frees of a plan.
namespace {
struct StateScratch {
  int device = -1;
  size_t bytes = 0;
  unsigned char *d = nullptr;
  std::vector<unsigned char> h;
  // no destructor: freeing device memory while the process exits can race the
  // HIP runtime's own teardown; the buffer is a few KB and the process owns it
};
thread_local StateScratch t_scratch;

// Host-side initial states (node.ts:21-26) of a validated configuration, N entries; live entries are
// overwritten by the kernel.
void initial_states(const bo_trials_cfg *cfg, bo_node_state *st) {
  // (the Byzantine family: a Byzantine node is alive and has no protocol state; no kernel writes its entry)
  const bool byz_mode = mode_traits(cfg->mode)->is(benor::kModeByz);
  for (uint32_t i = 0; i < cfg->N; ++i) {
    const bool f = cfg->faulty[i] != 0;
    const bool byz = byz_mode && cfg->faulty[i] == 2u;
    st[i].killed = f && !byz ? 1 : 0;
    st[i].x = f ? -1 : (cfg->init_mode == BO_INIT_FIXED ? cfg->init[i] : -1);
    st[i].decided = f ? -1 : 0;
    st[i].pad = 0;
    st[i].k = f ? -1 : 0;
  }
}

int run_states_lockstep(const bo_trials_cfg *cfg, uint64_t trial, bo_node_state *nodes_out, uint32_t *rounds_out) {
  std::vector<uint32_t> live;
  std::vector<uint4> plane;
  benor::KParams kp;
  int rc = plan_host(cfg, live, plane, kp);
  if (rc) return rc;
  int dev = 0;
  rc = check_device(&dev);
  if (rc) return rc;
  const uint32_t N = cfg->N, H = bo_hist_len(cfg->k_max), m = kp.m;
  // layout: states [N] | hist [H] u64 | rounds u32 (+pad) | live [m] u32 | init [W] uint4
  const size_t o_st = 0, o_h = (sizeof(bo_node_state) * N + 15u) & ~size_t(15);
  const size_t o_r = o_h + sizeof(uint64_t) * H, o_live = (o_r + 16u + 15u) & ~size_t(15);
  const size_t o_init = (o_live + sizeof(uint32_t) * m + 15u) & ~size_t(15);
  const size_t bytes = o_init + sizeof(uint4) * plane.size();
  StateScratch &sc = t_scratch;
  if (sc.device != dev || sc.bytes < bytes) {
    if (sc.d) (void)hipFree(sc.d);
    sc.d = nullptr;
    sc.bytes = 0;
    HIP_TRY(hipMalloc(&sc.d, bytes));
    sc.bytes = bytes;
    sc.device = dev;
  }
  sc.h.assign(bytes, 0);
  initial_states(cfg, reinterpret_cast<bo_node_state *>(sc.h.data() + o_st));
  if (m) std::memcpy(sc.h.data() + o_live, live.data(), sizeof(uint32_t) * m);
  if (!plane.empty()) std::memcpy(sc.h.data() + o_init, plane.data(), sizeof(uint4) * plane.size());
  HIP_TRY(hipMemcpy(sc.d, sc.h.data(), bytes, hipMemcpyHostToDevice));
  bo_plan pl;                      // on the stack: its device tables are views into the scratch buffer
  pl.kp = kp;
  pl.cfg = *cfg;
  pl.device = dev;
  pl.live_ids = live;
  pl.kp.live_ids = reinterpret_cast<uint32_t *>(sc.d + o_live);
  pl.kp.init_plane = reinterpret_cast<uint4 *>(sc.d + o_init);
  rc = plan_launch_impl(&pl, trial, 1, reinterpret_cast<uint64_t *>(sc.d + o_h),
                        reinterpret_cast<bo_node_state *>(sc.d + o_st), reinterpret_cast<uint32_t *>(sc.d + o_r),
                        nullptr);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(sc.h.data(), sc.d, o_r + sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::memcpy(nodes_out, sc.h.data() + o_st, sizeof(bo_node_state) * N);
  if (rounds_out) std::memcpy(rounds_out, sc.h.data() + o_r, sizeof(uint32_t));
  return BO_OK;
}
}  // namespace

// One trial's per-node states through a plan of its own; `rule`: NULL, or the threshold rule that replaces the plan's.
static int run_states_plan(const bo_trials_cfg *cfg, const bo_rule *rule, uint64_t trial, bo_node_state *nodes_out,
                           uint32_t *rounds_out) {
  bo_plan *created = nullptr;
  int rc = plan_create_impl(cfg, &created, false, rule);
  if (rc) return rc;
  const std::unique_ptr<bo_plan> pl(created);
  const uint32_t N = cfg->N, H = bo_hist_len(cfg->k_max);
  std::vector<bo_node_state> st(N);
  initial_states(cfg, st.data());
  DeviceBuf<bo_node_state> d_st;
  DeviceBuf<uint64_t> d_h;
  DeviceBuf<uint32_t> d_r;
  hipError_t e = d_st.alloc(N);
  if (e == hipSuccess) e = d_h.alloc(H);
  if (e == hipSuccess) e = d_r.alloc(1);
  if (e == hipSuccess) e = hipMemcpy(d_st.d, st.data(), sizeof(bo_node_state) * N, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_h.d, 0, sizeof(uint64_t) * H);
  if (e == hipSuccess) e = hipMemset(d_r.d, 0, sizeof(uint32_t));
  if (e == hipSuccess) rc = plan_launch_impl(pl.get(), trial, 1, d_h.d, d_st.d, d_r.d, nullptr);
  uint32_t rounds = 0;
  if (e == hipSuccess && rc == BO_OK) e = hipMemcpy(nodes_out, d_st.d, sizeof(bo_node_state) * N, hipMemcpyDeviceToHost);
  if (e == hipSuccess && rc == BO_OK) e = hipMemcpy(&rounds, d_r.d, sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(e, "bo_run_trial_states");
  if (rc) return rc;
  if (rounds & 0x80000000u) return fail(BO_ERR_INTERNAL, "event-level message pool filled up: the run stopped early");
  if (rounds_out) *rounds_out = rounds;
  return BO_OK;
}

int bo_run_trial_states(const bo_trials_cfg *cfg, uint64_t trial, bo_node_state *nodes_out, uint32_t *rounds_out) {
  if (!cfg || !nodes_out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  if (cfg->mode == BO_MODE_LOCKSTEP) return run_states_lockstep(cfg, trial, nodes_out, rounds_out);
  return run_states_plan(cfg, nullptr, trial, nodes_out, rounds_out);
}

int bo_run_trial_states_rule(const bo_trials_cfg *cfg, const bo_rule *rule, uint64_t trial, bo_node_state *nodes_out,
                             uint32_t n) {
  if (!nodes_out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  const int rc = check_rule_base(cfg, rule);
  if (rc) return rc;
  if (n < cfg->N) return fail(BO_ERR_INVALID_ARGUMENT, "bo_run_trial_states_rule: nodes_out holds fewer than N entries");
  return run_states_plan(cfg, rule, trial, nodes_out, nullptr);
}

// ------------------------------------------------------------ live runs
namespace {
void slot_destroy(LiveSlot *sl) {
  if (sl->d) (void)hipFree(sl->d);
  if (sl->hp) (void)hipHostFree(sl->hp);
  if (sl->box) (void)hipHostFree(sl->box);
  if (sl->s) (void)hipStreamDestroy(sl->s);
  delete sl;
}

LiveSlot *slot_acquire(int dev) {
  {
    std::lock_guard<std::mutex> g(g_slots_mu);
    for (size_t i = 0; i < g_free_slots.size(); ++i)
      if (g_free_slots[i]->device == dev) {
        LiveSlot *sl = g_free_slots[i];
        g_free_slots.erase(g_free_slots.begin() + (long)i);
        return sl;
      }
  }
  auto *sl = new LiveSlot();
  sl->device = dev;
  const size_t box_bytes = sizeof(uint32_t) * benor::kLiveBoxWords;
  if (hipStreamCreateWithFlags(&sl->s, hipStreamNonBlocking) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void **>(&sl->box), box_bytes, hipHostMallocMapped | hipHostMallocCoherent) !=
          hipSuccess ||
      hipHostGetDevicePointer(reinterpret_cast<void **>(&sl->dbox), sl->box, 0) != hipSuccess) {
    slot_destroy(sl);
    return nullptr;
  }
  return sl;
}

// Back to the pool after its run ended (the stream is idle): a large buffer is
// freed rather than kept (k concurrent N = 4096 runs kept k
// message pools of 268 MB for the life of the process).
void slot_release(LiveSlot *sl) {
  if (!sl) return;
  if (sl->bytes > kSlotKeepBytes) {
    (void)hipFree(sl->d);
    sl->d = nullptr;
    sl->bytes = 0;
  }
  std::lock_guard<std::mutex> g(g_slots_mu);
  g_free_slots.push_back(sl);
}

size_t align_up(size_t v, size_t a) { return (v + a - 1u) & ~(a - 1u); }

// One trial of a network on the workgroup-batched event kernel
// (benor_event_live.hip), on the slot's stream: the plan (host), the slot's
// buffer -- flag | states [N] | hist [H] | rounds | live ids [m] | init x [N]
// | stop schedule | message pool (HBM form only) -- one upload and the launch.
// `live`: the kernel polls the slot's mailbox for GET /stop and /getState.
int wg_launch(LiveSlot *sl, const bo_trials_cfg *cfg, bool live, WgRun &run) {
  std::vector<uint32_t> ids;
  std::vector<uint4> plane;
  benor::KParams kp;
  int rc = plan_host(cfg, ids, plane, kp, true);
  if (rc) return rc;
  const uint32_t N = cfg->N, H = bo_hist_len(cfg->k_max), m = kp.m;
  std::vector<uint64_t> stops;
  if (cfg->crash_at)
    for (uint32_t i = 0; i < N; ++i)
      if (cfg->crash_at[i] != 0xFFFFFFFFu) stops.push_back(((uint64_t)cfg->crash_at[i] << 12) | i);
  std::sort(stops.begin(), stops.end());
  const size_t o_st = 16u, o_h = align_up(o_st + sizeof(bo_node_state) * N, 16u);
  const size_t o_r = o_h + sizeof(uint64_t) * H, o_stats = align_up(o_r + 4u, 16u);
  const size_t o_live = o_stats + 24u * sizeof(uint64_t);
  const size_t o_ix = align_up(o_live + sizeof(uint32_t) * m, 16u);
  const size_t o_stops = align_up(o_ix + N, 16u);
  const size_t o_pool = align_up(o_stops + sizeof(uint64_t) * stops.size(), 256u);
  const size_t bytes = o_pool + (benor::event_wg_lds_pool(kp) ? 0u : (size_t)kp.ev_cap * 4u);
  if (sl->bytes < bytes) {
    if (sl->d) (void)hipFree(sl->d);
    sl->d = nullptr;
    sl->bytes = 0;
    HIP_TRY(hipMalloc(&sl->d, bytes));
    sl->bytes = bytes;
  }
  if (sl->hp_bytes < o_pool) {                  // (the slot's stream is idle: its last run ended)
    if (sl->hp) (void)hipHostFree(sl->hp);
    sl->hp = nullptr;
    sl->hp_bytes = 0;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sl->hp), o_pool, hipHostMallocDefault));
    sl->hp_bytes = o_pool;
  }
  unsigned char *const h = sl->hp;
  std::memset(h, 0, o_pool);
  initial_states(cfg, reinterpret_cast<bo_node_state *>(h + o_st));
  if (m) std::memcpy(h + o_live, ids.data(), sizeof(uint32_t) * m);
  std::memcpy(h + o_ix, cfg->init, N);
  if (!stops.empty()) std::memcpy(h + o_stops, stops.data(), sizeof(uint64_t) * stops.size());
  if (live) {
    // the mailbox: no request, no stop landed, no snapshot asked (the slot's
    // previous kernel has ended)
    std::memset(sl->box, 0, sizeof(uint32_t) * benor::kLiveEv);
    for (uint32_t i = 0; i < N; ++i) sl->box[benor::kLiveEv + i] = 0xFFFFFFFFu;
    std::memset(sl->box + benor::kSnapReq, 0, sizeof(uint32_t) * (benor::kSnapSt - benor::kSnapReq));
  }
  HIP_TRY(hipMemcpyAsync(sl->d, h, o_pool, hipMemcpyHostToDevice, sl->s));
  kp.hist = reinterpret_cast<unsigned long long *>(sl->d + o_h);
  kp.overflow = reinterpret_cast<uint32_t *>(sl->d);
  kp.node_out = reinterpret_cast<bo_node_state *>(sl->d + o_st);
  kp.rounds_out = reinterpret_cast<uint32_t *>(sl->d + o_r);
  kp.live_ids = reinterpret_cast<uint32_t *>(sl->d + o_live);
  kp.init_x = reinterpret_cast<int8_t *>(sl->d + o_ix);
  kp.ev_stops = reinterpret_cast<uint64_t *>(sl->d + o_stops);
  kp.ev_nstops = (uint32_t)stops.size();
  kp.scratch = reinterpret_cast<uint32_t *>(sl->d + o_pool);
  kp.ev_lanes = 1u;                              // one trial
  kp.live_box = live ? sl->dbox : nullptr;
  kp.ev_stats = benor::knob("BENOR_EVENT_STATS") ? reinterpret_cast<unsigned long long *>(sl->d + o_stats) : nullptr;
  kp.trial_begin = 0;
  kp.trial_count = 1;
  run.o_st = o_st;
  run.o_r = o_r;
  run.o_stats = o_stats;
  run.N = N;
  run.F = cfg->F;
  HIP_TRY(benor::launch_event_wg(kp, 1, sl->s));
  HIP_TRY(hipMemcpyAsync(h, sl->d, o_r + 4u, hipMemcpyDeviceToHost, sl->s));   // read by wg_read
  return BO_OK;
}

// The run's head (flag | states | hist | rounds), read back on the slot's stream.
int wg_read(LiveSlot *sl, const WgRun &run, uint32_t N, std::vector<bo_node_state> &states) {
  if (const char *path = benor::knob("BENOR_EVENT_STATS")) {   // diagnostics: one JSON line per run
    unsigned long long s[24] = {};
    if (hipMemcpyAsync(s, sl->d + run.o_stats, sizeof s, hipMemcpyDeviceToHost, sl->s) == hipSuccess &&
        hipStreamSynchronize(sl->s) == hipSuccess)
      if (FILE *f = std::fopen(path, "a")) {
        static const char *names[23] = {"batches", "events", "batch_slots", "trigger_batches", "conflict_cut",
                                        "cyc_top", "cyc_picks", "cyc_lookup", "cyc_deliver", "cyc_cross",
                                        "cyc_writes_trigger", "cyc_bcast", "cycles", "wall_ticks", "cross_batches",
                                        "snapshots", "ev_work", "ev_wait", "ev_write", "ev_pre", "ev_drain",
                                        "cyc_trigger", "cyc_prepare"};
        std::fprintf(f, "{\"N\": %u, \"F\": %u", run.N, run.F);
        for (int i = 0; i < 23; ++i) std::fprintf(f, ", \"%s\": %llu", names[i], s[i]);
        std::fprintf(f, "}\n");
        std::fclose(f);
      }
  }
  // the head was copied into the pinned buffer behind the kernel (wg_launch)
  const hipError_t e = hipStreamSynchronize(sl->s);
  if (e != hipSuccess) return hip_fail(e, "event-level run");
  const unsigned char *head = sl->hp;
  uint32_t flag = 0, rounds = 0;
  std::memcpy(&flag, head, 4u);
  std::memcpy(&rounds, head + run.o_r, 4u);
  states.resize(N);
  std::memcpy(states.data(), head + run.o_st, sizeof(bo_node_state) * N);
  int rc = plan_flag_error(flag);
  if (!rc && (rounds & 0x80000000u))
    rc = fail(BO_ERR_INTERNAL, "event-level message pool filled up: the run stopped early");
  return rc;
}

// bo_consensus_start_sched with a /stop schedule: one trial on the
// workgroup-batched event kernel, synchronously.
int run_sched_wg(const bo_trials_cfg *cfg, std::vector<bo_node_state> &states) {
  int dev = 0;
  int rc = check_device(&dev);
  if (rc) return rc;
  LiveSlot *sl = slot_acquire(dev);
  if (!sl) return fail(BO_ERR_HIP, "event-level run: stream allocation failed");
  WgRun run;
  rc = wg_launch(sl, cfg, false, run);
  if (!rc) rc = wg_read(sl, run, cfg->N, states);
  if (hipStreamSynchronize(sl->s) == hipSuccess && rc != BO_ERR_HIP) slot_release(sl);
  else slot_destroy(sl);
  return rc;
}

// The end of a live run whose stream reported `e` (hipStreamSynchronize or a
// finished hipStreamQuery): read back, merge the final states, forget the run.
// Idempotent -- the first caller finalizes, later ones get its result.
int live_finalize(bo_network *net, const std::shared_ptr<bo_live> &lr, hipError_t e) {
  std::lock_guard<std::mutex> w(net->wait_mu);
  {
    std::lock_guard<std::mutex> g(net->mu);
    if (net->live != lr) return net->live_rc;
  }
  const uint32_t N = net->N;
  std::vector<bo_node_state> states;
  int rc = e != hipSuccess ? hip_fail(e, "bo_consensus_wait") : wg_read(lr->slot, lr->run, N, states);
  if (rc == BO_ERR_HIP) lr->failed = true;       // the slot's stream is not trusted again
  std::lock_guard<std::mutex> g(net->mu);
  net->live.reset();                             // from here a /stop is ordered after the run
  net->in_flight = false;
  net->live_rc = rc;
  if (!rc) {
    net->stop_events.assign(lr->slot->box + benor::kLiveEv, lr->slot->box + benor::kLiveEv + N);
    merge_states(net, lr->active, states);
  }
  return rc;
}
}  // namespace

bo_live::~bo_live() {
  if (!slot) return;
  if (failed || hipStreamSynchronize(slot->s) != hipSuccess) {
    // a faulted or aborted run: its stream, mailbox and buffer are not reused
    slot_destroy(slot);
  } else {
    slot_release(slot);
  }
}

// startConsensus whose GET /stop requests land while it runs (node.ts:191-194
// served during the round loop): the event-level kernel is launched and the
// call returns, as the reference's GET /start answers before consensus
// finishes (node.ts:167-188).  bo_node_stop / bo_consensus_stop post to the
// running kernel, bo_get_state(s) answer from its snapshots, and
// bo_consensus_wait / bo_consensus_poll end the run.
int bo_consensus_start_live(bo_network *net, uint64_t seed, uint32_t k_max) {
  StartPlan sp;
  int rc = start_prologue(net, k_max, nullptr, 0u, sp);
  if (rc || !sp.launch) return rc;
  const bo_trials_cfg cfg = start_cfg(net, seed, k_max, sp, BO_MODE_EVENT);
  int dev = 0;
  rc = check_device(&dev);
  auto lr = std::make_shared<bo_live>();
  lr->active = sp.active;
  if (!rc) {
    lr->slot = slot_acquire(dev);
    if (!lr->slot) rc = fail(BO_ERR_HIP, "live run: stream / mailbox allocation failed");
  }
  if (!rc) rc = wg_launch(lr->slot, &cfg, true, lr->run);
  std::lock_guard<std::mutex> g(net->mu);
  if (rc) {
    if (rc == BO_ERR_HIP) lr->failed = true;
    net->in_flight = false;
    net->started = false;          // nothing ran: the start may be retried
    return rc;
  }
  net->live = lr;
  net->live_rc = 0;
  net->stop_events.clear();
  // stops served between the prologue and now reach the kernel too
  std::vector<uint32_t> late;
  for (uint32_t i : sp.active)
    if (net->st[i].killed) late.push_back(i);
  if (!late.empty()) live_post(lr.get(), late.data(), (uint32_t)late.size());
  return BO_OK;
}

int bo_consensus_wait(bo_network *net) {
  if (!net) return fail(BO_ERR_INVALID_ARGUMENT, "net is NULL");
  std::shared_ptr<bo_live> lr;
  {
    std::lock_guard<std::mutex> g(net->mu);
    lr = net->live;
  }
  if (!lr) return BO_OK;
  const hipError_t e = hipStreamSynchronize(lr->slot->s);   // no lock held: /stop, /getState stay served
  return live_finalize(net, lr, e);
}

int bo_consensus_poll(bo_network *net, int *running_out) {
  if (!net || !running_out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  *running_out = 0;
  std::shared_ptr<bo_live> lr;
  {
    std::lock_guard<std::mutex> g(net->mu);
    lr = net->live;
  }
  if (!lr) return BO_OK;
  const hipError_t e = hipStreamQuery(lr->slot->s);
  if (e == hipErrorNotReady) {
    *running_out = 1;
    return BO_OK;
  }
  return live_finalize(net, lr, e);
}

namespace {
// Every node's state into out[N]: the network's own states, or -- while a live
// run is in flight -- a snapshot the kernel takes at its next batch boundary
// (the delivery count it reflects in *events_out), with the killed flags of
// GET /stop requests it has not applied yet (node.ts:191-194 sets killed at
// once).  A run that ends before it answers is finalized and its final states
// returned.
int get_states_impl(bo_network *net, bo_node_state *out, uint64_t *events_out) {
  if (events_out) *events_out = UINT64_MAX;
  std::shared_ptr<bo_live> lr;
  {
    std::lock_guard<std::mutex> g(net->mu);
    lr = net->live;
    if (!lr) {
      std::copy(net->st.begin(), net->st.end(), out);
      return net->live_rc;
    }
  }
  LiveSlot *sl = lr->slot;
  hipError_t q = hipStreamQuery(sl->s);
  if (q == hipErrorNotReady) {
    std::lock_guard<std::mutex> s(net->snap_mu);
    // a snapshot served within the last kSnapReuse answers this request too:
    // the reference's getNodesState is N concurrent GET /getState
    // (__test__/tests/utils.ts:14-20), and each snapshot costs the kernel its
    // host-memory writes (a tight poll loop slowed a run 4x)
    auto answer = [&]() {
      std::lock_guard<std::mutex> g(net->mu);
      std::copy(net->st.begin(), net->st.end(), out);   // nodes that do not run keep theirs
      for (size_t a = 0; a < lr->active.size(); ++a) {
        const uint32_t i = lr->active[a], w0 = lr->snap_words[2u * a], w1 = lr->snap_words[2u * a + 1u];
        bo_node_state s;
        s.killed = (int8_t)((w0 & 0xFFu) | (uint32_t)(net->st[i].killed != 0));   // /stop posted since
        s.x = (int8_t)(w0 >> 8);
        s.decided = (int8_t)(w0 >> 16);
        s.pad = 0;
        s.k = (int32_t)w1;
        out[i] = s;
      }
      if (events_out) *events_out = lr->snap_e;
      return BO_OK;
    };
    constexpr auto kSnapReuse = std::chrono::microseconds(500);
    if (lr->snap_ok && std::chrono::steady_clock::now() - lr->snap_t < kSnapReuse) return answer();
    uint32_t *box = sl->box;
    const uint32_t want = __atomic_add_fetch(&box[benor::kSnapReq], 1u, __ATOMIC_RELEASE);
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0;; ++spin) {
      if (__atomic_load_n(&box[benor::kSnapSeq], __ATOMIC_ACQUIRE) == want) {
        lr->snap_e = (uint64_t)__atomic_load_n(&box[benor::kSnapE], __ATOMIC_RELAXED) |
                     ((uint64_t)__atomic_load_n(&box[benor::kSnapE + 1u], __ATOMIC_RELAXED) << 32);
        lr->snap_words.resize(2u * lr->active.size());
        for (size_t a = 0; a < lr->active.size(); ++a) {
          const uint32_t i = lr->active[a];
          lr->snap_words[2u * a] = box[benor::kSnapSt + 2u * i];
          lr->snap_words[2u * a + 1u] = box[benor::kSnapSt + 2u * i + 1u];
        }
        lr->snap_t = std::chrono::steady_clock::now();
        lr->snap_ok = true;
        return answer();
      }
      if ((spin & 63u) == 63u) {
        q = hipStreamQuery(sl->s);
        if (q != hipErrorNotReady) break;          // the run ended before it served the request
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10))
          return fail(BO_ERR_INTERNAL, "a live run did not serve a /getState snapshot within 10 s");
        std::this_thread::yield();
      }
    }
  }
  const int rc = live_finalize(net, lr, q);
  std::lock_guard<std::mutex> g(net->mu);
  std::copy(net->st.begin(), net->st.end(), out);
  return rc;
}
}  // namespace

int bo_get_states(const bo_network *net, bo_node_state *out, uint32_t n, uint64_t *events_out) {
  if (!net || !out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  if (n != net->N) return fail(BO_ERR_INVALID_ARGUMENT, "out must have N entries");
  return get_states_impl(const_cast<bo_network *>(net), out, events_out);
}

int bo_live_stop_events(const bo_network *net, uint32_t *events_out, uint32_t n) {
  if (!net || !events_out) return fail(BO_ERR_INVALID_ARGUMENT, "NULL argument");
  if (n != net->N) return fail(BO_ERR_INVALID_ARGUMENT, "events_out must have N entries");
  std::lock_guard<std::mutex> g(net->mu);
  if (net->live) return fail(BO_ERR_INVALID_ARGUMENT, "a live run is in flight: bo_consensus_wait first");
  for (uint32_t i = 0; i < n; ++i) events_out[i] = i < net->stop_events.size() ? net->stop_events[i] : 0xFFFFFFFFu;
  return BO_OK;
}

double bo_popc_peak(uint32_t iters) {
  if (check_device(nullptr)) return 0.0;
  int dev = 0, cus = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  DeviceBuf<uint32_t> sink_buf;
  if (sink_buf.alloc((size_t)cus * 8u) != hipSuccess) return 0.0;
  uint32_t *const sink = sink_buf.d;
  const int grid = cus * 8, inner = 2048;
  double words = 0;
  const float ms = timed_launches_ms(iters, [&] { (void)benor::launch_popc_peak(sink, grid, inner, nullptr, &words); });
  if (ms <= 0) return 0.0;
  return words * iters / (ms * 1e-3);
}

double bo_mfma_peak(uint32_t iters) {
  if (check_device(nullptr)) return 0.0;
  int dev = 0, cus = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const int grid = cus * 2, inner = 4096;   // 2 waves per SIMD
  DeviceBuf<float> sink_buf;
  if (sink_buf.alloc((size_t)grid) != hipSuccess) return 0.0;
  float *const sink = sink_buf.d;
  double terms = 0;
  const float ms = timed_launches_ms(iters, [&] { (void)benor::launch_mfma_peak(sink, grid, inner, nullptr, &terms); });
  if (ms <= 0) return 0.0;
  return terms * iters / (ms * 1e-3);
}

}  // extern "C"
