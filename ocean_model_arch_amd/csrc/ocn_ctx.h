// ocn_ctx.h -- the model context and what its sources share (ocn_ctx.hip, ctx_comm.hip, ctx_setup.hip, and through
// ocn_ens.h the ensemble's host sources).  Internal: not part of the C ABI (include/ocn_sw.h), included by those only.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "ocn_internal.h"
#include "ocn_step_plan.h"

namespace ocn {

#define HIPCHK(call)                                          \
    do {                                                      \
        int _rc = check_hip((call), #call);                   \
        if (_rc) return _rc;                                  \
    } while (0)
#define RC(call)                                              \
    do {                                                      \
        int _rc = (call);                                     \
        if (_rc) return _rc;                                  \
    } while (0)


// ------------------------------------------------------------------ halo segments
// w strided 1-D runs of doubles side by side: dst[i*dst_stride + j*dst_jstride] =
// src[i*src_stride + j*src_jstride], i < count, j < w.  A column strip several layers deep is one
// such segment (merge_columns: w adjacent columns), so a wave's loads take the layers of 64 / w rows
// from shared cache lines instead of one line per element and layer.
struct Seg {
    const double *src;
    double *dst;
    long src_stride, dst_stride;
    int count;
    int w = 1;
    long src_jstride = 0, dst_jstride = 0;
};

// one workgroup of k_segments per chunk of a segment (ctx_comm.hip kSegChunk elements)
struct SegChunk { int seg, e0; };

// A segment list on the device with its chunk table (make_seglist)
struct SegList {
    Seg *d = nullptr;
    SegChunk *ch = nullptr;
    int n = 0, nch = 0;
};

// ------------------------------------------------------------------ geometry helpers
// decomposition.f90:94-290, directions macros/kernel_macros.fi:4-12
struct Rect { int x0, x1, y0, y1; };
static const int kDirDm[9] = {0, 1, -1, 0, 0, 1, 1, -1, -1};
static const int kDirDn[9] = {0, 0, 0, 1, -1, 1, -1, 1, -1};

}  // namespace ocn

using namespace ocn;

// ------------------------------------------------------------------ context
struct GBlock {            // one block of the global block grid
    int bm, bn;
    ocn_block g;           // pitch filled for local blocks only
    int rank;              // -1 land block (bglob_proc = -1)
    int k;                 // local index on its rank
    double weight;         // sea points (bglob_weight)
};

struct LBlock {
    ocn_block g;
    int bm, bn, gid;
    int nbr_rank[8], nbr_k[8], nbr_gid[8];
    void *slab = nullptr;
    std::vector<void *> ptr;           // field table, indexed by field_slot(id)
    uint8_t *bits = nullptr;           // compact static fields (sw_stencils.h): mask bytes
    float *rows = nullptr;             // and metric row tables
    void *sshp_alt = nullptr;          // second sshp buffer of the recompute steps (one_step_fused)
    void *up_alt = nullptr, *vp_alt = nullptr;   // second ubrtrp / vbrtrp buffers of the one-pass steps
    std::vector<void *> ffp_alt;       // second ff1p buffer of every tracer (one-pass steps' tracer step)
    double *kc = nullptr;              // device: h_r, mu of the one-pass step's known-constant variant
    // one_step_x2 (one 2-deep state exchange per one-pass step, the march over the whole interior):
    unsigned own = 0;                  // halo points neighbour blocks own (sw_stencils.h own_class bits)
    float *ext = nullptr;              // metric values of rows bnd_y1 / bnd_y2 as the neighbours form them
    float *rows_x = nullptr;           // the row table with those two rows (launch_rows_ext)
    double *hr_x = nullptr;            // h_r with its second halo ring from the neighbours
    double *ring2 = nullptr;           // the state's second halo ring as the reference leaves it (saved)
    // one_step_x4 (two one-pass steps per launch, one 4-deep state exchange per pair): mask bytes and the
    // row table over the block widened by kXRing rings (launch_x4_tables; bits_x4 based at
    // A(bnd_x1 - kXRing, bnd_y1 - kXRing), pitch g.pitch)
    uint8_t *bits_x4 = nullptr;
    float *rows_x4 = nullptr;
    SegList save, restore;   // its save / restore runs (k_segments)
    // x4 pairs with tracers: the first step's new ssh, sshp, ubrtr, vbrtr (based like the fields: kXRing
    // extra rows; MarchStep::trs), the state the second tracer step reads
    double *trs[4] = {nullptr, nullptr, nullptr, nullptr};
    template <typename T> T *f(int id) const { return (T *)ptr[field_slot(id)]; }
};

// Loopback transport (ocn_ctx_attach_loopback): the N ranks of a decomposition as N contexts of
// ONE process on one device, each driven by its own host thread.  It replaces exactly two RCCL
// calls and nothing else -- the ncclRecv / ncclSend pair of an exchange (run_sync) and the
// ncclAllReduce of the role-flip vote (check_coherence) -- so the remote branch of the halo plans
// (device pack / unpack, per-peer messages, per-role plans, sync_ca, overlap forks) runs as in
// production.  An exchange is two host rendezvous with the peers:
//   A: each rank has enqueued its pack and recorded lb_ev_a, and publishes its plan; then every
//      rank copies each peer's send buffer (for it) into its own receive buffer, on its stream,
//      after the peer's lb_ev_a, and records lb_ev_b;
//   B: every rank's stream waits for its peers' lb_ev_b, so no send buffer is repacked before the
//      peer's copy out of it has run (the completion guarantee of ncclGroupEnd).
// The counters make the rendezvous of the k-th exchange of every rank meet (all ranks run the
// same sequence of exchanges, as with RCCL); a peer cannot pass phase A of exchange k+1 before
// this rank passed phase B of exchange k, so a published plan / recorded event is never replaced
// before it was consumed.
struct HaloPlan;
struct Loopback {
    int n = 0;
    std::vector<ocn_ctx *> ctx;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<uint64_t> cnt[4];              // per rank: exchange A/B, reduce A/B phases passed
    std::vector<const HaloPlan *> plan;        // plan of the rank's current exchange (phase A)
    std::vector<int32_t *> vote;               // the rank's flag word (reduce phase A)
    bool failed = false;
    int refs = 0;
};

struct HaloPlan {
    SegList local;                    // intra-process copies
    // remote: per peer rank, pack segments (into send buffer) and unpack segments (from recv)
    struct Peer { int rank; long count; double *send, *recv; };
    std::vector<Peer> peers;
    SegList pack, unpack;
};

// ocn_ctx::fb_state
enum { kFbUnchecked = 0, kFbDevice = 1, kFbZero = 2, kFbGeneral = 3, kFbHr = 4 };

#ifndef OCN_COMM_PRIO
#define OCN_COMM_PRIO 1   // the comm stream at the device's highest stream priority
#endif
struct ocn_ctx {
    ocn_basin basin;
    ocn_sw_params sw;
    ocn_decomp dec;
    std::vector<int32_t> mask;         // global (nx, ny) column-major
    std::vector<float> topo;           // bottom topography, (nx-4) x (ny-4) interior points (empty: none)
    int bnx = 1, bny = 1;
    std::vector<GBlock> gblocks;       // (bm-1) + (bn-1)*bnx
    std::vector<LBlock> blocks;
    hipStream_t stream = nullptr;
    hipStream_t comm_stream = nullptr;  // halo exchanges overlapped with interior compute
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // the known-constant check's verdict copied to pinned host memory behind an event: a later call
    // reads it once the event has completed (hipEventQuery: no wait), learn_fb_async
    hipEvent_t ev_fb = nullptr;
    int32_t *h_fbz = nullptr;
    bool fb_copy = false;
    int overlap = -1;            // OCN_OPT_OVERLAP: 0 none, 1 standard steps, 2 + role-flip steps, -1 auto
    // OCN_OPT_OVERLAP auto with peers on other ranks: the x2 / x4 steps' form (inner part beside the
    // exchange, or exchange then march) chosen from a measurement (ov_begin).  One slot per step form
    // (ov_slot[0]: x2 steps, [1]: x4 pairs; a call that runs both loses neither's measurement): state 0 =
    // nothing measured, 1 = a sequential step's events recorded, 2 = an overlapped one's too (the next
    // vote reduces them).  ov_final 0 = undecided, 3 = decided (ov_level), 4 = gave up after kOvMaxVotes
    // votes without a decision (level 2, no further probes); ov_kind = the step form measured last or
    // decided from (2: x2 steps, 4: x4 pairs); ov_votes = the votes taken while undecided; ov_probes =
    // the steps run as probes; ov_ms = the two step times the decision used (maxima over the ranks)
    struct OvSlot {
        int state = 0;
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    };
    OvSlot ov_slot[2];
    int ov_final = 0, ov_kind = 0, ov_level = 2, ov_votes = 0, ov_probes = 0;
    double ov_ms[2] = {0.0, 0.0};
    int xdelay_us = 0;           // OCN_OPT_XCHG_DELAY (tests): a device wait before each exchange with remote peers
    int32_t *d_nbad = nullptr;
    int32_t *d_red = nullptr;    // the loopback vote's reduction (allreduce_max): 64 words behind d_nbad's
    unsigned *d_bar = nullptr;   // the multi-step launch's grid-barrier words (kMultiBarBytes)
    ncclComm_t comm = nullptr;
    bool comm_aborted = false;         // fail_fatal aborted the communicator: calls with exchanges fail
    Loopback *lb = nullptr;            // test transport between contexts of one process (ocn_ctx_attach_loopback)
    hipEvent_t lb_ev_a = nullptr, lb_ev_b = nullptr;
    std::map<std::vector<int>, HaloPlan> plans;
    bool initialized = false;
    bool use_graph = false;
    // the launches a captured step replays depend on everything in its key (march and ring_sea
    // select launch forms and the ring launch; options that change them also drop the cache)
    struct Graph { hipGraphExec_t exec; double tau; ocn::StepKind kind; bool compact, march, ring_sea; int role, kc_mode; bool kc_nv; int pair_rows; };
    std::vector<Graph> graphs;         // one captured step per key
    std::vector<void *> allocs;
    // per-stage HIP-event timing (OCN_OPT_STAGE_TIMING): pending (stage, start, stop) records
    bool stage_timing = false;
    struct Rec { int stage; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> event_pool;
    double stage_ms[OCN_NUM_TIMERS] = {0};
    int64_t stage_n[OCN_NUM_TIMERS] = {0};
    bool fused = true;
    std::vector<int> sync_a, sync_a_reuse, sync_b, sync_ca, sync_ca_reuse;
    // compact static fields: requested (OCN_OPT_COMPACT), in use, stale (real(4) fields
    // changed since they were built), or unusable because raw real(4) pointers were handed out
    bool compact_req = true, compact = false, static_dirty = true;
    bool march = true;   // OCN_OPT_MARCH
    mutable bool r4_escaped = false;
    // role-flip steps (one_step_fused): role = 1 while the ssh/sshn, ubrtr/ubrtrn, vbrtr/vbrtrn
    // buffers of every block are swapped (only inside an ocn_ctx_step call); coherent = the pairs
    // agree outside their write sets (sw_stencils.h Coherence), coherent_known = that was checked
    // after the state last changed outside ocn_ctx_step; r8_escaped = raw pointers of a pair were
    // handed out (check at every call); flip = OCN_OPT_FLIP
    bool flip = true, coherent = false, flip_used = false, rc_used = false;
    bool capturing = false;      // a step is being captured into a hipGraph
    bool sync_pending = false;   // an exchange on comm_stream not yet joined (fork_sync)
    bool ring_sea = true;   // some halo-ring point has a mask set (Prepare); else no ring launch
    bool udiv_ok = true;    // every row divisor of the one-pass step in [2^-60, 2^60] (Prepare)
    bool recompute = true;  // OCN_OPT_RECOMPUTE: recompute steps in role-flip calls
    bool onepass = true;    // OCN_OPT_ONEPASS: one-pass steps in single-block role-flip calls
    // OCN_OPT_PAIR: two one-pass steps per launch (one_step_pair) -- 0 never, 1 on blocks of at least
    // kPairMinCells interior points, 2 on any block; pair_used: a call ran one
    int pair = 1;
    bool pair_used = false;
    // OCN_OPT_MULTI: the one-pass steps of a small single block as one launch per call
    // (one_step_multi); multi_used: the last call ran one
    bool multi = true, multi_used = false;
    mutable int multi_fits = -1;   // onepass_multi_fits of the one block (-1: not asked yet; geometry and device stay)
    // OCN_OPT_TRACER_STEP: tracer runs with one-pass steps -- expl_tracer of each step as one launch per
    // tracer (run_tracer_step), run with the next step, after its exchange; tr_call: this call does;
    // tr_pending: the current state's tracer step has not run yet; tr_alt_ok: the second ff1p
    // buffers agree with the fields outside the tracer step's write set.  Role bits 8 (ff1 / ff1n
    // traded) and 16 (ff1p / its second buffer traded), for every tracer at once.
    bool tr_step = true, tr_call = false, tr_pending = false;
    bool tr_forked = false;   // a tracer step runs on the comm stream beside the march (joined by run_step)
    mutable bool tr_alt_ok = false;
    bool known_const = true;   // OCN_OPT_KNOWN_CONSTANTS: the one-pass step's known-constant variant
    bool last_hybrid = true;   // OCN_OPT_ONEPASS_LAST: one-pass last steps with exchanges / ring work too
    bool one_used = false;
    // the one-pass steps' second sshp / ubrtrp / vbrtrp buffers agree with the fields outside a8's
    // write set (else they are copied at the start of the next such call)
    mutable bool alt_ok = false;
    // hh_init's stored depths were formed from the current state (the last step of the previous
    // call or init_state ran it and nothing has changed the state since): the first step of a
    // call may then be a one-pass step too, as a reuse step.  Never again once an r8 field's
    // device pointer was handed out (it may be written behind our back).
    mutable bool hh_consistent = false, r8_handed = false;
    // hh_init's n level -- hqn = h_r and its interpolations hun / hvn / hhn (depth.f90:14-99 with
    // ffs; no ssh in it) -- is what those arrays hold: a full hh_init wrote them from the current
    // h_r, masks and metrics, and nothing has written them since (the one-pass, pair and
    // multi-step launches never do).  last_finish's hh_init then leaves them as they are (32 B
    // per cell of its 96 B of stores).  Cleared by every other step kind, by any upload, stage,
    // sync or init, and never trusted once a raw pointer was handed out.
    mutable bool hn_fresh = false;
    // hhq_n may differ from h_r (an upload of either, or a raw pointer): every hh_init stores
    // hhq_n = h_r, but the role-flip steps' fused hh_init + A (CA) does not, so the standard tracer
    // stages after such a step copy it first (expl_tracer)
    mutable bool hqn_stale = false;
    // the one-pass step's known-constant precondition (sw_kernels.hip FallbackCheck: fallback points
    // and forcing +0.0, h_r and mu uniform): kFbUnchecked until a check ran after the arrays last
    // changed from outside the step; kFbDevice = its verdict is in device memory (d_fbz; both
    // variants are launched and the device picks, ocn_ctx.hip never waits for it) until a host
    // sync the caller makes anyway reads it (learn_fb): kFbZero / kFbHr (all but h_r: a
    // non-uniform rest depth, read by the OCN_KC_KNOWN_HR variant) / kFbGeneral
    mutable int fb_state = 0;
    int kc_mode = 0;             // OCN_KC_* of the current call's one-pass launches
    // OCN_OPT_INVISCID: the two-step launches' inviscid bodies (sw_kernels.hip MarchStep NV) where mu is
    // +0.0 (fb_inviscid: the word after the verdict, learnt with fb_state) and every r_diss row +0.0f with
    // finite metrics (rdiss_zero: Prepare).  kc_nv: this call's pairs run them (prepare_kc; with a
    // communicator every rank's verdict: nv_dev_ok, check_coherence); nv_used: a pair of the last call did
    bool inviscid = true, rdiss_zero = false, nv_dev_ok = false, kc_nv = false, nv_used = false;
    mutable bool fb_inviscid = false;
    int32_t *d_fbz = nullptr;    // the check's verdict word
    // lazy call tail (OCN_OPT_LAZY_TAIL): the last step run was a one-pass step; what the reference's
    // last step leaves beyond the state (vort, stresses, RHS terms, hh_init's levels, a8's copies) is
    // formed when the host next looks (complete_open: the step redone from the previous state, still
    // intact in the other buffers, as the call's last step), so 1-step calls run one-pass steps
    bool lazy = true, open = false, open_x2 = false;
    double open_tau = 0.0;
    // pairs in an open sequence (one_step_pair): open_pair = its last launch was a pair (the state
    // before it is two steps back: complete_open redoes the pair's first step single, then the tail);
    // deferred = the last 1 or 2 steps of the sequence, not yet run: a call runs pairs while 3 or
    // more steps are pending and leaves the rest to the next call -- the 1-step cadence runs a pair
    // every second call -- or to complete_open, which runs them as the last steps (a single + the
    // last step, or the last step: no step run twice); synchronize runs them (as a pair or alone)
    bool open_pair = false;
    int deferred = 0;
    bool deferred_check[2] = {false, false};
    // one_step_x2 (OCN_OPT_X2): its static conditions (ext_ok: the real(4) fields are init_state's,
    // so the ext rows are the neighbours' metric rows; rows_x_ok: their divisors in udiv's range;
    // edge_ring_sea: a8 / a9 work on a halo ring no neighbour fills), the device checks of the last
    // check_coherence (x2_dev_ok: the state's first halo ring holds the neighbours' values and its
    // halo points no exchange fills hold +0.0), whether the h_r copy is current, and whether the
    // state's second halo ring is saved (a sequence of x2 steps is under way)
    bool x2 = true, rows_x_ok = false, edge_ring_sea = true, x2_dev_ok = false;
    mutable bool ext_ok = false, hrx_ok = false;
    bool ring2_saved = false, x2_used = false;
    // one_step_x4 (OCN_OPT_X4): pairs of x2 steps with one 4-deep exchange each; x4_tab_ok: its tables
    // were built from init_state's real(4) fields with every divisor in udiv's range; x4_dev_ok: the
    // last vote found every rank able to run them (a communicator attached); x4_used: the last call did
    // x4: 0 off, 1 auto (tracer runs: only with peers on other ranks), 3 always
    int x4 = 1;
    bool x4_tab_ok = false, x4_dev_ok = false, x4_used = false;
    bool fb_x2 = false;          // the known-constant check's verdict is for the x2 range / tables
    mutable bool coherent_known = false, r8_escaped = false;
    int multi_spin = kMultiSpin;   // OCN_OPT_MULTI_SPIN (the multi-step launch's barrier bound)
    // OCN_OPT_CO_LAUNCH: an x2 step's march and the previous state's tracer step as one launch;
    // co_used: the last call did
    bool co_launch = true, co_used = false;
    double stage_max[OCN_NUM_TIMERS] = {0};   // longest record per timer (ocn_ctx_stage_stats)
    // halo exchanges with remote peers (run_sync): how many were enqueued; while a watchdog is set an
    // event after each (xq, under xmu) tells it the id of the last one the device completed (xdone)
    int64_t xchg = 0, xdone = -1;
    std::mutex xmu;
    std::deque<std::pair<int64_t, hipEvent_t>> xq;
    std::vector<hipEvent_t> xpool;
    // host-side watchdog (ocn_ctx_set_watchdog): the thread, the call it watches (call_depth > 0: a
    // guarded entry is running since call_t0), and whether it fired (wd_msg: what the calls return)
    double wd_s = 0;
    std::thread wd;
    std::mutex wd_mu;
    std::condition_variable wd_cv;
    bool wd_stop = false;
    int call_depth = 0;
    std::chrono::steady_clock::time_point call_t0;
    const char *call_name = "";
    std::atomic<bool> wd_fired{false};
    std::string wd_msg;
    std::mutex comm_mu;          // the communicator is aborted once: by the watchdog or by fail_fatal
    bool comm_abort_done = false;
    int role = 0;
    int steps_run = 0;           // launches statistics of the last call (ocn_ctx_get_option OCN_OPT_LAUNCHES)
    int64_t launches = 0;
    int32_t *d_flags = nullptr;
    bool batch = true;           // OCN_OPT_BATCH
    ocn::Batcher batcher;
    // a member of an ensemble (ocn_ens_create): the ensemble owns the context and its compute stream,
    // which the members share.  Inside ocn_ens_step (step_entry with collect) step_impl plans a multi-step
    // launch as ever but leaves it to the ensemble, which issues it with the other members': ens_pending = the
    // call left one, ens_k = its kind.  (What a call would plan, with none of its steps run: step_probe.)
    ocn_ens *ens = nullptr;
    bool ens_pending = false;
    // forced (ocn_ens_forcing_set): the ensemble writes OCN_RHSX / OCN_RHSY of this member for each step's own
    // time -- the general one-pass variant at once (prepare_kc), no pair launches (pair_ok)
    bool forced = false;
    ocn::StepKind ens_k{};
};

namespace ocn {

// real(8) fields of a context: the SW set, then flux_x, flux_y and ff1/ff1p/ff1n per tracer
inline int num_r8(const ocn_ctx *c)
{
    return OCN_NUM_R8 + (c->sw.use_tracers > 0 ? 2 + 3 * c->sw.tracer_num : 0);
}
inline bool has_r8(const ocn_ctx *c, int id) { return id >= OCN_SSH && id < OCN_SSH + num_r8(c); }
inline bool has_field(const ocn_ctx *c, int id) { return is_r4(id) || has_r8(c, id); }
// a tracer field (ff1 / ff1p / ff1n of some tracer)
inline bool is_tracer_field(int id) { return id >= OCN_TRACER_BASE; }
inline bool is_alt_field(int id) { return id == OCN_SSHP || id == OCN_UBRTRP || id == OCN_VBRTRP; }
inline size_t field_bytes(const LBlock &b) { return (size_t)b.g.pitch * (b.g.bnd_y2 - b.g.bnd_y1 + 1) * 8; }
inline bool has_comm(const ocn_ctx *c) { return c->comm || c->lb || c->comm_aborted; }
// block b's one-pass variant for the current call (ctx kc_mode, the device verdict, its constants)
inline OnepassKC kc_of(const ocn_ctx *c, const LBlock &b) { return OnepassKC{c->kc_mode, c->d_fbz, b.kc, c->kc_nv}; }

// ---- ctx_comm.hip: halo plans, the RCCL / loopback transport, the watchdog
int make_seglist(ocn_ctx *c, const std::vector<Seg> &v, SegList &out);
int launch_segs(const SegList &l, hipStream_t s, int32_t *cmp = nullptr);
int get_plan(ocn_ctx *c, const std::vector<int> &fields, HaloPlan *&out, int depth = 1, int priv = 0);
int run_sync(ocn_ctx *c, const std::vector<int> &fields, hipStream_t stream = nullptr, int32_t *cmp = nullptr,
             int depth = 1, int priv = 0);
// d_nbad's words of the known-constant check (ctx_setup.hip allocate): the verdict the launches' gates read,
// and right after it the word FallbackCheck ORs into when mu's one value is not +0.0 (flag[1]; the host's alone)
constexpr int kFbzWord = 16, kFbzWords = 2;
constexpr int kVoteWords = 12;   // the role-flip vote (check_coherence): one word per condition (d_flags has 16)
// the measured overlap choice gives up after this many votes without a decision (include/ocn_sw.h
// ocn_overlap_info states the number)
constexpr int kOvMaxVotes = OCN_OVERLAP_MAX_VOTES;
int allreduce_max(ocn_ctx *c, int32_t *word, hipStream_t s, int words = 1);
int nccl_rc(ncclResult_t r, const char *what);
int fail_fatal(ocn_ctx *c, int rc);
int64_t poll_xdone(ocn_ctx *c);
void wd_loop(ocn_ctx *c);

// An entry that may take part in a collective, watched while a watchdog is set
struct CallGuard {
    ocn_ctx *c;
    CallGuard(ocn_ctx *ctx, const char *name);
    ~CallGuard();
};
template <class F> static int guarded(ocn_ctx *c, const char *name, F &&f)
{
    if (c->wd_fired.load()) return set_error(OCN_ERR_COMM, c->wd_msg);
    int rc;
    {
        CallGuard g(c, name);
        rc = f();
    }
    if (c->wd_fired.load()) {   // (the call returned because the watchdog ended it)
        std::lock_guard<std::mutex> g(c->comm_mu);
        if (c->comm) { c->comm = nullptr; c->comm_aborted = true; }
        return set_error(OCN_ERR_COMM, c->wd_msg);
    }
    return rc;
}

// ---- ctx_setup.hip: decomposition, storage, the initial state, the compact tables
void set_mask(ocn_ctx *c, const int32_t *mask);
int decompose(ocn_ctx *c);
int host_ctx(const ocn_basin *basin, const ocn_decomp *dec, const int32_t *mask, ocn_ctx *&c);
int allocate(ocn_ctx *c);
int upload_field(ocn_ctx *c, const LBlock &b, int id, const void *host, bool async);
int init_state(ocn_ctx *c);
int prepare_static(ocn_ctx *c);

// ---- ocn_ctx.hip: timers, stages, the step driver
int get_event(ocn_ctx *c, hipEvent_t &e);
int timer_begin(ocn_ctx *c, int id, ocn_ctx::Rec &rec);
int timer_end(ocn_ctx *c, ocn_ctx::Rec &rec);
int envoke(ocn_ctx *c, int stage, double tau);
bool has_exchange(const ocn_ctx *c);
void swap_roles(ocn_ctx *c);
void swap_alt3(ocn_ctx *c);
int run_step(ocn_ctx *c, double tau, const StepKind &k);
int finish_call(ocn_ctx *c, int rc);
int complete_open(ocn_ctx *c);
int step_entry(ocn_ctx *c, double tau, int32_t nsteps, int32_t check_every, bool collect = false);
int step_probe(ocn_ctx *c, double tau, int32_t nsteps, int32_t check_every, bool *multi, bool *go);
// field id counts as uploaded: ocn_ctx_upload's bookkeeping and nothing else, for an entry that has
// rewritten the field's current array on the context's stream (ocn_ens_transform); no pending tail open
void field_uploaded(ocn_ctx *c, int id);
// shared: the compute stream of the ensemble `ens` the context becomes a member of (null: its own)
int ctx_create(const ocn_basin *basin, const ocn_sw_params *sw, const ocn_decomp *dec, const int32_t *mask,
               hipStream_t shared, ocn_ens *ens, ocn_ctx **out);
int ctx_destroy(ocn_ctx *c);
// k_output_r4 of a real(8) array on stream s
int launch_output_r4(const double *src, const float *lu, long pitch, int w, int h, float undef, float *dst,
                     hipStream_t s);

// f(b) for every block of the context.  With OCN_OPT_BATCH and several blocks the launches f makes
// on stream s are batched (ocn_internal.h Batcher): each kernel of the loop is launched once for all
// the blocks (up to kPack of them per launch) instead of once per block.  Only for loops whose
// launches read and write their own block's arrays, with nothing but batchable launches on s.
// co: the loop's launches read nothing another writes -- a march batch and the tracer-step batch
// after it may go as one launch (Batcher::co_launch; batched for one block too)
template <class F> static int each_block(ocn_ctx *c, hipStream_t s, F &&f, bool co = false)
{
    const bool on = c->batch && (c->blocks.size() > 1 || co);
    if (on) {
        batch_begin(&c->batcher, s);
        c->batcher.co_launch = co;
    }
    int rc = OCN_OK;
    for (size_t i = 0; i < c->blocks.size() && rc == OCN_OK; ++i) {
        if (on) batch_next(&c->batcher);
        rc = f(c->blocks[i]);
    }
    if (on) {
        const int r2 = batch_end(&c->batcher);
        if (rc == OCN_OK) rc = r2;
        if (co && c->batcher.co_launched) c->co_used = true;
    }
    return rc;
}

}  // namespace ocn
