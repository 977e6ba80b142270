// ocn_ctx.hip -- PSy layer of the MI355X shallow-water step: the stages, every step form, the call
// driver (step_impl, step_probe, complete_open, run_deferred, finish_call: the device phases around the plans
// of ocn_step_plan.h), check_coherence and the ocn_ctx_*
// entries of the C ABI.  The context itself is ocn_ctx.h; its halo exchange is ctx_comm.hip, its
// decomposition, storage and initial state ctx_setup.hip, the ensemble layer ocn_ens*.hip.
//
// Reference counterparts (Andrcraft9/ocean_model_arch):
//   dispatcher     core/kernel_interface.f90:48-119 (envoke) + interface/shallow_water/sw_interface.f90
//   algorithm      control/shallow_water/shallow_water.f90:22-94 (expl_shallow_water)
#include "ocn_ctx.h"

namespace ocn {

static thread_local std::string g_last_error;

int set_error(int code, const std::string &msg)
{
    g_last_error = msg;
    return code;
}

static std::atomic<long long> g_launches{0};
void count_launch() { g_launches.fetch_add(1, std::memory_order_relaxed); }

int check_hip(hipError_t e, const char *what)
{
    if (e == hipSuccess) return OCN_OK;
    return set_error(OCN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// One output record of a field (output.f90:101-106 copy_from_real8 + io.f90:343-349): real(4) of
// the interior value, undef where |lu| < 0.5; dst is the packed interior, Fortran order.
template <typename T>
__global__ void k_output_r4(const T *src, const float *lu, long pitch, int w, int h, float undef, float *dst)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x), j = (int)blockIdx.y;
    if (i >= w || j >= h) return;
    const long s = (long)j * pitch + i;
    dst[(long)j * w + i] = fabsf(lu[s]) < 0.5f ? undef : (float)src[s];
}
int launch_output_r4(const double *src, const float *lu, long pitch, int w, int h, float undef, float *dst,
                     hipStream_t s)
{
    hipLaunchKernelGGL(k_output_r4<double>, dim3((unsigned)((w + 255) / 256), (unsigned)h), dim3(256), 0, s, src, lu,
                       pitch, w, h, undef, dst);
    return check_launch();
}

// OCN_OPT_OVERLAP in effect: by default (-1) the role-flip steps' exchanges overlap their inner
// launches (2) when exchanges go to other ranks (RCCL: latency, not copy bandwidth), and run
// between the launches (1) when every exchange is a local device copy -- there the frame bands
// cost as much as the copies they hide (HISTORY.md section 5)
static int overlap_level(const ocn_ctx *c)
{
    if (c->overlap >= 0) return c->overlap;
    if (!(has_comm(c) && c->dec.nranks > 1)) return 1;
    return c->ov_final == 3 ? c->ov_level : 2;   // (measured: ov_begin, check_coherence; 4 = gave up: 2)
}

// The form of an x2 step (kind 2) or an x4 pair (kind 4) under OCN_OPT_OVERLAP auto with peers on
// other ranks.  Until the vote has decided, the first such step (not one that opens a sequence: its
// ring save would be timed too) runs in sequence and the next of the same kind overlapped, each
// between two events on the context stream (probe 1 / 2: ov_mark at its start and end); the next
// check_coherence max-reduces both times over the ranks and keeps the faster form (ov_level) --
// every rank the same.  Either form runs the same exchange (one group per step or pair), so ranks
// may differ in form meanwhile; the results are the same bit for bit.
// Each kind has its own slot (ocn_ctx::ov_slot): a call of pairs that ends in a single x2 step
// advances both measurements instead of starting each over.  `allow` must be the same on every rank
// (every rank runs the same step kinds -- the vote sees to that -- so the slots then advance
// together): not the opening step of a sequence, and for the pairs x4_inner_everywhere, which reads
// the global block table.  Once the choice is final (decided, or given up after kOvMaxVotes votes) no
// step is a probe.
static int ov_begin(ocn_ctx *c, int kind, bool allow, int &probe)
{
    probe = 0;
    const int lv = overlap_level(c);
    ocn_ctx::OvSlot &slot = c->ov_slot[kind == 4];
    // (a kind with both forms measured waits for the next vote: no probe of the other kind meanwhile)
    if (c->overlap >= 0 || !(has_comm(c) && c->dec.nranks > 1) || c->capturing || !allow || c->ov_final ||
        c->ov_slot[0].state >= 2 || c->ov_slot[1].state >= 2)
        return lv;
    for (hipEvent_t &e : slot.ev)
        if (!e && hipEventCreate(&e) != hipSuccess) return lv;
    probe = slot.state + 1;
    return probe;   // (probe 1: level 1, in sequence; probe 2: level 2, overlapped)
}
// probe's start (end = false) or end event on the context stream; the end advances the kind's slot
static int ov_mark(ocn_ctx *c, int kind, int probe, bool end)
{
    if (!probe) return OCN_OK;
    ocn_ctx::OvSlot &slot = c->ov_slot[kind == 4];
    HIPCHK(hipEventRecord(slot.ev[2 * (probe - 1) + (end ? 1 : 0)], c->stream));
    if (end) {
        slot.state = probe;
        c->ov_kind = kind;
        ++c->ov_probes;
    }
    return OCN_OK;
}
static void ov_reset(ocn_ctx *c)   // (OCN_OPT_OVERLAP set: measured again)
{
    c->ov_slot[0].state = c->ov_slot[1].state = 0;
    c->ov_final = c->ov_kind = c->ov_votes = 0;
    c->ov_level = 2;
}

// ------------------------------------------------------------------ stages (envoke)
// sync lists: interface/shallow_water/sw_interface.f90 envoke_*_sync
static const std::vector<int> kSyncSsh = {OCN_SSHN};
static const std::vector<int> kSyncHhUpdate = {OCN_HHU_N, OCN_HHV_N, OCN_HHH_N};
static const std::vector<int> kSyncVort = {OCN_VORT};
static const std::vector<int> kSyncUvTrans = {OCN_HHU_P, OCN_HHV_P, OCN_HHH_P};
static const std::vector<int> kSyncStress = {OCN_STR_T, OCN_STR_S};
static const std::vector<int> kSyncUv = {OCN_VBRTRN, OCN_UBRTRN};
static const std::vector<int> kSyncHhInit = {OCN_HHU, OCN_HHV, OCN_HHH};
// role-flip steps with halo exchanges: halo values that must equal the neighbours' (ocn_ctx.hip
// check_coherence)
static const std::vector<int> kHaloCheck = {OCN_SSH, OCN_UBRTR, OCN_VBRTR, OCN_HHU, OCN_HHV, OCN_HHQ_REST};

static int stage_kernel(ocn_ctx *c, const LBlock &b, int stage, double tau)
{
    const ocn_block *g = &b.g;
    void *s = c->stream;
    if (c->compact) {   // the compact tables (prepare_static): mask bytes and row metrics
        const Compact t{b.bits, b.rows, c->march};
        return launch_stage(g, b.ptr.data(), (int)b.ptr.size(), &t, stage, c->sw, tau, c->d_nbad, c->stream);
    }
#define R4(id) b.f<const float>(id)
#define R8(id) b.f<double>(id)
    switch (stage) {
    case OCN_STAGE_SW_UPDATE_SSH:
        return ocn_sw_update_ssh(g, tau, R4(OCN_LU), R4(OCN_DX), R4(OCN_DY), R4(OCN_DXH), R4(OCN_DYH),
                                 R8(OCN_HHU), R8(OCN_HHV), R8(OCN_SSHN), R8(OCN_SSHP), R8(OCN_UBRTR),
                                 R8(OCN_VBRTR), s);
    case OCN_STAGE_HH_UPDATE:
        return ocn_hh_update(g, R4(OCN_LU), R4(OCN_LLU), R4(OCN_LLV), R4(OCN_LUH), R4(OCN_DX), R4(OCN_DY),
                             R4(OCN_DXT), R4(OCN_DYT), R4(OCN_DXH), R4(OCN_DYH), R4(OCN_DXB), R4(OCN_DYB),
                             R8(OCN_HHQ_N), R8(OCN_HHU_N), R8(OCN_HHV_N), R8(OCN_HHH_N), R8(OCN_SSH),
                             R8(OCN_HHQ_REST), s);
    case OCN_STAGE_UV_TRANS_VORT:
        return ocn_uv_trans_vort(g, R4(OCN_LUU), R4(OCN_DXT), R4(OCN_DYT), R4(OCN_DXB), R4(OCN_DYB),
                                 R8(OCN_UBRTR), R8(OCN_VBRTR), R8(OCN_VORT), s);
    case OCN_STAGE_UV_TRANS:
        return ocn_uv_trans(g, R4(OCN_LCU), R4(OCN_LCV), R4(OCN_LUU), R4(OCN_DXH), R4(OCN_DYH), R8(OCN_UBRTR),
                            R8(OCN_VBRTR), R8(OCN_VORT), R8(OCN_HHQ), R8(OCN_HHU), R8(OCN_HHV), R8(OCN_HHH),
                            R8(OCN_RHSX_ADV), R8(OCN_RHSY_ADV), s);
    case OCN_STAGE_STRESS_COMPONENTS:
        return ocn_stress_components(g, R4(OCN_LU), R4(OCN_LUU), R4(OCN_DX), R4(OCN_DY), R4(OCN_DXT),
                                     R4(OCN_DYT), R4(OCN_DXH), R4(OCN_DYH), R4(OCN_DXB), R4(OCN_DYB),
                                     R8(OCN_UBRTRP), R8(OCN_VBRTRP), R8(OCN_STR_T), R8(OCN_STR_S), s);
    case OCN_STAGE_UV_DIFF2:
        return ocn_uv_diff2(g, R4(OCN_LCU), R4(OCN_LCV), R4(OCN_DX), R4(OCN_DY), R4(OCN_DXT), R4(OCN_DYT),
                            R4(OCN_DXH), R4(OCN_DYH), R4(OCN_DXB), R4(OCN_DYB), R8(OCN_MU), R8(OCN_STR_T),
                            R8(OCN_STR_S), R8(OCN_HHQ), R8(OCN_HHU), R8(OCN_HHV), R8(OCN_HHH), R8(OCN_RHSX_DIF),
                            R8(OCN_RHSY_DIF), s);
    case OCN_STAGE_SW_UPDATE_UV:
        return ocn_sw_update_uv(g, tau, R4(OCN_LCU), R4(OCN_LCV), R4(OCN_DXT), R4(OCN_DYT), R4(OCN_DXH),
                                R4(OCN_DYH), R4(OCN_DXB), R4(OCN_DYB), R8(OCN_HHU), R8(OCN_HHU_N), R8(OCN_HHU_P),
                                R8(OCN_HHV), R8(OCN_HHV_N), R8(OCN_HHV_P), R8(OCN_HHH), R8(OCN_SSH),
                                R8(OCN_UBRTR), R8(OCN_UBRTRN), R8(OCN_UBRTRP), R8(OCN_VBRTR), R8(OCN_VBRTRN),
                                R8(OCN_VBRTRP), R4(OCN_R_DISS), R4(OCN_RLH_S), R8(OCN_RHSX), R8(OCN_RHSY),
                                R8(OCN_RHSX_ADV), R8(OCN_RHSY_ADV), R8(OCN_RHSX_DIF), R8(OCN_RHSY_DIF), s);
    case OCN_STAGE_SW_NEXT_STEP:
        return ocn_sw_next_step(g, c->sw.time_smooth, R4(OCN_LU), R4(OCN_LCU), R4(OCN_LCV), R8(OCN_SSH),
                                R8(OCN_SSHN), R8(OCN_SSHP), R8(OCN_UBRTR), R8(OCN_UBRTRN), R8(OCN_UBRTRP),
                                R8(OCN_VBRTR), R8(OCN_VBRTRN), R8(OCN_VBRTRP), s);
    case OCN_STAGE_HH_SHIFT:
        return ocn_hh_shift(g, c->sw.time_smooth, R4(OCN_LU), R4(OCN_LLU), R4(OCN_LLV), R4(OCN_LUH),
                            R8(OCN_HHQ), R8(OCN_HHQ_P), R8(OCN_HHQ_N), R8(OCN_HHU), R8(OCN_HHU_P), R8(OCN_HHU_N),
                            R8(OCN_HHV), R8(OCN_HHV_P), R8(OCN_HHV_N), R8(OCN_HHH), R8(OCN_HHH_P), R8(OCN_HHH_N), s);
    case OCN_STAGE_HH_INIT:
        return ocn_hh_init(g, c->sw.full_free_surface, R4(OCN_LU), R4(OCN_LLU), R4(OCN_LLV), R4(OCN_LUH),
                           R4(OCN_DX), R4(OCN_DY), R4(OCN_DXT), R4(OCN_DYT), R4(OCN_DXH), R4(OCN_DYH), R4(OCN_DXB),
                           R4(OCN_DYB), R8(OCN_HHQ), R8(OCN_HHQ_P), R8(OCN_HHQ_N), R8(OCN_HHU), R8(OCN_HHU_P),
                           R8(OCN_HHU_N), R8(OCN_HHV), R8(OCN_HHV_P), R8(OCN_HHV_N), R8(OCN_HHH), R8(OCN_HHH_P),
                           R8(OCN_HHH_N), R8(OCN_SSH), R8(OCN_SSHP), R8(OCN_HHQ_REST), s);
    case OCN_STAGE_CHECK_SSH_ERR:
        return ocn_check_ssh_err(g, R4(OCN_LU), R8(OCN_SSH), c->d_nbad, s);
    default:
        return set_error(OCN_ERR_ARG, "unknown stage id");
    }
#undef R4
#undef R8
}

static const std::vector<int> *stage_sync(int stage)
{
    switch (stage) {
    case OCN_STAGE_SW_UPDATE_SSH: return &kSyncSsh;
    case OCN_STAGE_HH_UPDATE: return &kSyncHhUpdate;
    case OCN_STAGE_UV_TRANS_VORT: return &kSyncVort;
    case OCN_STAGE_UV_TRANS: return &kSyncUvTrans;
    case OCN_STAGE_STRESS_COMPONENTS: return &kSyncStress;
    case OCN_STAGE_SW_UPDATE_UV: return &kSyncUv;
    case OCN_STAGE_HH_INIT: return &kSyncHhInit;
    default: return nullptr;   // uv_diff2, sw_next_step, hh_shift, check: empty sync
    }
}

// every plan a step can use, built before any graph capture (no hipMalloc while capturing)
static int prebuild_plans(ocn_ctx *c)
{
    // fused-step sync groups (shallow_water.f90 syncs regrouped, see one_step_fused)
    const ocn_sw_params &sw = c->sw;
    c->sync_a = {OCN_SSHN};
    if (sw.full_free_surface > 0) c->sync_a.insert(c->sync_a.end(), {OCN_HHU_N, OCN_HHV_N, OCN_HHH_N});
    if (sw.trans_terms > 0) c->sync_a.push_back(OCN_VORT);
    if (sw.ksw_lat > 0) c->sync_a.insert(c->sync_a.end(), {OCN_STR_T, OCN_STR_S});
    c->sync_a_reuse.clear();
    for (int id : c->sync_a)
        if (id != OCN_HHU_N && id != OCN_HHV_N && id != OCN_HHH_N) c->sync_a_reuse.push_back(id);
    c->sync_b = {};
    if (sw.trans_terms > 0) c->sync_b = {OCN_HHU_P, OCN_HHV_P, OCN_HHH_P};
    c->sync_b.insert(c->sync_b.end(), {OCN_VBRTRN, OCN_UBRTRN});
    HaloPlan *p;
    RC(get_plan(c, c->sync_a, p));
    RC(get_plan(c, c->sync_a_reuse, p));
    RC(get_plan(c, c->sync_b, p));
    if (sw.use_tracers > 0) {
        RC(get_plan(c, {OCN_FLUX_X, OCN_FLUX_Y}, p));
        for (int k = 1; k <= sw.tracer_num; ++k) {
            RC(get_plan(c, {OCN_FF1N(k)}, p));
            RC(get_plan(c, {OCN_FF1(k)}, p));
        }
    }
    for (const std::vector<int> *l : {&kSyncSsh, &kSyncHhUpdate, &kSyncVort, &kSyncUvTrans, &kSyncStress, &kSyncUv,
                                      &kSyncHhInit, &kHaloCheck})
        RC(get_plan(c, *l, p));
    // role-flip steps: after hh_init + the next step's A, one exchange of both launches' fields
    c->sync_ca = kSyncHhInit;
    c->sync_ca.insert(c->sync_ca.end(), c->sync_a.begin(), c->sync_a.end());
    c->sync_ca_reuse = kSyncHhInit;
    c->sync_ca_reuse.insert(c->sync_ca_reuse.end(), c->sync_a_reuse.begin(), c->sync_a_reuse.end());
    RC(get_plan(c, c->sync_ca, p));
    RC(get_plan(c, c->sync_ca_reuse, p));
    // the same plans with the pairs' buffers swapped (role 1)
    if (c->role == 0) {
        swap_roles(c);
        const int rc = prebuild_plans(c);
        swap_roles(c);
        RC(rc);
    }
    return OCN_OK;
}

// Timer events (OCN_OPT_STAGE_TIMING) only measure: no system-scope fence when they are recorded --
// the default record writes back and invalidates the caches, which showed as a ~10 us gap before
// every timed launch (rocprofv3 kernel trace) and slowed the launch after it.  A pool is made when
// timing is switched on, so no event is created inside a timed region.
static int make_timer_event(hipEvent_t &e)
{
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    return OCN_OK;
}
int get_event(ocn_ctx *c, hipEvent_t &e)
{
    if (!c->event_pool.empty()) { e = c->event_pool.back(); c->event_pool.pop_back(); return OCN_OK; }
    return make_timer_event(e);
}

int timer_begin(ocn_ctx *c, int id, ocn_ctx::Rec &rec)
{
    rec = ocn_ctx::Rec{id, nullptr, nullptr};
    if (!c->stage_timing) return OCN_OK;
    RC(get_event(c, rec.a)); RC(get_event(c, rec.b));
    HIPCHK(hipEventRecord(rec.a, c->stream));
    return OCN_OK;
}
int timer_end(ocn_ctx *c, ocn_ctx::Rec &rec)
{
    if (!c->stage_timing) return OCN_OK;
    HIPCHK(hipEventRecord(rec.b, c->stream));
    c->recs.push_back(rec);
    return OCN_OK;
}

int envoke(ocn_ctx *c, int stage, double tau)
{
    ocn_ctx::Rec rec;
    RC(timer_begin(c, stage, rec));
    RC(each_block(c, c->stream, [&](const LBlock &b) { return stage_kernel(c, b, stage, tau); }));
    RC(timer_end(c, rec));
    const std::vector<int> *sl = stage_sync(stage);
    if (sl) RC(run_sync(c, *sl));
    return OCN_OK;
}

// expl_shallow_water (shallow_water.f90:22-94) with the flag gates
static int one_step(ocn_ctx *c, double tau, bool check)
{
    const ocn_sw_params &sw = c->sw;
    RC(envoke(c, OCN_STAGE_SW_UPDATE_SSH, tau));
    if (sw.full_free_surface > 0) RC(envoke(c, OCN_STAGE_HH_UPDATE, tau));
    if (sw.trans_terms > 0) {
        RC(envoke(c, OCN_STAGE_UV_TRANS_VORT, tau));
        RC(envoke(c, OCN_STAGE_UV_TRANS, tau));
    }
    if (sw.ksw_lat > 0) {
        RC(envoke(c, OCN_STAGE_STRESS_COMPONENTS, tau));
        RC(envoke(c, OCN_STAGE_UV_DIFF2, tau));
    }
    RC(envoke(c, OCN_STAGE_SW_UPDATE_UV, tau));
    RC(envoke(c, OCN_STAGE_SW_NEXT_STEP, tau));
    if (sw.full_free_surface > 0) {
        RC(envoke(c, OCN_STAGE_HH_SHIFT, tau));
        RC(envoke(c, OCN_STAGE_HH_INIT, tau));
    }
    if (check) RC(envoke(c, OCN_STAGE_CHECK_SSH_ERR, tau));
    return OCN_OK;
}

// Fused step (sw_kernels.hip "fused step groups"): 4 launches and 3 halo syncs per step,
// bitwise the same state as one_step.  last = false skips stores no later kernel reads
// (sw_stencils.h FusedB / HhInit `full`); the last step of every ocn_ctx_step call leaves the
// full state.
//
// With halo exchanges to do (several blocks or ranks) and OCN_OPT_OVERLAP, each exchange runs
// on the comm stream while the compute stream works on points that neither feed it nor read
// its halos (sw_stencils.h frame_rects):
//   A.frame | fork: sync A || A.inner, B.inner | join | B.frame | fork: sync B || C1.inner |
//   join | C1.frame | C2.frame | fork: sync C2 || C2.inner | join
// Every halo write of an exchange lands on points the concurrent inner launches neither read
// nor write, and every value it sends was produced by the frame launch before the fork.
// Whether any exchange has strips: some local block has a neighbour block (local or on another
// rank) in one of the 8 directions -- exactly when plan_entries enumerates an entry.  Decided from
// the decomposition alone (no plan is built, so nothing can fail inside a graph capture).
bool has_exchange(const ocn_ctx *c)
{
    for (const LBlock &b : c->blocks)
        for (int d = 0; d < 8; ++d)
            if (b.nbr_rank[d] >= 0) return true;
    return false;
}

// An exchange forked onto the comm stream stays pending until join_sync (a no-op without one);
// a role-flip step may leave its last exchange pending for the next step's inner launch.
static int fork_sync(ocn_ctx *c, const std::vector<int> &fields)
{
    HIPCHK(hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(hipStreamWaitEvent(c->comm_stream, c->ev_fork, 0));
    RC(run_sync(c, fields, c->comm_stream));
    HIPCHK(hipEventRecord(c->ev_join, c->comm_stream));
    c->sync_pending = true;
    return OCN_OK;
}
static int join_sync(ocn_ctx *c)
{
    if (!c->sync_pending) return OCN_OK;
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    c->sync_pending = false;
    return OCN_OK;
}

// Block b's compact tables (prepare_static) as a launch's `cp` argument, nullptr while the context
// does not use them (the 2-D real(4) arrays then; the one-pass forms run only with the tables).  The
// value lives to the end of the call expression it is written in; the launches copy what they need.
struct CompactArg {
    Compact t;
    bool on;
    operator const Compact *() const { return on ? &t : nullptr; }
};
static CompactArg compact_of(const ocn_ctx *c, const LBlock &b)
{
    return CompactArg{Compact{b.bits, b.rows, c->march}, c->compact};
}
// block b's launch arguments: geometry, field table, compact tables (or nullptr)
#define FT(b) &(b).g, (b).ptr.data(), (int)(b).ptr.size(), compact_of(c, b)
// The buffer pairs whose roles a role-flip step swaps (a8's copies ssh := sshn etc.)
static const int kFlipPairs[3][2] = {{OCN_SSH, OCN_SSHN}, {OCN_UBRTR, OCN_UBRTRN}, {OCN_VBRTR, OCN_VBRTRN}};
void swap_roles(ocn_ctx *c)
{
    for (LBlock &b : c->blocks)
        for (const auto &pr : kFlipPairs) std::swap(b.ptr[field_slot(pr[0])], b.ptr[field_slot(pr[1])]);
    c->role ^= 1;
}
// recompute steps: sshp and its second buffer trade places (role bit 2)
static void swap_sshp(ocn_ctx *c)
{
    for (LBlock &b : c->blocks) std::swap(b.ptr[field_slot(OCN_SSHP)], b.sshp_alt);
    c->role ^= 2;
}
// one-pass steps: sshp, ubrtrp, vbrtrp and their second buffers trade places (role bit 4)
void swap_alt3(ocn_ctx *c)
{
    for (LBlock &b : c->blocks) {
        std::swap(b.ptr[field_slot(OCN_SSHP)], b.sshp_alt);
        std::swap(b.ptr[field_slot(OCN_UBRTRP)], b.up_alt);
        std::swap(b.ptr[field_slot(OCN_VBRTRP)], b.vp_alt);
    }
    c->role ^= 4;
}
// tracer steps (run_tracer_step): every tracer's ff1 and ff1n trade places (role bit 8, the role-flip
// form of tracer_next_step's ff := ffn), and ff1p with its second buffer (role bit 16)
static void swap_tracer_roles(ocn_ctx *c)
{
    for (LBlock &b : c->blocks)
        for (int k = 1; k <= c->sw.tracer_num; ++k)
            std::swap(b.ptr[field_slot(OCN_FF1(k))], b.ptr[field_slot(OCN_FF1N(k))]);
    c->role ^= 8;
}
static void swap_tracer_alt(ocn_ctx *c)
{
    for (LBlock &b : c->blocks)
        for (int k = 1; k <= c->sw.tracer_num; ++k) std::swap(b.ptr[field_slot(OCN_FF1P(k))], b.ffp_alt[(size_t)k - 1]);
    c->role ^= 16;
}
// "The second buffers start as copies": for every block, whole arrays, on the context stream -- the
// second buffers of the first nsw of sshp, ubrtrp, vbrtrp (3: the one-pass steps', 1: the recompute
// steps' sshp), and with `tracers` every tracer's second ff1p buffer := the field's current buffer
static int copy_to_alt(ocn_ctx *c, int nsw, bool tracers)
{
    for (LBlock &b : c->blocks) {
        const std::pair<void *, int> sw[3] = {{b.sshp_alt, OCN_SSHP}, {b.up_alt, OCN_UBRTRP}, {b.vp_alt, OCN_VBRTRP}};
        for (int i = 0; i < nsw; ++i)
            HIPCHK(hipMemcpyAsync(sw[i].first, b.ptr[field_slot(sw[i].second)], field_bytes(b), hipMemcpyDeviceToDevice,
                                  c->stream));
        for (int t = 1; tracers && t <= c->sw.tracer_num; ++t)
            HIPCHK(hipMemcpyAsync(b.ffp_alt[(size_t)t - 1], b.ptr[field_slot(OCN_FF1P(t))], field_bytes(b),
                                  hipMemcpyDeviceToDevice, c->stream));
    }
    return OCN_OK;
}
// a8's copies as the call's last step leaves them (sshn := ssh, ubrtrn := ubrtr, vbrtrn := vbrtr, whole
// arrays: the new state is in the first buffers, both buffers of each pair end equal)
static int copy_pairs(ocn_ctx *c)
{
    for (const LBlock &b : c->blocks)
        for (const auto &pr : kFlipPairs)
            HIPCHK(hipMemcpyAsync(b.ptr[field_slot(pr[1])], b.ptr[field_slot(pr[0])], field_bytes(b),
                                  hipMemcpyDeviceToDevice, c->stream));
    return OCN_OK;
}
static bool is_flip_field(int id)
{
    for (const auto &pr : kFlipPairs)
        if (id == pr[0] || id == pr[1]) return true;
    return id >= OCN_TRACER_BASE && (id - OCN_TRACER_BASE) % 3 != 1;   // a tracer's ff1 / ff1n (tracer steps)
}

// Whether role-flip steps are exact for the current state (synchronises):
//  - the pairs agree outside their write sets (sw_stencils.h Coherence);
//  - with halo exchanges, the halo ring of ssh / ubrtr / vbrtr, hhu / hhv and hhq_rest holds the
//    neighbours' values (what an exchange would deliver; compared, not written).  After a swap
//    the new ssh holds the exchanged sshn on the whole ring, where a8 copies only under lu (so the
//    land points of the ring must already agree), and the fused hh_init + A launch takes hh_init's
//    own ring values where the standard step takes the exchanged ones.
// Every rank must run the same kind of step (the exchanges differ), so with RCCL the verdicts
// are max-reduced over the ranks; eligible = false: this rank cannot run role-flip steps at all.
// The vote also carries the other per-rank conditions that decide which launches and exchanges a
// call runs (one 0/1 word each, max-reduced = OR over the ranks): every rank then takes the same
// one-pass / hybrid decisions, so the exchange sequences of all ranks match.
// kVoteX4: this rank cannot run one_step_x4's pairs (its tables, or the known-constant verdict its host
// has read for the x2 range) -- every rank then runs the same steps and exchanges
// kVoteOvSeq / kVoteOvOv (+ 2 for the x4 pairs' slot): the measured sequential / overlapped step times
// of the x2 steps in us (ov_begin; INT32_MAX from a rank that has not measured both: no decision from
// that kind)
enum { kVoteIncoherent = 0, kVoteIneligible, kVoteUdiv, kVoteHhStale, kVoteX2, kVoteX4, kVoteOvSeq, kVoteOvOv,
       kVoteOvSeq4, kVoteOvOv4, kVoteUsed };
static_assert(kVoteOvSeq4 == kVoteOvSeq + 2 && kVoteOvOv4 == kVoteOvOv + 2, "the overlap slots' vote words");
static_assert(kVoteUsed <= kVoteWords, "vote words");
struct VoteIn { bool eligible, udiv_ok, hh_consistent, x2_ok, x4_ok, nv_ok; };
struct VoteOut { bool udiv_ok, hh_consistent, x2_ok, x4_ok; };

// one_step_x2's condition on the state's halo points that no exchange fills (the rings 1 and 2 of a
// side, or corner, without a neighbour block): +0.0 in the six state arrays.  The reference never
// writes them (no a8 / a9 work on such a ring: ocn_ctx::edge_ring_sea) and init leaves +0.0 there;
// a neighbour's D formed next to such a point reads the neighbour's own copy of it, which then
// holds +0.0 as well (every rank checks and the verdicts are reduced).  ORs 1 into *flag otherwise.
// The same at the points of the outer halo ring (nx_end + 1, ny_end + 1) no neighbour fills for the
// nine depth arrays of hh_shift's u / v / h triples (a9's own arrays there: hh_init and hh_update
// stop at nx_end / ny_end): +0.0 makes a9 there an exact no-op (0 + ts (0 - 0 + 0) / 2 = +0), which
// the x2 steps then skip; the hybrid last step runs it as the reference does.
struct HaloZero {
    const double *a[6], *d[9];
    int w, h, nxs, nxe, nys, nye, bx1, by1;
    long pitch;
    unsigned own;
};
__global__ void k_halo_zero(HaloZero q, int32_t *flag)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)q.w * q.h) return;
    const int m = q.bx1 + (int)(i % q.w), n = q.by1 + (int)(i / q.w);
    const unsigned cx = m < q.nxs ? 0u : m > q.nxe ? 2u : 1u, cy = n < q.nys ? 0u : n > q.nye ? 2u : 1u;
    if ((cx == 1u && cy == 1u) || ((q.own >> (cx * 3u + cy)) & 1u)) return;   // interior, or a neighbour's
    const long at = (i % q.w) + (i / q.w) * q.pitch;
    auto nz = [&](const double *p) {
        unsigned long long x;
        const double v = p[at];
        __builtin_memcpy(&x, &v, 8);
        return x != 0ull;
    };
    bool bad = false;
    for (int k = 0; k < 6; ++k) bad |= nz(q.a[k]);
    const bool outer = (m == q.nxe + 1 && n >= q.nys - 1 && n <= q.nye + 1) ||
                       (n == q.nye + 1 && m >= q.nxs - 1 && m <= q.nxe + 1);
    if (outer)
        for (int k = 0; k < 9; ++k) bad |= nz(q.d[k]);
    if (bad) atomicOr(flag, 1);
}
static int launch_halo_zero(ocn_ctx *c, int32_t *flag)
{
    static const int ids[6] = {OCN_SSH, OCN_SSHP, OCN_UBRTR, OCN_UBRTRP, OCN_VBRTR, OCN_VBRTRP};
    static const int dids[9] = {OCN_HHU, OCN_HHU_P, OCN_HHU_N, OCN_HHV, OCN_HHV_P, OCN_HHV_N, OCN_HHH, OCN_HHH_P, OCN_HHH_N};
    for (const LBlock &b : c->blocks) {
        HaloZero q{};
        for (int k = 0; k < 6; ++k) q.a[k] = b.f<double>(ids[k]);
        for (int k = 0; k < 9; ++k) q.d[k] = b.f<double>(dids[k]);
        q.w = b.g.bnd_x2 - b.g.bnd_x1 + 1; q.h = b.g.bnd_y2 - b.g.bnd_y1 + 1;
        q.nxs = b.g.nx_start; q.nxe = b.g.nx_end; q.nys = b.g.ny_start; q.nye = b.g.ny_end;
        q.bx1 = b.g.bnd_x1; q.by1 = b.g.bnd_y1; q.pitch = (long)b.g.pitch; q.own = b.own;
        const long pts = (long)q.w * q.h;
        hipLaunchKernelGGL(k_halo_zero, dim3((unsigned)((pts + 255) / 256)), dim3(256), 0, c->stream, q, flag);
        RC(check_launch());
    }
    return OCN_OK;
}

static int check_coherence(ocn_ctx *c, const VoteIn &in, VoteOut &out)
{
    int32_t host[kVoteWords] = {0};
    host[kVoteIneligible] = !in.eligible;
    host[kVoteUdiv] = !in.udiv_ok;
    host[kVoteHhStale] = !in.hh_consistent;
    host[kVoteX2] = !in.x2_ok;
    // (one word, reduced by maximum: 2 = no pairs here, 1 = pairs but not their inviscid bodies, 0 = both)
    host[kVoteX4] = !in.x4_ok ? 2 : !in.nv_ok ? 1 : 0;
    // the measured overlap choice, while it is open (OCN_OPT_OVERLAP auto, peers on other ranks)
    const bool ov_open = c->overlap < 0 && has_comm(c) && c->dec.nranks > 1 && !c->ov_final;
    for (int sl = 0; sl < 2; ++sl) {
        host[kVoteOvSeq + 2 * sl] = host[kVoteOvOv + 2 * sl] = INT32_MAX;
        const ocn_ctx::OvSlot &slot = c->ov_slot[sl];
        if (!ov_open || slot.state != 2) continue;
        float ms[2] = {0.f, 0.f};   // both probe steps recorded (ov_begin): their times, in us
        HIPCHK(hipEventSynchronize(slot.ev[3]));
        HIPCHK(hipEventElapsedTime(&ms[0], slot.ev[0], slot.ev[1]));
        HIPCHK(hipEventElapsedTime(&ms[1], slot.ev[2], slot.ev[3]));
        for (int i = 0; i < 2; ++i)
            host[kVoteOvSeq + 2 * sl + i] = (int32_t)std::min(1.0e9, std::max(1.0, std::round(1000.0 * ms[i])));
    }
    HIPCHK(hipMemcpyAsync(c->d_flags, host, sizeof(host), hipMemcpyHostToDevice, c->stream));
    if (in.eligible)
        RC(each_block(c, c->stream, [&](const LBlock &b) { return launch_coherence(&b.g, b.ptr.data(), b.bits, c->d_flags, c->stream); }));
    if (in.eligible && c->sw.use_tracers > 0 && c->tr_step)   // the tracer steps' ff1 / ff1n pairs too
        for (int t = 1; t <= c->sw.tracer_num; ++t)
            RC(each_block(c, c->stream, [&](const LBlock &b) {
                return launch_tracer_coherence(&b.g, b.ptr.data(), b.bits, t, c->d_flags, c->stream);
            }));
    const bool exch = has_exchange(c);
    if (exch) RC(run_sync(c, kHaloCheck, c->stream, c->d_flags));
    if (exch && c->x2) {   // one_step_x2: the rest of the state's first halo ring, and the unexchanged halos
        RC(run_sync(c, {OCN_SSHP, OCN_UBRTRP, OCN_VBRTRP}, c->stream, c->d_flags + kVoteX2));
        // tracer steps form tran_diff_fluxes' fluxes at the halo points neighbours own (the reference
        // exchanges them) from mu there: its first halo ring must hold the neighbours' values too
        if (c->sw.use_tracers > 0 && c->tr_step) RC(run_sync(c, {OCN_MU}, c->stream, c->d_flags + kVoteX2));
        RC(launch_halo_zero(c, c->d_flags + kVoteX2));
    }
    RC(allreduce_max(c, c->d_flags, c->stream, kVoteUsed));
    int32_t w[kVoteWords] = {0};
    HIPCHK(hipMemcpyAsync(w, c->d_flags, sizeof(int32_t) * kVoteUsed, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->coherent = w[kVoteIncoherent] == 0 && w[kVoteIneligible] == 0;
    c->coherent_known = !c->r8_escaped && !has_comm(c);
    out.udiv_ok = w[kVoteUdiv] == 0;
    out.hh_consistent = w[kVoteHhStale] == 0;
    out.x2_ok = w[kVoteX2] == 0 && exch && c->x2;
    c->x2_dev_ok = out.x2_ok;
    out.x4_ok = out.x2_ok && w[kVoteX4] < 2;
    // every rank takes the same decision from the reduced words: the first kind (x2 steps, then x4
    // pairs) every rank has measured in both forms decides, the faster form wins; a kind some rank has
    // not measured is measured again, together; kOvMaxVotes votes without a decision end the choice
    for (int sl = 0; sl < 2 && ov_open && !c->ov_final; ++sl) {
        const int32_t seq = w[kVoteOvSeq + 2 * sl], ovl = w[kVoteOvOv + 2 * sl];
        if (seq != INT32_MAX && ovl != INT32_MAX) {
            c->ov_ms[0] = 1.0e-3 * seq;
            c->ov_ms[1] = 1.0e-3 * ovl;
            c->ov_level = ovl < seq ? 2 : 1;
            c->ov_kind = sl ? 4 : 2;
            c->ov_final = 3;
        } else if (c->ov_slot[sl].state == 2) {
            c->ov_slot[sl].state = 0;
        }
    }
    if (ov_open && !c->ov_final && ++c->ov_votes >= kOvMaxVotes) {
        c->ov_final = 4;
        c->ov_level = 2;
    }
    c->x4_dev_ok = out.x4_ok;
    c->nv_dev_ok = w[kVoteX4] == 0;   // every rank's pairs run the inviscid bodies, or none's
    return OCN_OK;
}

// Role-flip steps: the step's a8 copies (ssh := sshn, ubrtr := ubrtrn, vbrtr := vbrtrn on the
// interior and the ring, under the masks) become a swap of the two buffers of each pair, and
// a8's time filters and check_ssh_err move into fused B (sw_kernels.hip MarchFusedB<true>), so
// the step is A | B+a8 | a8+a9 on the ring | swap | hh_init -- one full pass (C1) fewer.  Exact
// when the pairs are coherent (sw_stencils.h Coherence): inside the write sets the reference
// leaves both buffers of a pair equal to the new value, and the buffer that becomes "sshn" /
// "ubrtrn" / "vbrtrn" after the swap holds the old value there instead -- which no kernel
// reads before a1 / a7 of the next step rewrite it.  The last step of every call is a standard
// step; it leaves both buffers of each pair equal everywhere, so the swap is undone at the end
// of the call by swapping the pointers back, with no copy.  Used with the compact tables + march,
// tracer runs included (CA then also stores hh_init's hhq_p, which expl_tracer reads after every
// step).  With halo exchanges the swapped buffers are exchanged through plans built for the
// swapped roles (get_plan), the ring launch (a8 + a9 on the halo ring) runs after sync B, and
// each hh_init's sync and the next step's sync A are one exchange (sync_ca); the exchanges do
// not overlap computation in these steps.
// (the condition: ocn_step_plan.h flip_eligible)

// The reuse steps (sw_stencils.h) leave hh_update's n-level depths unexchanged: a9 then forms the
// p levels on the halo ring from stale values, which is harmless only because uv_trans's exchange of
// hhu_p / hhv_p / hhh_p rewrites them before the call ends.  With trans_terms = 0 the reference makes
// no such exchange and a9's ring values stay in the arrays, so with neighbours (other blocks or
// ranks: the same answer on every rank) each step is a standard fused step with hh_update and its
// exchange -- no reuse steps and no role-flip steps (whose fused hh_init + A is a reuse step's).
static bool reuse_allowed(const ocn_ctx *c)
{
    return c->sw.trans_terms > 0 || !(has_exchange(c) || has_comm(c));
}

// tracer steps (run_tracer_step, below): the pending one of the current state, and the tracer fields
// the exchanges of a one-pass call carry with the state
static int run_tracer_step(ocn_ctx *c, double tau);
static int run_tracer_step(ocn_ctx *c, double tau, hipStream_t st);
static int tracer_step_block(ocn_ctx *c, const LBlock &b, int k, double tau, hipStream_t st);
static std::vector<int> with_tracers(const ocn_ctx *c, const std::vector<int> &fields);

// The part of block b's interior the one-pass step covers when halos are exchanged: the interior
// less w points on each side that has a neighbour block -- E, W, N, S, or a diagonal one of that
// side: a diagonal neighbour receives this block's interior corner point (CA's stored depths in
// sync CA), so that point must lie in a frame band.  In a grid without holes a diagonal neighbour
// comes with both side neighbours; where all-land blocks were dropped it may be the only one at
// its corner, and the corner then stayed in the inner march, which stores no depths: the
// neighbour's corner halo of hhu / hhv / hhh's p and n levels kept stale values after the
// hybrid last step.
static bool side_fed(const LBlock &b, int side)   // side: 1 E, 2 W, 3 N, 4 S (kDirDm / kDirDn)
{
    static const int diag[5][2] = {{0, 0}, {5, 6}, {7, 8}, {5, 7}, {6, 8}};   // E: NE SE, W: NW SW, N: NE NW, S: SE SW
    return b.nbr_rank[side - 1] >= 0 || b.nbr_rank[diag[side][0] - 1] >= 0 || b.nbr_rank[diag[side][1] - 1] >= 0;
}
// (every inner range of a step form: the hybrid steps' 1- and 2-point frames, the x2 steps' and the x4
// pairs' bands -- ew columns off each fed E / W side, ns rows off each fed N / S side)
static Range inner_range(const LBlock &b, int ew, int ns)
{
    Range r{b.g.nx_start, b.g.nx_end, b.g.ny_start, b.g.ny_end};
    if (side_fed(b, 2)) r.m0 += ew;
    if (side_fed(b, 1)) r.m1 -= ew;
    if (side_fed(b, 4)) r.n0 += ns;
    if (side_fed(b, 3)) r.n1 -= ns;
    return r;
}
// The E / W bands of an x2 step or x4 pair: `tile` columns -- what one wave (kX2BandCols) or pair
// workgroup (kX4BandCols) marches whatever the band's width, so the wider band takes them off the
// inner launch for nothing -- where the block is at least three of them wide, else the exchange's depth
static int band_cols(const LBlock &b, int tile, int depth)
{
    return b.g.nx_end - b.g.nx_start + 1 >= 3 * tile ? tile : depth;
}

// A one-pass step with halo exchanges (several blocks or ranks), or with a8 / a9 work on the
// halo ring.  The one-pass march needs D (hh_init's depths, vort, stresses) at the points next to
// the ones it updates, formed from the state one point further out; at a halo the reference holds
// D as exchanged from the neighbour, which would need the neighbour's state TWO points out -- the
// reference never exchanges that.  So the points one away from an exchanged side take the
// role-flip path (D stored by CA, exchanged, read back by B) and the rest the one-pass march:
//   CA frame (hh_init of the previous step + this step's A, on the bands two points deep along
//   the exchanged sides and their halos) | sync CA | B on the one-point bands | sync B, as a side
//   chain on the comm stream beside the one-pass march of the inner part on the compute stream |
//   join | swap | ring launch (a8 + a9 on the halo ring).  With OCN_OPT_OVERLAP 0 (or while
//   capturing a graph) the same launches run in that order on one stream, the inner march
//   between sync CA and B.  (The side chain is the overlap of every level >= 1: with local copies
//   too it hides the latency-bound frame launches -- one GPU, 4x2 blocks of a 4096^2 box: 0.947
//   -> 0.856 ms per step, 2x2 of 2048^2: 0.334 -> 0.294; the earlier split of the inner march
//   into two halves beside the two exchanges took 1.065 / 0.398.)
// All of a8's filtered sshp / ubrtrp / vbrtrp go to the second buffers (the inner part reads the
// current ones at neighbours); the ring launch reads the current ones and writes the new ones on
// the ring after the swap, as the recompute steps do with sshp.
static int hybrid_tail(ocn_ctx *c, double tau, const StepKind &k, bool last);
// last: the call's last step (StepKind::one_last with exchanges or ring work): the CA frames' A
// stores hh_update's levels and sync CA exchanges them (the halo values the reference's a2 sync
// leaves and its a9 on the halo ring reads), the inner march also stores vort, the stresses and
// the RHS terms (MarchStep<.., true>), B on the bands keeps the RHS terms (fused B `full`), and the
// tail adds a8's copies and hh_init with every level + its sync
static int one_step_hybrid(ocn_ctx *c, double tau, const StepKind &k, bool last = false)
{
    const ocn_sw_params &sw = c->sw;
    ocn_ctx::Rec rec;
    int32_t *nbad = k.check ? c->d_nbad : nullptr;
    hipStream_t s = c->stream;
    const bool xch = has_exchange(c);
    // the previous step's hh_init and this step's A on the frames (bnd range outside inner_ca)
    auto ca_frames = [&](hipStream_t st) -> int {
        RC(each_block(c, st, [&](const LBlock &b) -> int {
            Range in = inner_range(b, 2, 2);
            if (!side_fed(b, 2)) in.m0 = b.g.bnd_x1;   // no frame on the sides without a neighbour
            if (!side_fed(b, 1)) in.m1 = b.g.bnd_x2;
            if (!side_fed(b, 4)) in.n0 = b.g.bnd_y1;
            if (!side_fed(b, 3)) in.n1 = b.g.bnd_y2;
            RC(launch_fused_ca(FT(b), OCN_PART_FRAME, sw, tau, !last, false,
                               st, &in));
            return OCN_OK;
        }));
        return OCN_OK;
    };
    // B on the one-point bands along the exchanged sides
    auto b_bands = [&](hipStream_t st) -> int {
        RC(each_block(c, st, [&](const LBlock &b) -> int {
            const Range in = inner_range(b, 1, 1);
            const Range all{b.g.nx_start, b.g.nx_end, b.g.ny_start, b.g.ny_end};
            if (in.m0 == all.m0 && in.m1 == all.m1 && in.n0 == all.n0 && in.n1 == all.n1) return OCN_OK;
            RC(launch_fused_b(FT(b), OCN_PART_ALL, sw, tau, last, true, st, nbad, true, false, (double *)b.sshp_alt,
                              (double *)b.up_alt, (double *)b.vp_alt, &in));
            return OCN_OK;
        }));
        return OCN_OK;
    };
    if (xch && overlap_level(c) >= 1 && !c->capturing) {
        // side chain (OCN_OPT_OVERLAP >= 1): CA frames | sync CA | B bands | sync B on the comm stream,
        // beside the whole inner march on the compute stream -- the two read nothing the other
        // writes (disjoint points; the inner march forms its D from the state, the bands read
        // CA's stored D and the exchanged halos), so the frame launches and both exchanges hide
        // behind it
        // The inner march is enqueued first (the fork event recorded before it): with several
        // blocks the host's enqueueing of the side chain's ~3 launches per block took longer than
        // the GPU's previous work, and the compute stream sat idle until it was done
        HIPCHK(hipEventRecord(c->ev_fork, s));
        RC(timer_begin(c, OCN_TIMER_ONEPASS, rec));
        RC(each_block(c, s, [&](const LBlock &b) -> int {
            const Range in = inner_range(b, 1, 1);
            RC(launch_onepass(FT(b), sw, tau, nbad, (double *)b.sshp_alt,
                              (double *)b.up_alt, (double *)b.vp_alt, s, &in, last, kc_of(c, b)));
            return OCN_OK;
        }));
        RC(timer_end(c, rec));
        HIPCHK(hipStreamWaitEvent(c->comm_stream, c->ev_fork, 0));
        RC(ca_frames(c->comm_stream));
        RC(run_sync(c, last ? c->sync_ca : c->sync_ca_reuse, c->comm_stream));
        RC(b_bands(c->comm_stream));
        RC(run_sync(c, c->sync_b, c->comm_stream));
        HIPCHK(hipEventRecord(c->ev_join, c->comm_stream));
        c->sync_pending = true;
        RC(join_sync(c));
        return hybrid_tail(c, tau, k, last);
    }
    // without overlap (or while capturing a graph): CA frames | sync CA | inner | B bands | sync B
    RC(timer_begin(c, OCN_TIMER_FUSED_CA, rec));
    RC(ca_frames(s));
    RC(timer_end(c, rec));
    if (xch) RC(run_sync(c, last ? c->sync_ca : c->sync_ca_reuse));
    RC(timer_begin(c, OCN_TIMER_ONEPASS, rec));
    RC(each_block(c, s, [&](const LBlock &b) -> int {
        const Range in = inner_range(b, 1, 1);
        RC(launch_onepass(FT(b), sw, tau, nbad, (double *)b.sshp_alt,
                          (double *)b.up_alt, (double *)b.vp_alt, s, &in, last, kc_of(c, b)));
        return OCN_OK;
    }));
    RC(timer_end(c, rec));
    if (xch) {
        RC(timer_begin(c, OCN_TIMER_FUSED_B, rec));
        RC(b_bands(s));
        RC(timer_end(c, rec));
        RC(run_sync(c, c->sync_b));
    }
    return hybrid_tail(c, tau, k, last);
}

// the end of a hybrid one-pass step (one_step_hybrid): the role swaps, the ring launch, and the
// next step's CA + sync before a standard last step -- or, on the call's last step, a8's copies
// (both buffers of each pair end equal, as one_step_last leaves them) and hh_init with every level
// (a10; the levels a9 and hh_update leave are rewritten by it on the same ranges) and its sync
static int hybrid_tail(ocn_ctx *c, double tau, const StepKind &k, bool last)
{
    const ocn_sw_params &sw = c->sw;
    ocn_ctx::Rec rec;
    hipStream_t s = c->stream;
    const bool xch = has_exchange(c);
    swap_alt3(c);
    std::vector<std::vector<void *>> pre;   // the ring launch's field tables (pair roles before the swap)
    for (const LBlock &b : c->blocks) pre.push_back(b.ptr);
    swap_roles(c);
    if (c->ring_sea) {   // a8 + a9 on the ring: the previous sshp / ubrtrp / vbrtrp in, the new ones out
        RC(timer_begin(c, OCN_TIMER_FUSED_C1, rec));
        for (size_t i = 0; i < c->blocks.size(); ++i) {
            const LBlock &b = c->blocks[i];
            RC(launch_fused_c1(&b.g, pre[i].data(), (int)pre[i].size(), compact_of(c, b), OCN_PART_FRAME, sw, nullptr, s,
                               (const double *)b.sshp_alt, (const double *)b.up_alt, (const double *)b.vp_alt));
        }
        RC(timer_end(c, rec));
    }
    if (last) {
        RC(copy_pairs(c));
        RC(timer_begin(c, OCN_STAGE_HH_INIT, rec));
        RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_c2(FT(b), OCN_PART_ALL, sw, true, s); }));
        RC(timer_end(c, rec));
        if (xch) RC(run_sync(c, *stage_sync(OCN_STAGE_HH_INIT)));
        return OCN_OK;
    }
    if (k.next_a) {   // the next step is the last, standard one: hh_init + its fused A, then their sync
        RC(timer_begin(c, OCN_TIMER_FUSED_CA, rec));
        RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_ca(FT(b), OCN_PART_ALL, sw, tau, k.next_reuse,
                               false, s); }));
        RC(timer_end(c, rec));
        if (xch) RC(run_sync(c, k.next_reuse ? c->sync_ca_reuse : c->sync_ca));
    }
    return OCN_OK;
}

// The last step of a single-block one-pass call (no exchange, no a8 / a9 work on the halo ring):
// the one-pass march that also stores vort, the stresses and the RHS terms (sw_kernels.hip
// MarchStep<.., true>), the role swaps, a8's copies (ssh := sshn, ubrtr := ubrtrn, vbrtr := vbrtrn:
// both buffers of each pair end equal, as the reference leaves them), then hh_init with every
// level (a10; a9's results on its range are rewritten by it).  Replaces CA + fused B + C1 +
// hh_init of the standard last step.
// what follows the last step's march (one block, no exchange; the roles swapped): a8's copies
// (ssh := sshn, ubrtr := ubrtrn, vbrtr := vbrtrn, whole arrays: both buffers of each pair end equal,
// as the reference leaves them) and hh_init with every level (a10, depth.f90:14-99)
static int last_finish(ocn_ctx *c)
{
    hipStream_t s = c->stream;
    ocn_ctx::Rec rec;
    // a8's copies sshn := ssh, ubrtrn := ubrtr, vbrtrn := vbrtr (the new state is in the first
    // buffers): in the hh_init march, which reads ssh anyway (one pass instead of three copies)
    auto copy_of = [](const LBlock &b) {
        auto p = [&](int id) { return (double *)b.ptr[field_slot(id)]; };
        return TailCopy{{p(OCN_SSH), p(OCN_UBRTR), p(OCN_VBRTR)}, {p(OCN_SSHN), p(OCN_UBRTRN), p(OCN_VBRTRN)}};
    };
    if (!c->march) RC(copy_pairs(c));
    // (not while capturing a graph: the replays would not see hn_fresh)
    const bool keep_n = c->hn_fresh && !c->capturing && !c->r8_handed && !c->r4_escaped;
    RC(timer_begin(c, OCN_STAGE_HH_INIT, rec));
    RC(each_block(c, s, [&](const LBlock &b) {
        const TailCopy tc = copy_of(b);
        return launch_fused_c2(FT(b), OCN_PART_ALL, c->sw, true, s, keep_n, c->march ? &tc : nullptr);
    }));
    RC(timer_end(c, rec));
    c->hn_fresh = !c->capturing;
    return OCN_OK;
}

static int one_step_last(ocn_ctx *c, double tau, const StepKind &k)
{
    const ocn_sw_params &sw = c->sw;
    ocn_ctx::Rec rec;
    hipStream_t s = c->stream;
    RC(timer_begin(c, OCN_TIMER_ONEPASS, rec));
    RC(each_block(c, s, [&](const LBlock &b) { return launch_onepass(FT(b), sw, tau, k.check ? c->d_nbad : nullptr,
                          (double *)b.sshp_alt, (double *)b.up_alt, (double *)b.vp_alt, s, nullptr, true,
                          kc_of(c, b)); }));
    RC(timer_end(c, rec));
    swap_alt3(c);
    swap_roles(c);
    return last_finish(c);
}

// ------------------------------------------------------------------ one-pass steps with one exchange
// With halo exchanges the reference holds D (hh_init's depths, vort, the stresses) at a halo as the
// neighbour formed it on its interior, from the neighbour's state one point further out -- two
// points into our halo.  one_step_x2 exchanges the state (ssh, sshp, ubrtr, ubrtrp, vbrtr, vbrtrp)
// two points deep once per step, so every block forms D on its halo itself (the same operands, the
// same arithmetic: sw_kernels.hip MarchStep X2, with the metric rows of the second ring from
// ext / rows_x and h_r's second ring from the h_r copy hr_x) and the one-pass march covers the whole
// interior: no CA / B frame launches and one exchange per step instead of two.  The state's first
// halo ring then holds the neighbours' values as the reference's a8 on the ring leaves it (checked
// in check_coherence); its second ring, which the reference never writes, is saved when a sequence
// of such steps starts and restored when it ends (x2_end, before the call's last step).
static const std::vector<int> kStateX2 = {OCN_SSH, OCN_SSHP, OCN_UBRTR, OCN_UBRTRP, OCN_VBRTR, OCN_VBRTRP};

static int ring2_run(ocn_ctx *c, bool save, hipStream_t s)
{
    for (const LBlock &b : c->blocks) RC(launch_segs(save ? b.save : b.restore, s));
    return OCN_OK;
}

// the end of a sequence of x2 steps: the second ring as the reference leaves it, the first ring of
// the current state exchanged (what the reference's exchanges and a8 on the ring leave there)
static int x2_end(ocn_ctx *c, hipStream_t s)
{
    RC(ring2_run(c, false, s));
    return run_sync(c, with_tracers(c, kStateX2), s);
}

// hr_x = h_r with the neighbours' second ring (the general variant of one_step_x2 reads it there) --
// four rings deep where x4 pairs may run (their h_r-read variant reads it on the block widened by
// kXRing rings, as the neighbours' own h_r); x4_tables: x4 pairs may run (their tables and the option)
static bool x4_tables(const ocn_ctx *c) { return c->x4 && c->x4_tab_ok; }
static int refresh_hrx(ocn_ctx *c)
{
    for (const LBlock &b : c->blocks)
        HIPCHK(hipMemcpyAsync(b.hr_x, b.ptr[field_slot(OCN_HHQ_REST)], field_bytes(b), hipMemcpyDeviceToDevice,
                              c->stream));
    auto swap_hr = [c] {
        for (LBlock &b : c->blocks) {
            void *t = b.ptr[field_slot(OCN_HHQ_REST)];
            b.ptr[field_slot(OCN_HHQ_REST)] = b.hr_x;
            b.hr_x = (double *)t;
        }
    };
    swap_hr();
    const int rc = run_sync(c, {OCN_HHQ_REST}, c->stream, nullptr, x4_tables(c) ? 4 : 2, 1);
    swap_hr();
    RC(rc);
    c->hrx_ok = true;
    return OCN_OK;
}

// every plan one_step_x2 and x2_end use, for the pair / second-buffer roles a call passes through
// (built before any graph capture)
static int prebuild_x2(ocn_ctx *c)
{
    int rc = OCN_OK;
    for (int i = 0; i < 4 && rc == OCN_OK; ++i) {
        if (i & 1) swap_roles(c);
        if (i & 2) swap_alt3(c);
        HaloPlan *p;
        rc = get_plan(c, kStateX2, p, 2);
        if (rc == OCN_OK) rc = get_plan(c, kStateX2, p, 1);
        if (rc == OCN_OK && c->x4 && c->x4_tab_ok) rc = get_plan(c, kStateX2, p, 4);   // (one_step_x4)
        if (i & 2) swap_alt3(c);
        if (i & 1) swap_roles(c);
    }
    return rc;
}

// The part of the interior an x2 step computes without the exchange: the interior less 2 points
// on every side a neighbour (diagonals included) fills halos of -- a point's stencil reaches the
// state 2 points away (D at +-1, formed from the state at +-1).
constexpr int kX2BandCols = 60;   // a one-pass wave's output columns (sw_kernels.hip MarchStep, kHalo 2)
static Range x2_inner(const LBlock &b) { return inner_range(b, band_cols(b, kX2BandCols, 2), 2); }

// An x2 step's or x4 pair's launches with the exchange overlapped (OCN_OPT_OVERLAP 2): inner(b) for
// every block on the compute stream, timed as `timer`; beside it on the comm stream the second ring's
// save (save: the first step of a sequence), the exchange of `fields` `depth` points deep, then bands(b)
// for every block (co: its launches may go as one, each_block); the join orders what follows after both.
// OCN_TIMER_EXPOSED: from the inner launches' end to the comm chain's end.
template <class Inner, class Bands>
static int overlapped_exchange(ocn_ctx *c, int timer, int depth, const std::vector<int> &fields, bool save,
                               Inner &&inner, Bands &&bands, bool co)
{
    hipStream_t s = c->stream;
    ocn_ctx::Rec rec;
    HIPCHK(hipEventRecord(c->ev_fork, s));
    RC(timer_begin(c, timer, rec));
    RC(each_block(c, s, inner));
    RC(timer_end(c, rec));
    ocn_ctx::Rec xrec{OCN_TIMER_EXPOSED, nullptr, nullptr};
    if (c->stage_timing) {
        RC(get_event(c, xrec.a)); RC(get_event(c, xrec.b));
        HIPCHK(hipEventRecord(xrec.a, s));
    }
    HIPCHK(hipStreamWaitEvent(c->comm_stream, c->ev_fork, 0));
    if (save) RC(ring2_run(c, true, c->comm_stream));
    RC(run_sync(c, fields, c->comm_stream, nullptr, depth));
    RC(each_block(c, c->comm_stream, bands, co));
    if (xrec.b) {
        HIPCHK(hipEventRecord(xrec.b, c->comm_stream));
        c->recs.push_back(xrec);
    }
    HIPCHK(hipEventRecord(c->ev_join, c->comm_stream));
    c->sync_pending = true;
    return join_sync(c);
}

// One x2 step.  With OCN_OPT_OVERLAP 2 (the default when the context exchanges with other ranks;
// not while capturing a graph): the inner part (x2_inner) on the compute stream beside the exchange
// and then the frame bands on the comm stream (which runs at the device's highest priority) -- the
// exchange's latency hides behind the inner march.  The two parts write disjoint points of the new
// state (other buffers than the ones read), the exchange writes halos only the frame reads; the join
// orders the next step after both.  With only local copies (one GPU) the exchange costs less than
// the extra frame launch: one GPU, 4x2 blocks of 4096^2, 0.482 ms per step in sequence against
// 0.521 overlapped; 2x2 of 2048^2 0.154 against 0.170.
static int one_step_x2(ocn_ctx *c, double tau, const StepKind &k)
{
    const ocn_sw_params &sw = c->sw;
    hipStream_t s = c->stream;
    ocn_ctx::Rec rec;
    int32_t *nbad = k.check ? c->d_nbad : nullptr;
    auto march = [&](const LBlock &b, hipStream_t st, const Range *range, const Range *frame_of) -> int {
        std::vector<void *> tab = b.ptr;
        tab[field_slot(OCN_HHQ_REST)] = b.hr_x;
        const Compact t{b.bits, b.rows_x, c->march};
        return launch_onepass(&b.g, tab.data(), (int)tab.size(), &t, sw, tau, nbad, (double *)b.sshp_alt,
                              (double *)b.up_alt, (double *)b.vp_alt, st, range, false, kc_of(c, b), b.own, frame_of);
    };
    // OCN_OPT_CO_LAUNCH: the previous state's tracer step in a march launch after the exchange (one
    // tracer, block batching: sw_kernels.hip k_march_tracer_b) -- both read the state just exchanged,
    // the march writes the other buffers, the tracer step only the tracers'.  One block per rank too
    // (the C5 layout over 8 GPUs: two launches per step become one)
    const bool co = c->tr_pending && c->co_launch && c->sw.tracer_num == 1 && c->batch;
    auto co_done = [c] {
        c->tr_pending = false;
        swap_tracer_roles(c);
        swap_tracer_alt(c);
    };
    int probe = 0;
    const int lv = ov_begin(c, 2, !k.x2_save, probe);
    RC(ov_mark(c, 2, probe, false));
    if (lv >= 2 && !c->capturing) {
        RC(overlapped_exchange(c, OCN_TIMER_ONEPASS, 2, with_tracers(c, kStateX2), k.x2_save,   // the state two points deep
            [&](const LBlock &b) -> int {
                const Range in = x2_inner(b);
                return march(b, s, &in, nullptr);
            },
            [&](const LBlock &b) -> int {   // the bands (+ the tracer step)
                const Range in = x2_inner(b);
                RC(march(b, c->comm_stream, nullptr, &in));
                return co ? tracer_step_block(c, b, 1, tau, c->comm_stream) : OCN_OK;
            }, co));
        if (co) co_done();
    } else {
        if (k.x2_save) RC(ring2_run(c, true, s));
        RC(run_sync(c, with_tracers(c, kStateX2), s, nullptr, 2));   // the state two points deep
        if (c->tr_pending && !co && !c->capturing && c->comm_stream) {
            // the previous state's tracer step beside this step's march (on the comm stream: both read
            // the state just exchanged, the march writes the other buffers, the tracer step only the
            // tracers'); joined by the next step (run_step) or the call's end (finish_call)
            HIPCHK(hipEventRecord(c->ev_fork, s));
            HIPCHK(hipStreamWaitEvent(c->comm_stream, c->ev_fork, 0));
            RC(run_tracer_step(c, tau, c->comm_stream));
            HIPCHK(hipEventRecord(c->ev_join, c->comm_stream));
            c->sync_pending = true;
            c->tr_forked = true;
        }
        RC(timer_begin(c, OCN_TIMER_ONEPASS, rec));
        if (co) {   // (a variant that cannot co-launch flushes the two batches in order: the same results)
            RC(each_block(c, s, [&](const LBlock &b) -> int {
                RC(march(b, s, nullptr, nullptr));
                return tracer_step_block(c, b, 1, tau, s);
            }, true));
            co_done();
        } else {
            RC(each_block(c, s, [&](const LBlock &b) { return march(b, s, nullptr, nullptr); }));
        }
        RC(timer_end(c, rec));
    }
    RC(ov_mark(c, 2, probe, true));
    // the previous state's tracer step: it reads that state (untouched by the march) and the tracers
    // with their first halo ring, both just exchanged
    RC(run_tracer_step(c, tau));
    swap_alt3(c);
    swap_roles(c);
    return OCN_OK;
}

// Two one-pass steps as one launch per block (sw_kernels.hip MarchStep PAIR): the first step's new
// state stays in LDS, the second's is written where a single step writes -- so the pair is one role
// flip of the pairs and of the second buffers, as a single one-pass step is.  Single block, no
// exchange, a variant chosen on the host (pair_ok); 98 B per cell for two steps in the known-constant
// variant, 162 in the general one.  k.one_last: the second step is the call's last (the pending tail's
// last two steps in one launch, complete_open): its consumer waves also store vort, the stresses and
// the RHS terms (MarchStep PAIR + LAST), then last_finish -- in place of a single one-pass step + the
// last step's own march.
static int one_step_pair(ocn_ctx *c, double tau, const StepKind &k)
{
    ocn_ctx::Rec rec;
    hipStream_t s = c->stream;
    RC(timer_begin(c, k.one_last ? OCN_TIMER_ONEPASS2_LAST : OCN_TIMER_ONEPASS2, rec));
    RC(each_block(c, s, [&](const LBlock &b) {
        const Compact t{b.bits, b.rows, c->march};
        return launch_onepass_pair(&b.g, b.ptr.data(), (int)b.ptr.size(), &t, c->sw, tau, k.check ? c->d_nbad : nullptr,
                                   k.check2 ? c->d_nbad : nullptr, (double *)b.sshp_alt, (double *)b.up_alt,
                                   (double *)b.vp_alt, s, kc_of(c, b), k.one_last);
    }));
    RC(timer_end(c, rec));
    swap_alt3(c);
    swap_roles(c);
    return k.one_last ? last_finish(c) : OCN_OK;
}

// Two x2 steps as one launch per block (sw_kernels.hip MarchStep PAIR + X2): the state exchanged FOUR
// points deep once (the pair's producers form the first step on the interior and the 2 halo rings
// neighbours own -- their D 3 deep, from the state 4 deep -- the consumers the second step on the
// interior), so a block with neighbours runs pairs as a single block does: one exchange and one
// launch per two steps instead of one each per step.  The extra rings live outside the reference's
// arrays (allocate: kXRing more rows, the row padding); the second ring is saved / restored around
// the sequence as for the x2 steps (ring2_run, x2_end).  The known-constant variant (x4_now).
// (shared/mpp/syncborder_block2D_gen_all.fi:100-129 per stage in the reference: 7 per step)
// The part of the interior a pair of x2 steps computes without the exchange: the interior less 4
// points on every side a neighbour (diagonals included) fills halos of (the pair reads the state 4
// points out: the producers' D 3 out, from the state 4 out).
// The E / W bands are a whole pair tile wide (kX4BandCols, where the block is wide enough): a band's
// tiles cost the same whatever its width up to that (a pair workgroup marches 116 columns), so the
// wider band takes that many columns off the inner launch for nothing -- one GPU, 2x1 blocks of
// 4096^2 overlapped: see DESIGN.md 4.4
constexpr int kX4BandCols = 116;   // sw_kernels.hip MarchStep::kPairCols
static Range x4_inner(const LBlock &b) { return inner_range(b, band_cols(b, kX4BandCols, 4), 4); }
// Whether every kept block of the GRID, on whatever rank, keeps an inner part under an x4 pair: x4_inner's
// rule from the global block table, so every rank has the same answer (ov_begin's `allow`: a rank whose
// own blocks all keep one would otherwise measure pairs its peers cannot, and the vote never conclude)
static bool x4_inner_everywhere(const ocn_ctx *c)
{
    auto kept = [&](int bm, int bn) {
        return bm >= 1 && bm <= c->bnx && bn >= 1 && bn <= c->bny &&
               c->gblocks[(size_t)(bm - 1) + (size_t)(bn - 1) * c->bnx].rank >= 0;
    };
    for (const GBlock &g : c->gblocks) {
        if (g.rank < 0) continue;
        auto fed = [&](int dm, int dn) {   // side_fed: the side's neighbour or one of its two diagonal ones
            for (int t = -1; t <= 1; ++t)
                if (kept(g.bm + (dm ? dm : t), g.bn + (dn ? dn : t))) return true;
            return false;
        };
        const int w = g.g.nx_end - g.g.nx_start + 1, h = g.g.ny_end - g.g.ny_start + 1;
        const int ew = w >= 3 * kX4BandCols ? kX4BandCols : 4;   // band_cols
        if (w - (fed(-1, 0) ? ew : 0) - (fed(1, 0) ? ew : 0) < 1 || h - (fed(0, -1) ? 4 : 0) - (fed(0, 1) ? 4 : 0) < 1)
            return false;
    }
    return true;
}

// With OCN_OPT_OVERLAP 2 (the default with remote peers; not while capturing): the inner part
// (x4_inner) on the compute stream beside the exchange on the comm stream (the device's highest
// priority), then the bands around it there -- the RCCL group's latency hides behind the inner
// pair; the two launches write disjoint points of the new state (other buffers than the ones read),
// the exchange writes halos only the bands read.
// Tracer runs (tracer steps, c->tr_call): the exchange carries the tracers 2 deep; the pending tracer
// step of the state before the pair (A) runs over the interior and the first halo ring neighbours own
// (launch_tracer_step ext: as those neighbours update it), co-launched with the pair where it can be;
// the producers also write the first step's new state (LBlock::trs), and the tracer step of that state
// (B) runs after the pair from there -- two tracer steps per exchange, as the reference runs one per
// step after its exchanges; the second tracer ring is saved / restored with the state's (ring2_run).
static int one_step_x4(ocn_ctx *c, double tau, const StepKind &k)
{
    hipStream_t s = c->stream;
    ocn_ctx::Rec rec;
    c->hn_fresh = false;
    const bool tr = c->tr_call, trA = tr && c->tr_pending;
    const bool co = trA && c->co_launch && c->sw.tracer_num == 1 && c->batch;
    auto tr_a = [&](const LBlock &b, int t, hipStream_t st) -> int {
        std::vector<void *> tab = b.ptr;
        tab[field_slot(OCN_HHQ_REST)] = b.hr_x;   // (h_r with the neighbours' second ring)
        const Compact ct{b.bits, b.rows_x, c->march};
        return launch_tracer_step(&b.g, tab.data(), (int)tab.size(), &ct, t, tau, c->sw.time_smooth,
                                  (double *)b.ptr[field_slot(OCN_FF1N(t))], (double *)b.ffp_alt[(size_t)t - 1], b.own,
                                  st, true);
    };
    auto tr_b = [&](const LBlock &b, int t, hipStream_t st) -> int {
        std::vector<void *> tab = b.ptr;   // the state the pair's first step formed
        tab[field_slot(OCN_SSH)] = b.trs[0]; tab[field_slot(OCN_SSHP)] = b.trs[1];
        tab[field_slot(OCN_UBRTR)] = b.trs[2]; tab[field_slot(OCN_VBRTR)] = b.trs[3];
        const Compact ct{b.bits, b.rows_x, c->march};
        return launch_tracer_step(&b.g, tab.data(), (int)tab.size(), &ct, t, tau, c->sw.time_smooth,
                                  (double *)b.ptr[field_slot(OCN_FF1N(t))], (double *)b.ffp_alt[(size_t)t - 1], b.own,
                                  st, false);
    };
    auto tr_done = [c] {
        swap_tracer_roles(c);
        swap_tracer_alt(c);
    };
    auto pair = [&](const LBlock &b, hipStream_t st, const Range *range, const Range *frame_of) -> int {
        ocn_block bx = b.g;   // the block widened by kXRing rings, the bases moved to A(bnd_x1 - kXRing, bnd_y1 - kXRing)
        bx.bnd_x1 -= kXRing; bx.bnd_x2 += kXRing; bx.bnd_y1 -= kXRing; bx.bnd_y2 += kXRing;
        const long sh = (long)kXRing * b.g.pitch + kXRing;
        std::vector<void *> tab(b.ptr.size(), nullptr);
        for (int id = OCN_SSH; id < OCN_SSH + num_r8(c); ++id) tab[field_slot(id)] = b.f<double>(id) - sh;
        tab[field_slot(OCN_HHQ_REST)] = b.hr_x - sh;   // (the h_r-read variant: h_r with the neighbours' 4 rings)
        const Compact t{b.bits_x4, b.rows_x4, c->march};
        double *trs_x[4];
        for (int i = 0; i < 4; ++i) trs_x[i] = b.trs[i] ? b.trs[i] - sh : nullptr;
        return launch_onepass_pair_x4(&bx, tab.data(), (int)tab.size(), &t, c->sw, tau, k.check ? c->d_nbad : nullptr,
                                      k.check2 ? c->d_nbad : nullptr, (double *)b.sshp_alt - sh, (double *)b.up_alt - sh,
                                      (double *)b.vp_alt - sh, st, kc_of(c, b), b.own, range, (int)c->blocks.size(),
                                      frame_of, tr ? trs_x : nullptr);
    };
    bool inner_ok = true;   // (every block keeps an inner part: the bands around it are disjoint)
    for (const LBlock &b : c->blocks) {
        const Range in = x4_inner(b);
        inner_ok = inner_ok && in.m0 <= in.m1 && in.n0 <= in.n1;
    }
    int probe = 0;
    // (measured only where every block of the grid keeps one: the same on every rank)
    const int lv = ov_begin(c, 4, !k.x2_save && x4_inner_everywhere(c), probe);
    RC(ov_mark(c, 4, probe, false));
    if (lv >= 2 && !c->capturing && inner_ok) {
        RC(overlapped_exchange(c, OCN_TIMER_ONEPASS2, 4, tr ? with_tracers(c, kStateX2) : kStateX2, k.x2_save,   // the state 4 deep
            [&](const LBlock &b) -> int {
                const Range in = x4_inner(b);
                return pair(b, s, &in, nullptr);
            },
            [&](const LBlock &b) -> int {   // the bands (+ tracer step A)
                const Range in = x4_inner(b);
                RC(pair(b, c->comm_stream, nullptr, &in));
                return co ? tr_a(b, 1, c->comm_stream) : OCN_OK;
            }, co));
    } else {
        if (k.x2_save) RC(ring2_run(c, true, s));
        RC(run_sync(c, tr ? with_tracers(c, kStateX2) : kStateX2, s, nullptr, 4));   // the state four points deep
        RC(timer_begin(c, OCN_TIMER_ONEPASS2, rec));
        RC(each_block(c, s, [&](const LBlock &b) -> int {
            RC(pair(b, s, nullptr, nullptr));
            return co ? tr_a(b, 1, s) : OCN_OK;
        }, co));
        RC(timer_end(c, rec));
    }
    RC(ov_mark(c, 4, probe, true));
    if (trA) {   // tracer step A (here when not co-launched: after the join, it reads the exchanged halos)
        c->tr_pending = false;
        for (int t = co ? 2 : 1; t <= c->sw.tracer_num; ++t)
            RC(each_block(c, s, [&](const LBlock &b) { return tr_a(b, t, s); }));
        tr_done();
    }
    if (tr) {   // tracer step B: the state of the pair's first step
        for (int t = 1; t <= c->sw.tracer_num; ++t)
            RC(each_block(c, s, [&](const LBlock &b) { return tr_b(b, t, s); }));
        tr_done();
    }
    swap_alt3(c);
    swap_roles(c);
    return OCN_OK;
}

// Several one-pass steps as one launch (sw_kernels.hip k_march_multi: a grid barrier
// between the steps; the block's tiles resident together): single small block, no exchange, a
// variant chosen on the host (multi_ok).  Step parity alternates the buffers as the role flips of
// single launches do, so the host flips the roles k.multi times.
static int one_step_multi(ocn_ctx *c, double tau, const StepKind &k)
{
    ocn_ctx::Rec rec;
    hipStream_t s = c->stream;
    const LBlock &b = c->blocks[0];
    const Compact t{b.bits, b.rows, c->march};
    RC(timer_begin(c, OCN_TIMER_ONEPASS_MULTI, rec));
    RC(launch_onepass_multi(&b.g, b.ptr.data(), (int)b.ptr.size(), &t, c->sw, tau, k.multi, k.check ? c->d_nbad : nullptr,
                            (double *)b.sshp_alt, (double *)b.up_alt, (double *)b.vp_alt, c->d_bar,
                            c->d_nbad + 61, s, kc_of(c, b), c->multi_spin));
    RC(timer_end(c, rec));
    if (k.multi & 1) {
        swap_alt3(c);
        swap_roles(c);
    }
    return OCN_OK;
}

static int one_step_fused(ocn_ctx *c, double tau, const StepKind &k)
{
    if (k.multi) return one_step_multi(c, tau, k);
    if (k.pair && k.x2) return one_step_x4(c, tau, k);
    if (k.pair) return one_step_pair(c, tau, k);
    // every other step kind may write the n-level depths (hh_update, hh_shift, hh_init), except a
    // single-block one-pass step (not followed by the fused hh_init + A) and the last step's march
    if (!((k.one || k.one_last) && !k.x2 && !k.next_a && !has_exchange(c) && !c->ring_sea)) c->hn_fresh = false;
    if (k.x2) return one_step_x2(c, tau, k);
    if (k.one_last && k.x2_end) RC(x2_end(c, c->stream));
    if (k.one_last && c->tr_pending) {   // the previous state's tracer step, then its tracers' halos
        RC(run_tracer_step(c, tau));
        if (has_exchange(c)) RC(run_sync(c, with_tracers(c, {})));
    }
    if (k.one_last) return has_exchange(c) || c->ring_sea ? one_step_hybrid(c, tau, k, true) : one_step_last(c, tau, k);
    const bool check = k.check, first = k.first, last = k.last, flip = k.flip;
    const ocn_sw_params &sw = c->sw;
    ocn_ctx::Rec rec;
    int32_t *nbad = check ? c->d_nbad : nullptr;
    hipStream_t s = c->stream;
    const bool ffs = sw.full_free_surface > 0;
    const bool full_c2 = last || sw.use_tracers > 0;   // tracers read hh_init's hhq_p every step
    // sw_stencils.h "reuse" steps: hun/hvn/hhn are hh_init's hu/hv/hh of the previous step.  Not
    // on the first step of a call (the host may have changed ssh since) nor on the last one.
    const bool reuse = sw.full_free_surface == 1 && !first && !last && reuse_allowed(c);
    const std::vector<int> &sync_a = reuse ? c->sync_a_reuse : c->sync_a;
    if (flip) {
        if (last) return set_error(OCN_ERR_STATE, "role-flip step on a last step");
        if (k.one && (has_exchange(c) || c->ring_sea)) return one_step_hybrid(c, tau, k);
        if (k.one) {   // the whole step in one launch (single block: no exchange, no ring launch)
            RC(timer_begin(c, OCN_TIMER_ONEPASS, rec));
            RC(each_block(c, s, [&](const LBlock &b) { return launch_onepass(FT(b), sw, tau, nbad,
                                  (double *)b.sshp_alt, (double *)b.up_alt, (double *)b.vp_alt, s, nullptr, false,
                                  kc_of(c, b)); }));
            RC(timer_end(c, rec));
            swap_alt3(c);
            swap_roles(c);
            if (k.next_a) {   // the next step is the last, standard one: hh_init + its fused A
                RC(timer_begin(c, OCN_TIMER_FUSED_CA, rec));
                RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_ca(FT(b), OCN_PART_ALL, sw, tau,
                                       k.next_reuse, false, s); }));
                RC(timer_end(c, rec));
            }
            return OCN_OK;
        }
        // With halo exchanges and OCN_OPT_OVERLAP = 2 (not while capturing a graph: the last
        // exchange stays pending into the next step), each exchange runs on the comm stream beside
        // the inner part (launch_march_part) of the next launch:
        //   [A.frame | fork: sync A || A.inner] B.inner | join | B.frame | fork: sync B || swap,
        //   CA.inner | join | ring launch (the roles before the swap) | CA.frame | fork: sync CA
        //   || the next step's B.inner ...
        // The default (overlap_level) with remote peers; off with only local copies, whose cost
        // the frame bands match (one GPU, 2x2 / 4x2 blocks: 1.61 vs 1.47, 1.89 vs 1.69 ms per step).
        const bool ov = overlap_level(c) >= 2 && has_exchange(c) && !c->capturing;
        if (!k.a_done) {
            RC(timer_begin(c, OCN_TIMER_FUSED_A, rec));
            if (ov) {
                RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_a(FT(b), OCN_PART_FRAME, sw, tau, reuse, s); }));
                RC(fork_sync(c, sync_a));
                RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_a(FT(b), OCN_PART_INNER, sw, tau, reuse, s); }));
            } else {
                RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_a(FT(b), OCN_PART_ALL, sw, tau, reuse, s); }));
            }
            RC(timer_end(c, rec));
            if (!ov) RC(run_sync(c, sync_a));
        }
        RC(timer_begin(c, OCN_TIMER_FUSED_B, rec));
        for (int part : ov ? std::initializer_list<int>{OCN_PART_INNER, OCN_PART_FRAME}
                           : std::initializer_list<int>{OCN_PART_ALL}) {
            if (part == OCN_PART_FRAME) RC(join_sync(c));
            RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_b(FT(b), part, sw, tau, false, reuse, s, nbad, true, k.rc, (double *)b.sshp_alt); }));
        }
        RC(timer_end(c, rec));
        // the current roles' ubrtrn / vbrtrn (+ hhu_p / hhv_p / hhh_p)
        if (ov) RC(fork_sync(c, c->sync_b));
        else RC(run_sync(c, c->sync_b));
        if (k.rc) swap_sshp(c);
        std::vector<std::vector<void *>> pre;   // the ring launch's field tables (roles before the swap)
        for (const LBlock &b : c->blocks) pre.push_back(b.ptr);
        swap_roles(c);
        // hh_init + the next step's fused A (full_free_surface = 1), else hh_init alone
        auto hh_init = [&](int part) -> int {
            RC(each_block(c, s, [&](const LBlock &b) -> int {
                if (k.next_a)
                    RC(launch_fused_ca(FT(b), part, sw, tau, k.next_reuse,
                                       k.next_reuse && k.rc_next, s));
                else
                    RC(launch_fused_c2(FT(b), part, sw, full_c2, s));
                return OCN_OK;
            }));
            return OCN_OK;
        };
        const int hh_timer = k.next_a ? OCN_TIMER_FUSED_CA : OCN_STAGE_HH_INIT;
        const bool hh = !k.next_one && (k.next_a || ffs);   // a one-pass step forms hh_init's values itself
        if (ov && hh) {
            RC(timer_begin(c, hh_timer, rec));
            RC(hh_init(OCN_PART_INNER));
            RC(timer_end(c, rec));
        }
        RC(join_sync(c));
        if (c->ring_sea) {   // a8 + a9 on the ring (no interior points); nothing to do on an all-land ring
            RC(timer_begin(c, OCN_TIMER_FUSED_C1, rec));
            for (size_t i = 0; i < c->blocks.size(); ++i) {
                const LBlock &b = c->blocks[i];
                // recompute steps: B filtered sshp into the other buffer, now the current one; a8
                // on the ring reads the previous one (sshp_alt after the swap) and completes it
                RC(launch_fused_c1(&b.g, pre[i].data(), (int)pre[i].size(), compact_of(c, b), OCN_PART_FRAME, sw, nullptr, s,
                                   k.rc ? (const double *)b.sshp_alt : nullptr));
            }
            RC(timer_end(c, rec));
        }
        if (hh) {
            RC(timer_begin(c, hh_timer, rec));
            RC(hh_init(ov ? OCN_PART_FRAME : OCN_PART_ALL));
            RC(timer_end(c, rec));
            // with CA, hh_init's sync and the next step's sync A in one exchange: A's a1 took
            // hhu / hhv on the low halo ring from hh_init's registers, the values it delivers there
            const std::vector<int> &l = !k.next_a ? *stage_sync(OCN_STAGE_HH_INIT)
                                        : k.next_reuse ? c->sync_ca_reuse : c->sync_ca;
            if (ov) RC(fork_sync(c, l));
            else RC(run_sync(c, l));
        }
        return OCN_OK;
    }
    if (!(overlap_level(c) && has_exchange(c))) {
        RC(join_sync(c));
        if (!k.a_done) {   // else fused A and its sync ran with the previous step's hh_init
            RC(timer_begin(c, OCN_TIMER_FUSED_A, rec));
            RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_a(FT(b), OCN_PART_ALL, sw, tau, reuse, s); }));
            RC(timer_end(c, rec));
            RC(run_sync(c, sync_a));
        }
        RC(timer_begin(c, OCN_TIMER_FUSED_B, rec));
        RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_b(FT(b), OCN_PART_ALL, sw, tau, last, reuse, s); }));
        RC(timer_end(c, rec));
        RC(run_sync(c, c->sync_b));
        RC(timer_begin(c, OCN_TIMER_FUSED_C1, rec));
        RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_c1(FT(b), OCN_PART_ALL, sw, nbad, s); }));
        RC(timer_end(c, rec));
        if (ffs) {
            RC(timer_begin(c, OCN_STAGE_HH_INIT, rec));
            RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_c2(FT(b), OCN_PART_ALL, sw, full_c2, s); }));
            RC(timer_end(c, rec));
            RC(run_sync(c, *stage_sync(OCN_STAGE_HH_INIT)));
        }
        return OCN_OK;
    }
    if (!k.a_done) {   // else fused A and its sync ran with the previous step's hh_init
        RC(timer_begin(c, OCN_TIMER_FUSED_A, rec));
        RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_a(FT(b), OCN_PART_FRAME, sw, tau, reuse, s); }));
        RC(fork_sync(c, sync_a));
        RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_a(FT(b), OCN_PART_INNER, sw, tau, reuse, s); }));
        RC(timer_end(c, rec));
    }
    RC(timer_begin(c, OCN_TIMER_FUSED_B, rec));
    RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_b(FT(b), OCN_PART_INNER, sw, tau, last, reuse, s); }));
    RC(join_sync(c));   // sync A, or the previous role-flip step's last exchange
    RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_b(FT(b), OCN_PART_FRAME, sw, tau, last, reuse, s); }));
    RC(fork_sync(c, c->sync_b));
    RC(timer_end(c, rec));
    RC(timer_begin(c, OCN_TIMER_FUSED_C1, rec));
    RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_c1(FT(b), OCN_PART_INNER, sw, nbad, s); }));
    RC(join_sync(c));
    RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_c1(FT(b), OCN_PART_FRAME, sw, nbad, s); }));
    RC(timer_end(c, rec));
    if (ffs) {
        RC(timer_begin(c, OCN_STAGE_HH_INIT, rec));
        RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_c2(FT(b), OCN_PART_FRAME, sw, full_c2, s); }));
        RC(fork_sync(c, *stage_sync(OCN_STAGE_HH_INIT)));
        RC(each_block(c, s, [&](const LBlock &b) { return launch_fused_c2(FT(b), OCN_PART_INNER, sw, full_c2, s); }));
        RC(join_sync(c));
        RC(timer_end(c, rec));
    }
    return OCN_OK;
}
#undef FT

// ------------------------------------------------------------------ tracers
// expl_tracer (control/tracer.f90:33-62): for every tracer, envoke of the three tracer stages
// with the syncs of interface/tracer/tracer_interface.f90 (flux_x, flux_y; ff1n; none).
static const std::vector<int> kSyncFlux = {OCN_FLUX_X, OCN_FLUX_Y};

static int tracer_stage(ocn_ctx *c, int stage, int k, double tau, bool compact)
{
    ocn_ctx::Rec rec;
    RC(timer_begin(c, OCN_TIMER_TRACER + stage, rec));
    RC(each_block(c, c->stream, [&](const LBlock &b) -> int {
        const Compact t{b.bits, b.rows};
        RC(launch_tracer(&b.g, b.ptr.data(), (int)b.ptr.size(), compact ? &t : nullptr, stage, k, tau, c->sw.time_smooth,
                          c->stream));
        return OCN_OK;
    }));
    RC(timer_end(c, rec));
    if (stage == OCN_TSTAGE_TRAN_DIFF_FLUXES) RC(run_sync(c, kSyncFlux));
    if (stage == OCN_TSTAGE_TRAN_DIFF_TRACER) RC(run_sync(c, {OCN_FF1N(k)}));
    return OCN_OK;
}

static int expl_tracer(ocn_ctx *c, double tau, bool compact)
{
    if (c->sw.use_tracers <= 0) return OCN_OK;
    RC(join_sync(c));   // an exchange a role-flip step left in flight (hh_init's hhu / hhv halos)
    // tran_diff_tracer reads hhq_n, which the step's hh_init set to h_r (depth.f90:14-99, whole
    // array) -- the role-flip steps' CA leaves it as it was, which is h_r unless one of them was
    // uploaded or written through a raw pointer since the last hh_init that stored it
    if (c->hqn_stale || c->r8_handed || c->capturing) {
        for (const LBlock &b : c->blocks)
            HIPCHK(hipMemcpyAsync(b.ptr[field_slot(OCN_HHQ_N)], b.ptr[field_slot(OCN_HHQ_REST)], field_bytes(b),
                                  hipMemcpyDeviceToDevice, c->stream));
        if (!c->capturing) c->hqn_stale = false;
    }
    for (int k = 1; k <= c->sw.tracer_num; ++k)
        for (int stage = 0; stage < OCN_NUM_TSTAGES; ++stage) RC(tracer_stage(c, stage, k, tau, compact));
    return OCN_OK;
}

// Tracer runs with one-pass steps (OCN_OPT_TRACER_STEP): a one-pass step keeps hh_init's depths in
// registers, so expl_tracer after it (control/tracer.f90:33-62, model.f90:156) runs later, as ONE
// launch per tracer (sw_kernels.hip launch_tracer_step, sw_stencils.h TracerStep) that forms the
// depths it reads from the state with hh_init's own functions -- with the next step, after that
// step's exchange (which carries the tracers' ff1 / ff1p one point deep with the state: with_tracers)
// and before anything writes the state it reads.  Its ffn goes to the ff1n buffer and the roles of
// ff1 / ff1n trade (tracer_next_step's ff := ffn); the filtered ff1p to the second buffer.  The call's
// last step (standard hh_init with every level) runs the standard stages after it.
// st: the stream it runs on (one_step_x2 forks it onto the comm stream beside the next step's march:
// the march reads the state the tracer step reads and writes the other buffers; the next step's
// exchange and march wait for it -- run_step joins first)
// tracer k's tracer step on block b
static int tracer_step_block(ocn_ctx *c, const LBlock &b, int k, double tau, hipStream_t st)
{
    return launch_tracer_step(&b.g, b.ptr.data(), (int)b.ptr.size(), compact_of(c, b), k, tau, c->sw.time_smooth,
                              (double *)b.ptr[field_slot(OCN_FF1N(k))], (double *)b.ffp_alt[(size_t)k - 1], b.own, st);
}
static int run_tracer_step(ocn_ctx *c, double tau, hipStream_t st)
{
    if (!c->tr_pending) return OCN_OK;
    c->tr_pending = false;
    ocn_ctx::Rec rec{OCN_TIMER_TRACER_STEP, nullptr, nullptr};
    if (c->stage_timing) {
        RC(get_event(c, rec.a)); RC(get_event(c, rec.b));
        HIPCHK(hipEventRecord(rec.a, st));
    }
    for (int k = 1; k <= c->sw.tracer_num; ++k)
        RC(each_block(c, st, [&](const LBlock &b) { return tracer_step_block(c, b, k, tau, st); }));
    if (rec.b) {
        HIPCHK(hipEventRecord(rec.b, st));
        c->recs.push_back(rec);
    }
    swap_tracer_roles(c);
    swap_tracer_alt(c);
    return OCN_OK;
}
static int run_tracer_step(ocn_ctx *c, double tau) { return run_tracer_step(c, tau, c->stream); }

static std::vector<int> with_tracers(const ocn_ctx *c, const std::vector<int> &fields)
{
    if (!c->tr_call) return fields;
    std::vector<int> out = fields;
    for (int k = 1; k <= c->sw.tracer_num; ++k) { out.push_back(OCN_FF1(k)); out.push_back(OCN_FF1P(k)); }
    return out;
}

// "The fields changed behind the step's back": what the step decisions rest on is dropped, by cause --
// a raw device pointer handed out (ocn_ctx_field), an upload or a sync of field id, a stage launched by
// the host, the initial state formed again.  (real(4) fields also void the compact tables: at the sites.)
enum class Changed { Pointer, Upload, Sync, Stage, Init };
static void fields_changed(ocn_ctx *c, Changed why, int id = -1)
{
    const bool ptr = why == Changed::Pointer, one = ptr || why == Changed::Upload || why == Changed::Sync;
    // a field the role-flip vote's checks cover (check_coherence: the pairs, and for the x2 steps sshp /
    // ubrtrp / vbrtrp, h_r and mu)
    const bool voted = is_flip_field(id) || is_alt_field(id) || id == OCN_HHQ_REST || id == OCN_MU;
    const bool r4_ptr = ptr && is_r4(id);   // (may be written behind our back: r4_escaped; of these flags only hn_fresh)
    if (!one || why == Changed::Sync || voted) c->coherent_known = false;
    // the current buffer changes; the one-pass steps' second buffer must be copied again
    if (!one || is_alt_field(id)) c->alt_ok = false;
    if (!one || is_tracer_field(id)) c->tr_alt_ok = false;
    if (why != Changed::Init && !r4_ptr) c->hh_consistent = false;   // (init: set once init_state has run hh_init)
    c->hn_fresh = false;
    if (!r4_ptr) c->fb_state = kFbUnchecked;
    // h_r's copy (refresh_hrx): any real(8) pointer, h_r itself otherwise (stage: left; init: init_state)
    if (ptr ? !is_r4(id) : one && id == OCN_HHQ_REST) c->hrx_ok = false;
    if (why == Changed::Upload && (id == OCN_HHQ_REST || id == OCN_HHQ_N)) c->hqn_stale = true;
    // a raw r8 pointer names the field's own buffer from now on and may be written at any time
    if (ptr && !is_r4(id)) c->r8_handed = true;
    if (ptr && voted) c->r8_escaped = true;
}

void field_uploaded(ocn_ctx *c, int id)
{
    if (is_r4(id)) { c->static_dirty = true; c->ext_ok = false; }
    fields_changed(c, Changed::Upload, id);
}

// An entry that may take part in a collective: the null check, then f watched under the entry's name
template <class F> static int entry(ocn_ctx *c, const char *name, F &&f)
{
    if (!c) return set_error(OCN_ERR_ARG, "null ctx");
    return guarded(c, name, f);
}

}  // namespace ocn

// ================================================================== C ABI (PSy layer)
extern "C" {

const char *ocn_last_error(void) { return g_last_error.c_str(); }
int ocn_abi_version(void) { return OCN_ABI_VERSION; }
#ifndef OCN_BUILD_ID
#define OCN_BUILD_ID "unknown"
#endif
const char *ocn_build_id(void) { return OCN_BUILD_ID; }
int64_t ocn_launch_count(void) { return (int64_t)g_launches.load(std::memory_order_relaxed); }

// shared: the compute stream of the ensemble `ens` the context becomes a member of (null: its own)
extern "C++" int ocn::ctx_create(const ocn_basin *basin, const ocn_sw_params *sw, const ocn_decomp *dec, const int32_t *mask,
                                 hipStream_t shared, ocn_ens *ens, ocn_ctx **out)
{
    if (!basin || !sw || !dec || !out) return set_error(OCN_ERR_ARG, "null argument");
    if (basin->nx < 5 || basin->ny < 5) return set_error(OCN_ERR_ARG, "nx, ny must be >= 5");
    if (dec->bnx < 1 || dec->bny < 1 || dec->nranks < 1 || dec->rank < 0 || dec->rank >= dec->nranks)
        return set_error(OCN_ERR_ARG, "bad decomposition request");
    if (sw->use_tracers > 0 && (sw->tracer_num < 1 || sw->tracer_num > kMaxTracers))
        return set_error(OCN_ERR_ARG, "tracer_num must be 1.." + std::to_string(kMaxTracers));
    ocn_ctx *c = new ocn_ctx();
    c->basin = *basin; c->sw = *sw; c->dec = *dec;
    c->bnx = dec->bnx; c->bny = dec->bny;
    c->ens = ens;
    set_mask(c, mask);
    int rc = check_hip(hipSetDevice(dec->device), "hipSetDevice");
    if (shared) c->stream = shared;
    else if (!rc) rc = check_hip(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate");
    // the comm stream at the highest priority: the side chains' short frame launches and the
    // exchanges take wave slots as they free up instead of queueing behind the inner marches
    if (!rc) {
        int lo = 0, hi = 0;
        rc = check_hip(hipDeviceGetStreamPriorityRange(&lo, &hi), "hipDeviceGetStreamPriorityRange");
        if (!rc)
            rc = check_hip(hipStreamCreateWithPriority(&c->comm_stream, hipStreamNonBlocking, OCN_COMM_PRIO ? hi : lo),
                           "hipStreamCreateWithPriority");
    }
    if (!rc) rc = check_hip(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming), "hipEventCreate");
    if (!rc) rc = check_hip(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming), "hipEventCreate");
    if (!rc) rc = check_hip(hipEventCreateWithFlags(&c->ev_fb, hipEventDisableTiming), "hipEventCreate");
    if (!rc) rc = check_hip(hipHostMalloc((void **)&c->h_fbz, kFbzWords * sizeof(int32_t), hipHostMallocDefault), "hipHostMalloc");
    if (!rc) rc = decompose(c);
    if (!rc) rc = allocate(c);
    if (!rc) rc = prebuild_plans(c);
    if (!rc) rc = check_hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    if (rc) { ctx_destroy(c); return rc; }
    *out = c;
    return OCN_OK;
}

int ocn_ctx_create(const ocn_basin *basin, const ocn_sw_params *sw, const ocn_decomp *dec, const int32_t *mask,
                   ocn_ctx **out)
{
    return ctx_create(basin, sw, dec, mask, nullptr, nullptr, out);
}

int ocn_ctx_destroy(ocn_ctx *c)
{
    if (c && c->ens) return set_error(OCN_ERR_ARG, "a member of an ensemble is destroyed by ocn_ens_destroy");
    return ctx_destroy(c);
}

extern "C++" int ocn::ctx_destroy(ocn_ctx *c)
{
    if (!c) return OCN_OK;
    if (c->wd.joinable()) {   // the watchdog first: nothing is watched from here on
        {
            std::lock_guard<std::mutex> g(c->wd_mu);
            c->wd_stop = true;
            c->wd_cv.notify_all();
        }
        c->wd.join();
    }
    (void)hipSetDevice(c->dec.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto &g : c->graphs) (void)hipGraphExecDestroy(g.exec);
    for (auto &r : c->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
    if (c->comm && !c->comm_abort_done) ncclCommDestroy(c->comm);
    for (auto &x : c->xq) (void)hipEventDestroy(x.second);
    for (hipEvent_t e : c->xpool) (void)hipEventDestroy(e);
    if (c->lb) {
        Loopback *L = c->lb;
        bool last;
        {
            std::lock_guard<std::mutex> g(L->mu);
            L->ctx[c->dec.rank] = nullptr;   // a rank still waiting for this one fails (lb_meet)
            last = --L->refs == 0;
            L->cv.notify_all();
        }
        if (last) delete L;
    }
    if (c->lb_ev_a) (void)hipEventDestroy(c->lb_ev_a);
    if (c->lb_ev_b) (void)hipEventDestroy(c->lb_ev_b);
    for (void *p : c->allocs) (void)hipFree(p);
    if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    for (const ocn_ctx::OvSlot &slot : c->ov_slot)
        for (hipEvent_t e : slot.ev)
            if (e) (void)hipEventDestroy(e);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_fb) (void)hipEventDestroy(c->ev_fb);
    if (c->h_fbz) (void)hipHostFree(c->h_fbz);
    if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
    if (c->stream && !c->ens) (void)hipStreamDestroy(c->stream);   // (a member's: the ensemble's)
    delete c;
    return OCN_OK;
}

int ocn_ctx_block_count(const ocn_ctx *c) { return c ? (int)c->blocks.size() : -1; }

int ocn_ctx_block_info(const ocn_ctx *c, int k, ocn_block_info *out)
{
    if (!c || !out || k < 0 || k >= (int)c->blocks.size()) return set_error(OCN_ERR_ARG, "bad block index");
    const LBlock &b = c->blocks[k];
    out->geom = b.g;
    out->bm = b.bm; out->bn = b.bn;
    for (int d = 0; d < 8; ++d) { out->nbr_rank[d] = b.nbr_rank[d]; out->nbr_k[d] = b.nbr_k[d]; }
    return OCN_OK;
}

static int alt_home(ocn_ctx *c);
void *ocn_ctx_field(const ocn_ctx *c, int k, int id)
{
    if (!c || k < 0 || k >= (int)c->blocks.size() || !has_field(c, id)) {
        set_error(OCN_ERR_ARG, "bad block index or field id");
        return nullptr;
    }
    ocn_ctx *w = const_cast<ocn_ctx *>(c);
    if (complete_open(w) != OCN_OK) return nullptr;   // the arrays hold what the reference leaves
    if (is_r4(id)) { c->r4_escaped = true; c->ext_ok = false; }   // may be written behind our back: no compact tables
    // a raw r8 pointer names the field's own buffer from now on (step_impl returns the current
    // values there at the end of every call)
    if (!is_r4(id) && alt_home(w) != OCN_OK) return nullptr;
    fields_changed(w, Changed::Pointer, id);
    return c->blocks[k].ptr[field_slot(id)];
}

void *ocn_ctx_stream(const ocn_ctx *c) { return c ? (void *)c->stream : nullptr; }

int ocn_comm_unique_id(void *out_id, int32_t nbytes)
{
    if (!out_id || nbytes < (int32_t)sizeof(ncclUniqueId)) return set_error(OCN_ERR_ARG, "buffer < 128 bytes");
    ncclUniqueId id;
    RC(nccl_rc(ncclGetUniqueId(&id), "ncclGetUniqueId"));
    std::memcpy(out_id, &id, sizeof(id));
    return OCN_OK;
}

int ocn_ctx_attach_comm(ocn_ctx *c, const void *unique_id, int32_t nbytes)
{
    if (!c || !unique_id || nbytes < (int32_t)sizeof(ncclUniqueId)) return set_error(OCN_ERR_ARG, "bad unique id");
    if (c->ens) return set_error(OCN_ERR_ARG, "a member of an ensemble takes no communicator");
    HIPCHK(hipSetDevice(c->dec.device));
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    if (c->comm) return set_error(OCN_ERR_STATE, "a communicator is attached already");
    RC(nccl_rc(ncclCommInitRank(&c->comm, c->dec.nranks, id, c->dec.rank), "ncclCommInitRank"));
    c->comm_aborted = false;
    return OCN_OK;
}

int ocn_ctx_attach_loopback(ocn_ctx *const *ctxs, int32_t n)
{
    if (!ctxs || n < 1 || n > 64) return set_error(OCN_ERR_ARG, "loopback: 1..64 contexts");
    for (int i = 0; i < n; ++i) {
        const ocn_ctx *c = ctxs[i];
        if (c && c->ens) return set_error(OCN_ERR_ARG, "loopback: a member of an ensemble takes no transport");
        if (!c || c->dec.nranks != n || c->dec.rank != i || c->dec.device != ctxs[0]->dec.device)
            return set_error(OCN_ERR_ARG, "loopback: context i must be rank i of nranks = n, all on one device");
        if (c->comm || c->lb || c->initialized)
            return set_error(OCN_ERR_STATE, "loopback: attach before ocn_ctx_init_state, once, without RCCL");
    }
    Loopback *L = new Loopback();
    L->n = n;
    L->ctx.assign(ctxs, ctxs + n);
    for (auto &v : L->cnt) v.assign((size_t)n, 0);
    L->plan.assign((size_t)n, nullptr);
    L->vote.assign((size_t)n, nullptr);
    L->refs = n;
    int rc = OCN_OK;
    for (int i = 0; i < n && !rc; ++i) {
        ocn_ctx *c = ctxs[i];
        rc = check_hip(hipSetDevice(c->dec.device), "hipSetDevice");
        if (!rc) rc = check_hip(hipEventCreateWithFlags(&c->lb_ev_a, hipEventDisableTiming), "hipEventCreate");
        if (!rc) rc = check_hip(hipEventCreateWithFlags(&c->lb_ev_b, hipEventDisableTiming), "hipEventCreate");
    }
    if (rc) { delete L; return rc; }
    for (int i = 0; i < n; ++i) ctxs[i]->lb = L;
    return OCN_OK;
}

int ocn_ctx_overlap_info(ocn_ctx *c, ocn_overlap_info *out)
{
    if (!c || !out) return set_error(OCN_ERR_ARG, "null argument");
    *out = ocn_overlap_info{};
    out->level = overlap_level(c);
    out->state = c->ov_final ? c->ov_final : c->ov_kind ? c->ov_slot[c->ov_kind == 4].state : 0;
    out->kind = c->ov_kind;
    out->probes = c->ov_probes;
    out->seq_ms = c->ov_ms[0];
    out->overlapped_ms = c->ov_ms[1];
    return OCN_OK;
}

int ocn_ctx_clock_info(ocn_ctx *c, int32_t reset, ocn_clock_info *out)
{
    if (!c || !out) return set_error(OCN_ERR_ARG, "null argument");
    *out = ocn_clock_info{};
    HIPCHK(hipSetDevice(c->dec.device));
    HIPCHK(hipStreamSynchronize(c->stream));
    unsigned long long v[3] = {0, 0, 0};
    RC(clock_read(reset != 0, v));
    out->launches = (int64_t)v[2];
    out->clock_ghz = v[1] ? (double)v[0] / ((double)v[1] * 10.0) : 0.0;
    out->sampled_ms = (double)v[1] * 1e-5;
    return OCN_OK;
}

int ocn_ctx_comm_info(ocn_ctx *c, ocn_comm_info *out)
{
    if (!c || !out) return set_error(OCN_ERR_ARG, "null argument");
    *out = ocn_comm_info{};
    out->comm_size = 1;
    if (c->lb) {
        out->transport = 2;
        out->comm_size = c->lb->n;
        out->comm_rank = c->dec.rank;
    } else if (c->comm || c->comm_aborted) {
        out->transport = 1;
        int v = 0, n = 0, r = 0;
        if (ncclGetVersion(&v) == ncclSuccess) out->nccl_version = v;
        std::lock_guard<std::mutex> g(c->comm_mu);
        if (c->comm && !c->comm_abort_done && ncclCommCount(c->comm, &n) == ncclSuccess &&
            ncclCommUserRank(c->comm, &r) == ncclSuccess) {
            out->comm_size = n;
            out->comm_rank = r;
        } else {
            out->comm_size = c->dec.nranks;
            out->comm_rank = c->dec.rank;
        }
    }
    out->exchanges = c->xchg;
    out->exchanges_done = c->wd_s > 0 ? poll_xdone(c) : -1;
    out->watchdog_s = c->wd_s;
    return OCN_OK;
}

int ocn_ctx_set_watchdog(ocn_ctx *c, double seconds)
{
    if (!c || !(seconds >= 0)) return set_error(OCN_ERR_ARG, "watchdog: null ctx or seconds < 0");
    {
        std::lock_guard<std::mutex> g(c->wd_mu);
        c->wd_s = seconds;
        c->call_t0 = std::chrono::steady_clock::now();   // (a call under way is timed from now)
    }
    if (seconds > 0 && !c->wd.joinable()) c->wd = std::thread(wd_loop, c);
    return OCN_OK;
}

int ocn_ctx_set_topography(ocn_ctx *c, const float *h, int64_t count)
{
    if (!c) return set_error(OCN_ERR_ARG, "null ctx");
    if (!h) { c->topo.clear(); return OCN_OK; }
    const int64_t n = (int64_t)(c->basin.nx - 4) * (c->basin.ny - 4);
    if (count != n) return set_error(OCN_ERR_ARG, "topography: (nx-4)*(ny-4) values expected");
    c->topo.assign(h, h + n);
    return OCN_OK;
}

int ocn_ctx_init_state(ocn_ctx *c)
{
    return entry(c, __func__, [&]() -> int {
        HIPCHK(hipSetDevice(c->dec.device));
        c->open = false;   // a pending call tail is void: every field is formed again
        c->open_pair = false;
        c->deferred = 0;
        c->ring2_saved = false;   // (a saved second ring of an x2 sequence is void: init forms it again)
        c->tr_pending = false;
        fields_changed(c, Changed::Init);
        // a multi-step launch's barrier timeout not yet reported is void too: the state is formed again
        if (c->d_nbad) HIPCHK(hipMemsetAsync(c->d_nbad + 61, 0, sizeof(int32_t), c->stream));
        const int rc = fail_fatal(c, init_state(c));
        c->hh_consistent = rc == OCN_OK && !c->r8_handed;   // init_data.f90:60-63 ran hh_init last
        c->hn_fresh = c->hh_consistent && !c->r4_escaped;    // (every level: the n one from h_r)
        return rc;
    });
}

int ocn_ctx_sync(ocn_ctx *c, int field_id)
{
    return entry(c, __func__, [&]() -> int {
        if (!has_r8(c, field_id)) return set_error(OCN_ERR_ARG, "sync: bad ctx or non-real(8) field");
        HIPCHK(hipSetDevice(c->dec.device));
        HaloPlan *p;
        RC(get_plan(c, {field_id}, p));
        // no neighbour block anywhere (one block, no other rank): the exchange writes nothing, so
        // nothing the step decisions rest on changes and a pending call tail may stay pending -- a
        // PSy-style caller syncing between 1-step calls pays no re-check, host wait or tail for it
        if (!p->local.n && p->peers.empty()) return OCN_OK;
        RC(complete_open(c));
        fields_changed(c, Changed::Sync, field_id);
        return run_sync(c, {field_id});
    });
}

int ocn_ctx_stage(ocn_ctx *c, int stage_id, double tau)
{
    return entry(c, __func__, [&]() -> int {
        HIPCHK(hipSetDevice(c->dec.device));
        if (stage_id < 0 || stage_id >= OCN_NUM_STAGES) return set_error(OCN_ERR_ARG, "bad stage id");
        RC(complete_open(c));
        fields_changed(c, Changed::Stage);
        RC(prepare_static(c));
        return envoke(c, stage_id, tau);
    });
}

static void drop_graphs(ocn_ctx *c)
{
    for (auto &g : c->graphs) (void)hipGraphExecDestroy(g.exec);
    c->graphs.clear();
}

// one model step (model.f90:146-160): expl_shallow_water, then expl_tracer
extern "C++" int ocn::run_step(ocn_ctx *c, double tau, const StepKind &k)
{
    if (c->tr_forked) {   // a tracer step forked beside the previous step's march (one_step_x2)
        RC(join_sync(c));
        c->tr_forked = false;
    }
    // tracer steps (OCN_OPT_TRACER_STEP): a one-pass step's tracer step runs with the next step; the
    // pending one of the state a single-block one-pass step reads runs before its march (x2 steps
    // and the last step: after their exchanges, one_step_x2 / one_step_fused)
    if (c->tr_call && k.one && !k.x2) RC(run_tracer_step(c, tau));
    if (!c->fused) c->hn_fresh = false;   // (the reference's stages)
    RC(c->fused ? one_step_fused(c, tau, k) : one_step(c, tau, k.check));
    if (c->tr_call && k.one) {
        c->tr_pending = true;
        return OCN_OK;
    }
    return expl_tracer(c, tau, c->compact);
}

// one step as a replayed hipGraph, captured once per (tau, step kind, compact, role, one-pass
// variant, fixed two-step tile height); a role-flip step swaps the host's pointer roles as the captured launches did.  The
// known-constant variant's constants and the device check's verdict are read from device memory
// by the launches, so a replay sees their current values.
static int graph_step(ocn_ctx *c, double tau, const StepKind &k)
{
    c->hn_fresh = false;   // (a replay runs whatever the captured step ran)
    for (const auto &g : c->graphs)
        if (g.tau == tau && g.kind == k && g.compact == c->compact && g.march == c->march && g.ring_sea == c->ring_sea &&
            g.role == c->role && g.kc_mode == c->kc_mode && g.kc_nv == c->kc_nv && g.pair_rows == pair_rows_fixed()) {
            HIPCHK(hipGraphLaunch(g.exec, c->stream));
            if (k.rc) swap_sshp(c);
            if (k.one || k.one_last) swap_alt3(c);
            if (k.flip || k.one_last) swap_roles(c);
            return OCN_OK;
        }
    if (c->graphs.size() >= 16) drop_graphs(c);
    const int role = c->role;
    hipGraph_t graph;
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    c->capturing = true;
    int rc = run_step(c, tau, k);
    c->capturing = false;
    hipError_t e = hipStreamEndCapture(c->stream, &graph);
    if (rc) return rc;
    HIPCHK(e);
    hipGraphExec_t exec;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    HIPCHK(e);
    c->graphs.push_back(ocn_ctx::Graph{exec, tau, k, c->compact, c->march, c->ring_sea, role, c->kc_mode, c->kc_nv,
                                        pair_rows_fixed()});
    HIPCHK(hipGraphLaunch(exec, c->stream));
    return OCN_OK;
}

int ocn_ctx_tracer_stage(ocn_ctx *c, int stage_id, int tracer, double tau)
{
    return entry(c, __func__, [&]() -> int {
        HIPCHK(hipSetDevice(c->dec.device));
        if (c->sw.use_tracers <= 0 || tracer < 1 || tracer > c->sw.tracer_num)
            return set_error(OCN_ERR_ARG, "no such tracer (use_tracers / tracer_num)");
        if (stage_id < 0 || stage_id >= OCN_NUM_TSTAGES) return set_error(OCN_ERR_ARG, "bad tracer stage id");
        RC(complete_open(c));
        return tracer_stage(c, stage_id, tracer, tau, false);
    });
}

// the current sshp / ubrtrp / vbrtrp (in the second buffers after one-pass steps: role bit 4)
// back into the fields' own buffers, stream-ordered
static int alt_home(ocn_ctx *c)
{
    if (!(c->role & 4)) return OCN_OK;
    RC(copy_to_alt(c, 3, false));
    swap_alt3(c);
    return OCN_OK;
}

// The stream has been synchronised by the caller: read a pending device verdict of the
// known-constant check, so that later calls launch only the variant it selected.
static void learn_fb(ocn_ctx *c)
{
    if (c->fb_state != kFbDevice) return;
    int32_t fv[kFbzWords] = {0, 0};   // the verdict, and the word after it: mu is not +0.0
    if (hipMemcpy(fv, c->d_fbz, sizeof(fv), hipMemcpyDeviceToHost) != hipSuccess) return;
    const int32_t f = fv[0];
    c->fb_state = f == 0 ? kFbZero : f == 1 ? kFbHr : kFbGeneral;
    c->fb_inviscid = fv[1] == 0;
    c->fb_copy = false;
}

// Without a synchronising call: the verdict's copy (prepare_kc) has arrived if its event has
// completed -- a query, never a wait -- so a caller of 1-step calls gets the host-chosen variant
// (and pair launches) a few calls after the check.
static void learn_fb_async(ocn_ctx *c)
{
    if (c->fb_state != kFbDevice || !c->fb_copy || hipEventQuery(c->ev_fb) != hipSuccess) return;
    const int32_t f = *(volatile int32_t *)c->h_fbz;
    c->fb_state = f == 0 ? kFbZero : f == 1 ? kFbHr : kFbGeneral;
    c->fb_inviscid = ((volatile int32_t *)c->h_fbz)[1] == 0;
    c->fb_copy = false;
}

// The one-pass variant of this call (OCN_KC_*): the known-constant one only when its precondition
// is known to hold; a raw r8 pointer in the caller's hands (r8_handed) may change the arrays at any
// time, so then always the general one (a check per call would cost a pass over 12 arrays);
// unchecked: the check runs on the stream and both variants are launched (the device picks) --
// no host wait inside a step.
// x2: for one_step_x2 (the whole interior; the halo points neighbours own are no fallback points;
// h_r with the neighbours' second ring).  A verdict for that range also holds for the hybrid
// steps' inner range (its points and their +-2 neighbourhood lie inside what it covered, with the
// same values there), not the other way round.
static int kc_of_fb(const ocn_ctx *c)
{
    return c->fb_state == kFbZero ? OCN_KC_KNOWN : c->fb_state == kFbHr ? OCN_KC_KNOWN_HR
         : c->fb_state == kFbGeneral ? OCN_KC_GENERAL : OCN_KC_DEVICE;
}
// The two-step launches' inviscid bodies (MarchStep NV) for a call whose variant is kc_mode: a known-
// constant variant chosen on the host from a verdict that found mu = +0.0, with every r_diss row +0.0f
// (never unchecked, after an upload, or with a raw r8 pointer handed out: kc_mode is then another);
// with a communicator only where every rank voted so (check_coherence)
static bool nv_local(const ocn_ctx *c)
{
    return c->inviscid && c->known_const && !c->r8_handed && c->rdiss_zero && c->fb_inviscid &&
           (c->fb_state == kFbZero || c->fb_state == kFbHr);
}
static void set_kc_mode(ocn_ctx *c, int mode)
{
    c->kc_mode = mode;
    c->kc_nv = (mode == OCN_KC_KNOWN || mode == OCN_KC_KNOWN_HR) && nv_local(c) && (!has_comm(c) || c->nv_dev_ok);
}
static int prepare_kc(ocn_ctx *c, bool x2 = false)
{
    if (!c->known_const || c->r8_handed || c->forced) { set_kc_mode(c, OCN_KC_GENERAL); return OCN_OK; }
    learn_fb_async(c);
    if (c->fb_state != kFbUnchecked && x2 && !c->fb_x2) c->fb_state = kFbUnchecked;
    if (c->fb_state == kFbUnchecked) {
        HIPCHK(hipMemsetAsync(c->d_fbz, 0, kFbzWords * sizeof(int32_t), c->stream));   // (the verdict and the mu word)
        for (const LBlock &b : c->blocks) {
            std::vector<void *> tab = b.ptr;
            if (x2) tab[field_slot(OCN_HHQ_REST)] = b.hr_x;
            const Range r = x2 ? Range{b.g.nx_start, b.g.nx_end, b.g.ny_start, b.g.ny_end} : inner_range(b, 1, 1);
            RC(launch_fallback_check(&b.g, tab.data(), b.bits, r, c->d_fbz, b.kc, c->stream, x2 ? b.own : 0u));
        }
        if (!c->capturing) {   // the verdict to pinned host memory, learn_fb_async
            HIPCHK(hipMemcpyAsync(c->h_fbz, c->d_fbz, kFbzWords * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipEventRecord(c->ev_fb, c->stream));
            c->fb_copy = true;
        }
        c->fb_state = kFbDevice;
        c->fb_x2 = x2;
    }
    set_kc_mode(c, kc_of_fb(c));
    return OCN_OK;
}

// The end of a call that leaves no step pending: nothing stays in flight, the pairs' roles return
// (the last step left both buffers of each pair equal), the recompute steps' sshp comes home
extern "C++" int ocn::finish_call(ocn_ctx *c, int rc)
{
    if (const int rj = join_sync(c); rc == OCN_OK) rc = rj;
    // a failed call drops its sequence: a saved second halo ring (x2 steps) must not be restored
    // over what the host uploads or init_state forms next
    if (rc != OCN_OK) c->ring2_saved = false;
    if (c->role & 1) swap_roles(c);
    if (c->role & 2) {   // sshp's buffers are not equal: the current one is copied into the field's own buffer
        RC(copy_to_alt(c, 1, false));
        swap_sshp(c);
    }
    // one-pass steps: sshp / ubrtrp / vbrtrp stay in the second buffers (every access goes through
    // the field table) unless a raw r8 pointer was handed out: then back into the fields' buffers
    if ((c->role & 4) && c->r8_handed) RC(alt_home(c));
    // tracer steps: the last step's standard tracer stages leave ff1 = ff1n everywhere (tracer_next_step's
    // ff := ffn where tran_diff_tracer wrote ffn and its exchange delivered it, both untouched elsewhere):
    // the roles return with no copy; the current ff1p is copied into the field's own buffer
    if (c->role & 8) swap_tracer_roles(c);
    if (c->role & 16) {
        RC(copy_to_alt(c, 0, true));
        swap_tracer_alt(c);
    }
    c->tr_pending = false;
    c->hh_consistent = rc == OCN_OK && !c->r8_handed;   // the last step ran a full hh_init
    return rc;
}

// The planner's snapshot of the context (ocn_step_plan.h StepFacts): taken once per call, where the call's
// launches are planned -- behind prepare_static and a tail (complete_open), which change what it holds
static StepFacts step_facts(const ocn_ctx *c)
{
    StepFacts f{};
    f.onepass = c->onepass; f.lazy = c->lazy; f.multi = c->multi; f.x2 = c->x2; f.flip = c->flip;
    f.recompute = c->recompute; f.known_const = c->known_const; f.last_hybrid = c->last_hybrid;
    f.use_graph = c->use_graph; f.stage_timing = c->stage_timing; f.tr_step = c->tr_step;
    f.compact = c->compact; f.march = c->march; f.fused = c->fused; f.forced = c->forced;
    f.pair = c->pair; f.x4 = c->x4;
    f.full_free_surface = c->sw.full_free_surface; f.trans_terms = c->sw.trans_terms;
    f.ksw_lat = c->sw.ksw_lat; f.use_tracers = c->sw.use_tracers;
    f.nblocks = (int)c->blocks.size();
    f.has_exchange = has_exchange(c); f.has_comm = has_comm(c); f.remote_peers = f.has_comm && c->dec.nranks > 1;
    f.ring_sea = c->ring_sea; f.edge_ring_sea = c->edge_ring_sea; f.rows_x_ok = c->rows_x_ok; f.x4_tab_ok = c->x4_tab_ok;
    f.min_extent = INT32_MAX;
    for (const GBlock &g : c->gblocks)
        if (g.rank >= 0) f.min_extent = std::min({f.min_extent, g.g.nx_end - g.g.nx_start, g.g.ny_end - g.g.ny_start});
    f.x4_pitch_ok = true;
    for (const LBlock &b : c->blocks)
        if (b.g.pitch < (int64_t)(b.g.bnd_x2 - b.g.bnd_x1 + 1 + 2 * kXRing)) f.x4_pitch_ok = false;
    if (f.nblocks == 1) {
        const ocn_block &g = c->blocks[0].g;
        f.cells0 = (long)(g.nx_end - g.nx_start + 1) * (g.ny_end - g.ny_start + 1);
        if (c->multi_fits < 0) c->multi_fits = onepass_multi_fits(&g);   // (asked once: 1-step calls are host-bound)
        f.multi_fits = c->multi_fits > 0;
    }
    f.r8_handed = c->r8_handed; f.reuse_allowed = reuse_allowed(c); f.hh_consistent = c->hh_consistent;
    f.udiv_ok = c->udiv_ok; f.ring2_saved = c->ring2_saved;
    return f;
}
// what prepare_kc and the last vote left for the planner
static Kc kc_state(const ocn_ctx *c) { return Kc{c->kc_mode, c->x4_dev_ok, c->fb_x2}; }

// The first call of a sequence long enough for pairs, right after prepare_kc issued the known-constant
// check: wait for its verdict where the call would then run pairs (ocn_step_plan.h await_kc_pays).  Not
// while a graph is captured (no host wait there).
static int await_kc(ocn_ctx *c, const StepFacts &f, bool x2, int nsteps)
{
    if (!c->fb_copy || c->capturing || !await_kc_pays(f, kc_state(c), x2, nsteps)) return OCN_OK;
    HIPCHK(hipEventSynchronize(c->ev_fb));
    learn_fb_async(c);
    set_kc_mode(c, kc_of_fb(c));
    return OCN_OK;
}

// The pending tail of an open sequence: the last step run (a one-pass step) is run again from the
// previous state -- untouched in the other buffer of each pair and the other sshp / ubrtrp / vbrtrp
// buffers -- as the call's last step (one_step_last: the same new state bit for bit, plus vort,
// the stresses, the RHS terms, a8's copies and hh_init with every level).  Its check_ssh_err
// count was taken the first time.  (The kinds: ocn_step_plan.h plan_tail.)
extern "C++" int ocn::complete_open(ocn_ctx *c)
{
    if (!c->open) return OCN_OK;
    c->open = false;
    HIPCHK(hipSetDevice(c->dec.device));
    const StepFacts f = step_facts(c);
    const TailPlan t = plan_tail(c->deferred, c->deferred_check, c->open_pair, c->open_x2, pair_ok(f, c->kc_mode),
                                 f.ring2_saved);
    c->deferred = 0;
    c->open_pair = false;
    if (t.swap_back) {
        swap_roles(c);
        swap_alt3(c);
        c->tr_pending = false;   // (the tracer step of the state before the last step has run)
    }
    for (int i = 0; i + 1 < t.n; ++i) {
        if (const int rc = run_step(c, c->open_tau, t.k[i])) return finish_call(c, rc);
        if (t.swap_back) c->tr_pending = false;   // (tracer runs: the pair ran the tracer step of that state too)
    }
    c->ring2_saved = t.ring2_saved;
    return finish_call(c, run_step(c, c->open_tau, t.k[t.n - 1]));
}

// one kind of a call: replayed as a captured graph or run; the pair launches' flags
static int run_kind(ocn_ctx *c, double tau, const StepKind &k, bool graph)
{
    if (k.pair) {
        c->pair_used = true;
        if (!k.one_last) c->nv_used = c->kc_nv;   // (a pair whose second step is the call's last runs the full body)
    }
    return graph ? graph_step(c, tau, k) : run_step(c, tau, k);
}

// A call while a sequence is open: goes_on = false if the sequence ends here (the caller forms the tail).
// Else the one-pass variant is prepared -- a device verdict the host has read since selects one -- and the
// call is planned (ocn_step_plan.h plan_open), its kinds handed to emit: step_impl runs them, step_probe none.
extern "C++" {
template <class Emit>
static int open_call(ocn_ctx *c, double tau, int32_t nsteps, int32_t check_every, bool &goes_on, OpenPlan &p, Emit &&emit)
{
    const StepFacts f = step_facts(c);
    goes_on = open_goes_on(f, tau == c->open_tau, c->open_x2);
    if (!goes_on) return OCN_OK;
    RC(prepare_kc(c, c->open_x2));
    p = plan_open(f, kc_state(c), c->open_x2, c->deferred, c->deferred_check, nsteps, check_every, emit);
    return OCN_OK;
}
}

// collect (inside ocn_ens_step): a multi-step launch is planned as ever but left to the ensemble, which
// issues it with the other members' (ens_pending, ens_k)
static int step_impl(ocn_ctx *c, double tau, int32_t nsteps, int32_t check_every, bool collect)
{
    HIPCHK(hipSetDevice(c->dec.device));
    if (nsteps < 0) return set_error(OCN_ERR_ARG, "nsteps < 0");
    if (nsteps == 0) return OCN_OK;
    c->pair_used = c->nv_used = false;
    c->co_used = false;
    c->multi_used = false;
    if (c->open) {
        bool goes_on = false;
        OpenPlan p{};
        int rc = OCN_OK;
        RC(open_call(c, tau, nsteps, check_every, goes_on, p, [&](const StepKind &k, bool graph) {
            if (k.multi) c->multi_used = true;
            if (k.multi && collect) { c->ens_k = k; c->ens_pending = true; }
            else rc = run_kind(c, tau, k, graph);
            c->open_pair = k.pair;
            return rc == OCN_OK;
        }));
        if (goes_on) {
            c->x4_used = c->open_x2 && p.mode == kOpenPairs;   // (x2 sequences: pairs of x2 steps, one_step_x4)
            if (rc) { c->open = false; c->deferred = 0; c->open_pair = false; return finish_call(c, rc); }
            c->deferred = p.deferred;   // (pairs: the last 1 or 2 steps wait for the next call or the tail)
            c->deferred_check[0] = p.deferred_check[0];
            c->deferred_check[1] = p.deferred_check[1];
            return OCN_OK;
        }
        RC(complete_open(c));
    }
    RC(prepare_static(c));   // (the stage path reads the compact tables too)
    const StepFacts f = step_facts(c);
    // with RCCL every rank takes part in the decisions (check_coherence reduces the verdicts)
    const bool x2_here = x2_local(f);
    Vote v{c->coherent, f.udiv_ok, f.hh_consistent, x2_here && c->x2_dev_ok};
    if (fresh_votes(f, nsteps, c->coherent_known)) {
        // one_step_x4 possible on this rank: its static conditions and a known-constant verdict for the x2
        // range its host has read (the variant the pairs run; kFbZero stays put through prepare_kc(x2))
        const bool x4_here = x2_here && x4_local(f) && (c->fb_state == kFbZero || c->fb_state == kFbHr) && c->fb_x2;
        VoteOut o;
        RC(check_coherence(c, VoteIn{flip_eligible(f), f.udiv_ok, f.hh_consistent, x2_here, x4_here, nv_local(c)}, o));
        v = Vote{c->coherent, o.udiv_ok, o.hh_consistent, x2_here && o.x2_ok};
    }
    FreshPlan p = plan_fresh(f, v, nsteps);
    c->x2_used = p.x2_call;
    c->flip_used = p.flip_call;
    c->tr_call = c->sw.use_tracers > 0 && p.one_call;
    c->tr_pending = false;
    if (c->tr_call && !c->tr_alt_ok) {   // the second ff1p buffers start as copies
        RC(copy_to_alt(c, 0, true));
        c->tr_alt_ok = true;
    }
    c->hh_consistent = false;   // until this call's last step has run
    c->one_used = p.one_call;
    if (p.x2_call) {
        if (!c->hrx_ok || has_comm(c)) RC(refresh_hrx(c));   // (with RCCL: every rank, every call)
        RC(prebuild_x2(c));
    }
    if (p.one_call) {
        RC(prepare_kc(c, p.x2_call));
        RC(await_kc(c, f, p.x2_call, nsteps));
    }
    if (p.rc_call) c->alt_ok = false;
    if (p.one_call && !c->alt_ok) {   // the second buffers start as copies (they agree outside a8's write set)
        RC(copy_to_alt(c, 3, false));
        c->alt_ok = true;
    }
    c->rc_used = p.rc_call && p.N >= 3;
    if (p.rc_call) RC(copy_to_alt(c, 1, false));   // the second sshp buffer starts as a copy: the two agree outside a8's write set
    RC(join_sync(c));
    p = fresh_pairs(f, p, kc_state(c));
    c->x4_used = p.x4_call;
    int rc = OCN_OK;
    for (int s = 1; s <= nsteps && rc == OCN_OK;) {
        const FreshStep st = fresh_step(p, s, check_every, c->ring2_saved);
        c->ring2_saved = st.ring2_saved;
        s += st.steps;
        rc = run_kind(c, tau, st.k, p.graph);
    }
    if (p.lazy_end && rc == OCN_OK) {   // the pending tail: complete_open
        c->open = true;
        c->open_pair = false;   // (the call's last step ran single)
        c->deferred = 0;
        c->open_tau = tau;
        c->open_x2 = p.x2_call;
        return OCN_OK;
    }
    return finish_call(c, rc);
}

// ocn_ctx_step's call (ocn_ens_step makes it for every member, under its own name, with collect)
extern "C++" int ocn::step_entry(ocn_ctx *c, double tau, int32_t nsteps, int32_t check_every, bool collect)
{
    // (a usage error before any collective: no peer waits on this rank yet, the communicator stays)
    if (!c->initialized) return set_error(OCN_ERR_STATE, "ocn_ctx_init_state not called");
    return fail_fatal(c, step_impl(c, tau, nsteps, check_every, collect));
}

// ocn_ens_step_record's and ocn_ens_step_forced's question before any step runs: multi = this call would be
// planned as ONE multi-step launch, the variant's choice (prepare_kc) included; go = it would go on with the open
// sequence at all, no deferred step ahead of its first one.  None of its steps is run.  (Steps an earlier
// call deferred stay deferred: the call itself runs them first.)
extern "C++" int ocn::step_probe(ocn_ctx *c, double tau, int32_t nsteps, int32_t check_every, bool *multi, bool *go)
{
    *multi = *go = false;
    if (!c->initialized) return set_error(OCN_ERR_STATE, "ocn_ctx_init_state not called");
    return fail_fatal(c, [&]() -> int {
        HIPCHK(hipSetDevice(c->dec.device));
        if (nsteps < 0) return set_error(OCN_ERR_ARG, "nsteps < 0");
        if (nsteps == 0 || !c->open) return OCN_OK;
        bool goes_on = false;
        OpenPlan p{};
        RC(open_call(c, tau, nsteps, check_every, goes_on, p, [](const StepKind &, bool) { return true; }));
        *multi = goes_on && p.mode == kOpenMulti;
        *go = goes_on && p.go;
        return OCN_OK;
    }());
}

int ocn_ctx_step(ocn_ctx *c, double tau, int32_t nsteps, int32_t check_every)
{
    return entry(c, __func__, [&] { return step_entry(c, tau, nsteps, check_every); });
}

int ocn_ctx_complete(ocn_ctx *c)
{
    return entry(c, __func__, [&] { return complete_open(c); });
}

// The steps an open sequence deferred (ocn_ctx_step leaves up to two requested steps not yet
// enqueued while pairs run), run now -- by the calls that look at what the steps did (their
// check_ssh_err counts, their launch times): as a pair or alone, the tail stays pending.
static int run_deferred(ocn_ctx *c)
{
    if (!c->open || !c->deferred) return OCN_OK;
    // (a pair only where pairs ran: pair_ok / x4_now held when they were deferred)
    const StepKind k = c->deferred == 2 ? continuing_pair(c->deferred_check[0], c->deferred_check[1], c->open_x2)
                                        : continuing_step(c->deferred_check[0], c->open_x2);
    c->open_pair = k.pair;
    c->deferred = 0;
    if (const int rc = run_step(c, c->open_tau, k)) { c->open = false; return finish_call(c, rc); }
    return OCN_OK;
}

// check_ssh_err_kernel's verdict (vel_ssh.f90:40-67): abort_model -> mpi_abort on the cart
// communicator (shared/errors.f90:30-37) stops every rank together, so with ranks the counts are
// max-reduced (one int32: ncclAllReduce, or the loopback vote) and every rank returns
// OCN_ERR_BLOWUP from the same synchronize.
static int sync_impl(ocn_ctx *c)
{
    HIPCHK(hipSetDevice(c->dec.device));
    RC(run_deferred(c));
    RC(join_sync(c));
    int32_t *cnt = c->d_nbad;
    if (has_comm(c)) {   // every rank's synchronize takes part (the collective of the check)
        cnt = c->d_nbad + 56;
        HIPCHK(hipMemcpyAsync(cnt, c->d_nbad, sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        RC(allreduce_max(c, cnt, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    learn_fb(c);
    int32_t nbad = 0, berr = 0;
    HIPCHK(hipMemcpy(&nbad, cnt, sizeof(nbad), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&berr, c->d_nbad + 61, sizeof(berr), hipMemcpyDeviceToHost));
    if (berr) {   // reported once: the flag is cleared (ocn_ctx_init_state starts the state over)
        HIPCHK(hipMemset(c->d_nbad + 61, 0, sizeof(berr)));
        return set_error(OCN_ERR_HIP, "multi-step launch: a grid barrier timed out (results invalid)");
    }
    if (nbad) return set_error(OCN_ERR_BLOWUP, "SIGFPRE predict error: |ssh| >= 1e4 on " + std::to_string(nbad) +
                                                   (has_comm(c) ? " sea points of a block (the most of any rank;"
                                                                  " check_ssh_err_kernel)"
                                                                : " sea points (check_ssh_err_kernel)"));
    return OCN_OK;
}

int ocn_ctx_synchronize(ocn_ctx *c)
{
    return entry(c, __func__, [&] { return fail_fatal(c, sync_impl(c)); });
}

int ocn_ctx_stage_times(ocn_ctx *c, double *ms, int64_t *counts) { return ocn_ctx_stage_stats(c, ms, counts, nullptr); }

int ocn_ctx_stage_stats(ocn_ctx *c, double *ms, int64_t *counts, double *ms_max)
{
    if (!c || !ms || !counts) return set_error(OCN_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->dec.device));
    RC(run_deferred(c));   // (their launches belong to this report, not the next one)
    RC(join_sync(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    learn_fb(c);
    for (auto &r : c->recs) {
        float t = 0.f;
        if (r.stage == OCN_TIMER_EXPOSED) {   // events on two streams: the comm chain may end first
            if (hipEventElapsedTime(&t, r.a, r.b) != hipSuccess || !(t > 0.f)) t = 0.f;
        } else {
            HIPCHK(hipEventElapsedTime(&t, r.a, r.b));
        }
        c->stage_ms[r.stage] += t;
        c->stage_n[r.stage] += 1;
        c->stage_max[r.stage] = std::max(c->stage_max[r.stage], (double)t);
        c->event_pool.push_back(r.a); c->event_pool.push_back(r.b);
    }
    c->recs.clear();
    for (int i = 0; i < OCN_NUM_TIMERS; ++i) {
        ms[i] = c->stage_ms[i]; counts[i] = c->stage_n[i];
        if (ms_max) ms_max[i] = c->stage_max[i];
    }
    for (int i = 0; i < OCN_NUM_TIMERS; ++i) { c->stage_ms[i] = 0; c->stage_n[i] = 0; c->stage_max[i] = 0; }
    return OCN_OK;
}

int ocn_ctx_download(ocn_ctx *c, int k, int id, void *host)
{
    return entry(c, __func__, [&]() -> int {
        if (!host || k < 0 || k >= (int)c->blocks.size() || !has_field(c, id))
            return set_error(OCN_ERR_ARG, "download: bad argument");
        HIPCHK(hipSetDevice(c->dec.device));
        RC(complete_open(c));
        const LBlock &b = c->blocks[k];
        const size_t es = is_r4(id) ? 4 : 8;
        const size_t w = (size_t)(b.g.bnd_x2 - b.g.bnd_x1 + 1), rows = (size_t)(b.g.bnd_y2 - b.g.bnd_y1 + 1);
        HIPCHK(hipStreamSynchronize(c->stream));
        learn_fb(c);
        HIPCHK(hipMemcpy2D(host, w * es, b.ptr[field_slot(id)], (size_t)b.g.pitch * es, w * es, rows,
                           hipMemcpyDeviceToHost));
        return OCN_OK;
    });
}

int ocn_ctx_output_r4(ocn_ctx *c, int k, int id, float undef, float *host)
{
    return entry(c, __func__, [&]() -> int {
        if (!host || k < 0 || k >= (int)c->blocks.size() || !has_field(c, id))
            return set_error(OCN_ERR_ARG, "output_r4: bad argument");
        HIPCHK(hipSetDevice(c->dec.device));
        RC(complete_open(c));
        const LBlock &b = c->blocks[k];
        const int w = b.g.nx_end - b.g.nx_start + 1, h = b.g.ny_end - b.g.ny_start + 1;
        if (w <= 0 || h <= 0) return OCN_OK;
        const long off = (long)(b.g.ny_start - b.g.bnd_y1) * b.g.pitch + (b.g.nx_start - b.g.bnd_x1);
        float *d = nullptr;
        HIPCHK(hipMallocAsync((void **)&d, (size_t)w * h * sizeof(float), c->stream));
        const float *lu = b.f<float>(OCN_LU) + off;
        const dim3 grid((unsigned)((w + 255) / 256), (unsigned)h);
        if (is_r4(id))
            hipLaunchKernelGGL(k_output_r4<float>, grid, dim3(256), 0, c->stream, b.f<float>(id) + off, lu,
                               (long)b.g.pitch, w, h, undef, d);
        else
            hipLaunchKernelGGL(k_output_r4<double>, grid, dim3(256), 0, c->stream, b.f<double>(id) + off, lu,
                               (long)b.g.pitch, w, h, undef, d);
        int rc = check_launch();
        if (rc == OCN_OK && hipMemcpyAsync(host, d, (size_t)w * h * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            rc = set_error(OCN_ERR_HIP, "output_r4: copy");
        (void)hipFreeAsync(d, c->stream);
        HIPCHK(hipStreamSynchronize(c->stream));
        learn_fb(c);
        return rc;
    });
}

int ocn_ctx_upload(ocn_ctx *c, int k, int id, const void *host)
{
    return entry(c, __func__, [&]() -> int {
        if (!host || k < 0 || k >= (int)c->blocks.size() || !has_field(c, id))
            return set_error(OCN_ERR_ARG, "upload: bad argument");
        HIPCHK(hipSetDevice(c->dec.device));
        RC(complete_open(c));
        HIPCHK(hipStreamSynchronize(c->stream));
        field_uploaded(c, id);
        return upload_field(c, c->blocks[k], id, host, false);
    });
}

int ocn_ctx_set_option(ocn_ctx *c, int32_t key, int64_t value)
{
    if (!c) return set_error(OCN_ERR_ARG, "null ctx");
    // an option may change what the next launches are: a pending call tail is formed first
    if (key != OCN_OPT_STAGE_TIMING) {
        HIPCHK(hipSetDevice(c->dec.device));
        RC(complete_open(c));
    }
    switch (key) {
    case OCN_OPT_GRAPH: c->use_graph = value != 0; return OCN_OK;
    case OCN_OPT_STAGE_TIMING:
        c->stage_timing = value != 0;
        if (c->stage_timing) HIPCHK(hipSetDevice(c->dec.device));
        while (c->stage_timing && c->event_pool.size() < 256) {
            hipEvent_t e;
            RC(make_timer_event(e));
            c->event_pool.push_back(e);
        }
        return OCN_OK;
    case OCN_OPT_FUSED:
        if (c->fused != (value != 0)) drop_graphs(c);
        c->fused = value != 0;
        return OCN_OK;
    case OCN_OPT_OVERLAP:
        if (c->overlap != value) drop_graphs(c);
        c->overlap = value < 0 ? -1 : value > 2 ? 2 : (int)value;
        if (c->overlap < 0) ov_reset(c);   // (auto again: measured again)
        return OCN_OK;
    case OCN_OPT_XCHG_DELAY: c->xdelay_us = value < 0 ? 0 : value > 1000000 ? 1000000 : (int)value; return OCN_OK;
    case OCN_OPT_MARCH:
        if (c->march != (value != 0)) drop_graphs(c);
        c->march = value != 0;
        return OCN_OK;
    case OCN_OPT_FLIP: c->flip = value != 0; return OCN_OK;
    case OCN_OPT_RECOMPUTE: c->recompute = value != 0; return OCN_OK;
    case OCN_OPT_ONEPASS: c->onepass = value != 0; return OCN_OK;
    case OCN_OPT_ONEPASS_LAST: c->last_hybrid = value != 0; return OCN_OK;
    case OCN_OPT_KNOWN_CONSTANTS:
        c->known_const = value != 0;   // (the check's verdict stays valid: it describes the arrays)
        return OCN_OK;
    case OCN_OPT_LAZY_TAIL: c->lazy = value != 0; return OCN_OK;
    case OCN_OPT_X2: c->x2 = value != 0; c->coherent_known = false; return OCN_OK;
    case OCN_OPT_PAIR: c->pair = value < 0 ? 0 : value > 2 ? 2 : (int)value; return OCN_OK;
    case OCN_OPT_MULTI: c->multi = value != 0; return OCN_OK;
    case OCN_OPT_TRACER_STEP:   // (the x2 vote checks mu's halo only for tracer steps: vote again)
        c->tr_step = value != 0;
        c->coherent_known = false;
        return OCN_OK;
    case OCN_OPT_MULTI_SPIN: c->multi_spin = value < 1 ? 1 : value > kMultiSpin ? kMultiSpin : (int)value; return OCN_OK;
    case OCN_OPT_X4:
        c->x4 = value <= 0 ? 0 : value >= 3 ? 3 : 1;
        c->coherent_known = false;
        c->hrx_ok = false;   // (h_r's copy 2 or 4 rings deep: refresh_hrx)
        return OCN_OK;
    case OCN_OPT_CO_LAUNCH: c->co_launch = value != 0; return OCN_OK;
    case OCN_OPT_INVISCID: c->inviscid = value != 0; return OCN_OK;   // (prepare_kc: from the next call on)
    case OCN_OPT_BATCH:
        if (c->batch != (value != 0)) drop_graphs(c);
        c->batch = value != 0;
        return OCN_OK;
    case OCN_OPT_COMPACT:   // (re)arms the compact tables: rebuilt from the real(4) fields at the next step
        c->compact_req = value != 0;
        c->r4_escaped = false;
        c->static_dirty = true;
        return OCN_OK;
    default: return set_error(OCN_ERR_ARG, "unknown option");
    }
}

int ocn_ctx_get_option(const ocn_ctx *c, int32_t key, int64_t *value)
{
    if (!c || !value) return set_error(OCN_ERR_ARG, "null argument");
    switch (key) {
    case OCN_OPT_GRAPH: *value = c->use_graph; return OCN_OK;
    case OCN_OPT_STAGE_TIMING: *value = c->stage_timing; return OCN_OK;
    case OCN_OPT_FUSED: *value = c->fused; return OCN_OK;
    case OCN_OPT_OVERLAP: *value = overlap_level(c); return OCN_OK;
    case OCN_OPT_COMPACT: *value = c->compact; return OCN_OK;
    case OCN_OPT_MARCH: *value = c->march; return OCN_OK;
    case OCN_OPT_FLIP: *value = c->flip && c->flip_used; return OCN_OK;
    case OCN_OPT_RECOMPUTE: *value = c->recompute && c->rc_used; return OCN_OK;
    case OCN_OPT_ONEPASS: {
        // 2: the known-constant variant ran, 3: the known-constant variant reading h_r (chosen by the
        // host, or by the device check whose verdict the host has read since)
        const bool z = c->kc_mode == OCN_KC_KNOWN || (c->kc_mode == OCN_KC_DEVICE && c->fb_state == kFbZero);
        const bool h = c->kc_mode == OCN_KC_KNOWN_HR || (c->kc_mode == OCN_KC_DEVICE && c->fb_state == kFbHr);
        *value = c->onepass && c->one_used ? (z ? 2 : h ? 3 : 1) : 0;
        return OCN_OK;
    }
    case OCN_OPT_KNOWN_CONSTANTS: *value = c->known_const; return OCN_OK;
    case OCN_OPT_ONEPASS_LAST: *value = c->last_hybrid; return OCN_OK;
    case OCN_OPT_LAZY_TAIL: *value = c->open ? 2 : c->lazy; return OCN_OK;
    case OCN_OPT_X2: *value = c->x2 && c->x2_used; return OCN_OK;
    case OCN_OPT_BATCH: *value = c->batch; return OCN_OK;
    case OCN_OPT_PAIR: *value = c->pair_used ? 2 : c->pair > 0; return OCN_OK;
    case OCN_OPT_MULTI: *value = c->multi_used ? 2 : c->multi; return OCN_OK;
    case OCN_OPT_TRACER_STEP: *value = c->tr_call ? 2 : c->tr_step; return OCN_OK;
    case OCN_OPT_MULTI_SPIN: *value = c->multi_spin; return OCN_OK;
    case OCN_OPT_X4: *value = c->x4_used ? 2 : c->x4; return OCN_OK;   // (0, 1 or 3 as set)
    case OCN_OPT_CO_LAUNCH: *value = c->co_used ? 2 : c->co_launch; return OCN_OK;
    case OCN_OPT_XCHG_DELAY: *value = c->xdelay_us; return OCN_OK;
    case OCN_OPT_INVISCID: *value = c->nv_used ? 2 : c->inviscid; return OCN_OK;
    default: return set_error(OCN_ERR_ARG, "unknown option");
    }
}

}  // extern "C"
