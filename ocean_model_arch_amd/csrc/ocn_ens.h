// ocn_ens.h -- the ensemble and what its host sources share (ocn_ens.hip, ocn_ens_diag.hip, ocn_ens_modify.hip,
// ocn_ens_filter.hip, ocn_ens_record.hip, ocn_ens_forcing.hip, ocn_ens_peak.hip, ocn_ens_run.hip).  Internal: not
// part of the C ABI (include/ocn_sw.h), included by those eight only.  No device code: the kernels behind these entries are in sw_kernels.hip and ens_*.hip.
#pragma once
#include "ocn_ctx.h"
#include "ocn_ens_plan.h"

// ------------------------------------------------------------------ the buffers of the entries
// One device allocation and one pinned host copy of the same size, made or grown when a call needs more, and for
// an entry that does not wait for its own copy an event: the stream has read the pinned side (awaited before it
// is written again, and before it is freed).  A failed reserve() leaves bytes = 0: the next call tries again.
struct EnsBuf {
    void *d = nullptr, *h = nullptr;
    size_t bytes = 0;
    hipEvent_t ev = nullptr;
    bool ev_set = false;

    int await() { return ev_set ? check_hip(hipEventSynchronize(ev), "hipEventSynchronize") : OCN_OK; }
    int sent(hipStream_t s) { HIPCHK(hipEventRecord(ev, s)); ev_set = true; return OCN_OK; }
    // room for `need` bytes, in multiples of `granule`; event: the buffer's users call await() / sent()
    int reserve(size_t need, size_t granule, bool event = false)
    {
        if (event && !ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (bytes >= need) return OCN_OK;
        RC(await());
        if (d) (void)hipFree(d);   // (waits for the launches that use it)
        if (h) (void)hipHostFree(h);
        d = h = nullptr;
        bytes = 0;
        const size_t grown = (need + granule - 1) / granule * granule;
        HIPCHK(hipMalloc(&d, grown));
        HIPCHK(hipHostMalloc(&h, grown, hipHostMallocDefault));
        bytes = grown;
        return OCN_OK;
    }
    void release()   // (the caller has waited for the stream, or hipFree does)
    {
        if (ev) (void)hipEventDestroy(ev);
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        *this = EnsBuf{};
    }
};

// Tables that go up through pinned memory call after call with no wait in between: one device side (stream order
// keeps its users apart) and two pinned copies -- a call fills one, the next call the other; ev[i]: the stream has
// read copy i (awaited before it is written again).  slot: the copy whose turn it is; the owner moves it.
struct EnsStage2 {
    void *d = nullptr, *h[2] = {nullptr, nullptr};
    size_t bytes = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ev_set[2] = {false, false};
    int slot = 0;

    int await(int i) { return ev_set[i] ? check_hip(hipEventSynchronize(ev[i]), "hipEventSynchronize") : OCN_OK; }
    int sent(int i, hipStream_t s) { HIPCHK(hipEventRecord(ev[i], s)); ev_set[i] = true; return OCN_OK; }
    // room for `need` bytes, in multiples of `granule`.  Growing waits for the device; the new allocations whole
    // before the old ones go, so a failed growth leaves the stage as it was
    int reserve(size_t need, size_t granule)
    {
        if (need <= bytes) return OCN_OK;
        for (int i = 0; i < 2; ++i) RC(await(i));
        const size_t grown = (need + granule - 1) / granule * granule;
        void *nd = nullptr, *nh[2] = {nullptr, nullptr};
        int rc = check_hip(hipMalloc(&nd, grown), "hipMalloc");
        for (int i = 0; i < 2 && !rc; ++i) rc = check_hip(hipHostMalloc(&nh[i], grown, hipHostMallocDefault), "hipHostMalloc");
        for (int i = 0; i < 2 && !rc; ++i)
            if (!ev[i]) rc = check_hip(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming), "hipEventCreate");
        if (rc) {
            if (nd) (void)hipFree(nd);
            for (void *p : nh)
                if (p) (void)hipHostFree(p);
            return rc;
        }
        if (d) (void)hipFree(d);   // (waits for the launches that use it)
        for (int i = 0; i < 2; ++i) {
            if (h[i]) (void)hipHostFree(h[i]);
            h[i] = nh[i];
            ev_set[i] = false;
        }
        d = nd;
        bytes = grown;
        return OCN_OK;
    }
    void release()   // (the caller has waited for the stream, or hipFree does)
    {
        if (d) (void)hipFree(d);
        for (int i = 0; i < 2; ++i) {
            if (h[i]) (void)hipHostFree(h[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
        *this = EnsStage2{};
    }
};

// ------------------------------------------------------------------ ensembles (ocn_sw.h)
struct ocn_ens {
    std::vector<ocn_ctx *> m;
    int device = 0;
    hipStream_t stream = nullptr;
    unsigned *d_bar = nullptr;     // kMultiBarBytes of barrier words per member
    // the launches' member table (sw_kernels.hip EnsEntry), made by ocn_ens_create: a call's launches fill
    // disjoint parts of one pinned copy, the next call takes the other
    EnsStage2 tab;
    int64_t cap_opt = 0;           // OCN_ENS_OPT_CAPACITY (0: none)
    int64_t max_group = 0;         // OCN_ENS_OPT_MAX_GROUP (0: none)
    ocn_ens_info_t last{};
    // ocn_ens_stats: per local block, one buffer per statistic (mean, variance, spread, minimum, maximum)
    // based like the members' arrays (raw: the allocations, made at first use), and the statistics the
    // last call on that block formed (OCN_ENS_STAT_* bits)
    struct Stats { void *raw[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
                   double *p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; int formed = 0; };
    std::vector<Stats> stats;
    // ocn_ens_extrema: the blocks' interiors, the members' (field, lu) table, the per-tile partials and
    // the results, in one device allocation made at first use; h_ext: the tables and the results in pinned host memory
    void *d_ext = nullptr, *h_ext = nullptr;
    // ocn_ens_transform: the weights transposed (ens_wt_stride x ens_wt_cols of all the members), made at first
    // use.  stage: the staging arrays of the path beyond kEnsStatsReg members, stage_n of
    // them stage_bytes apart, each the size of the largest block's array plus its base shift
    EnsBuf w;
    void *stage = nullptr;
    size_t stage_bytes = 0;
    int stage_n = 0;
    // ocn_ens_sample, ocn_ens_sample_h, ocn_ens_record_sample: a call's tables and behind them its results
    // (synchronous entries: no event)
    EnsBuf samp;
    // ocn_ens_local_update: the y and z rows, the taper and the blocks' observation lists
    EnsBuf lu;
    // ocn_ens_assimilate: the call's tables (taper, lists, values, variances, offsets, indices, blocks, the
    // operator's or the recorder's observations, the members' arrays per block), then the device-formed rows hx, y, z and the innovation, prior and
    // posterior vectors, the count and the gate's accept flags (the results come down into as.h at the offsets
    // they have in as.d; the event: the stream has read as.h's tables).  as_last: the last successful call's
    // results (nobs 0: none yet)
    EnsBuf as;
    struct AsLast { int nobs = 0, n = 0; size_t row = 0, hx_at = 0, vec_at = 0, count_at = 0; bool timed = false;
                    size_t accept_at = 0; bool gated = false; } as_last;
    // ocn_ens_set_gate: the squared threshold of the three entries' quality control (0.0: off, the ungated kernels)
    double gate2 = 0.0;
    // OCN_ENS_OPT_ASSIM_TIMING: events around the observation-space launch and the update's launches
    bool as_timing = false;
    hipEvent_t ev_t[3] = {nullptr, nullptr, nullptr};
    // ocn_ens_spread_save / ocn_ens_inflate: per field named so far, per local block, the saved spread
    // (buf[0]) and the factor applied (buf[1]), based like the members' arrays (raw: the allocations, made at
    // first use); formed[i]: buf[i] holds a successful call's result on every block; in_use: the members of
    // the save, one byte each
    struct Inflate {
        int32_t field = 0;
        std::vector<void *> raw[2];
        std::vector<double *> buf[2];
        bool formed[2] = {false, false};
        std::vector<uint8_t> in_use;
    };
    std::vector<Inflate> inflate;
    // ocn_ens_perturb: per local block the int64 scratch of Z, one array per member of the ensemble stride[k]
    // elements apart, based like the members' arrays (raw: the allocations, made at first use); n[k]: the
    // members in use of the last noise launch on block k (0: none yet)
    struct Perturb { std::vector<void *> raw; std::vector<long long *> z; std::vector<long> stride; std::vector<int> n; } perturb;
    // ocn_ens_record_*: the station recorder.  use: one byte per member; field: the operator's distinct fields
    // in the order of their first term; d_series: max_records x nobs x n doubles; d_op: the rows' starts, the
    // terms as ocn_ens_sample_h resolves them (slot: into a gather's pointer table) and, with one local block,
    // as the recording launch reads them (slot: the field's index in `field`), at start_at / term_at / lterm_at.
    // stage: the tables a call brings -- the recording launches' EnsRecMember, one for every member, then one
    // pointer table per gather, tab_b bytes each -- as the launches' member table goes up.
    // steps, records: counted since ocn_ens_record_begin; in_launch: records a marching launch wrote
    struct Recorder {
        bool active = false;
        int32_t nobs = 0, n = 0, every = 0, max_records = 0, records = 0;
        int64_t steps = 0, in_launch = 0;
        std::vector<uint8_t> use;
        std::vector<int32_t> field;
        void *d_series = nullptr, *d_op = nullptr;
        size_t start_at = 0, term_at = 0, lterm_at = 0, tab_b = 0;
        EnsStage2 stage;
    } rec;
    bool rec_in_launch = true;     // OCN_ENS_OPT_RECORD_IN_LAUNCH
    // ocn_ens_forcing_*: the moving-storm forcing.  storm: one per member (read where forced[i]); attached: the
    // forced members.  tab: the launches' table, EnsFrcMember block by block, member by member; held: what its
    // device side holds -- a call sends the table again only where it differs (the storms, who is forced, an
    // array that moved).  second: per member the second RHSx / RHSy buffers of the forcing launch (sw_kernels.hip
    // k_march_multi_frc), based like the member's own (raw: the allocations), made for a forced member at its
    // first such call.  applies, steps, in_launch: ocn_ens_forcing_info's counts
    struct Forcing {
        std::vector<ocn_ens_storm> storm;
        std::vector<uint8_t> forced;
        ocn_ens_forcing_model model{};
        int attached = 0;
        EnsStage2 tab;
        std::vector<EnsFrcMember> held;
        struct Second { void *raw[2] = {nullptr, nullptr}; double *p[2] = {nullptr, nullptr}; };
        std::vector<Second> second;
        int32_t in_launch = 0;
        int64_t applies = 0, steps = 0;
    } frc;
    bool frc_in_launch = true;     // OCN_ENS_OPT_FORCING_IN_LAUNCH
    // ocn_ens_peak_*: the peak map.  use: one byte per member; arr[k * M + i]: member i's arrays of local block k
    // (x = 0 the maximum, 1 the minimum; null where not asked for or not tracked), P based like the field's array,
    // S int32 with the same element index (raw: the allocations).  stage: the tables the launches read
    // (EnsPeakMember), one part per launch taken from the pinned copy in turn (ens_peak_slot; used: bytes of it
    // taken so far); tab_b: one table of every member of every block.  k: steps counted since
    // ocn_ens_peak_begin; in_launch: those whose update a marching launch did
    struct Peak {
        bool active = false;
        int32_t field = 0, what = 0, tracked = 0;
        int64_t k = 0, in_launch = 0;
        std::vector<uint8_t> use;
        struct Arr { void *raw[4] = {nullptr, nullptr, nullptr, nullptr}; double *p[2] = {nullptr, nullptr};
                     int32_t *s[2] = {nullptr, nullptr}; };
        std::vector<Arr> arr;
        EnsStage2 stage;
        size_t used = 0, tab_b = 0;
    } pk;
    bool pk_in_launch = true;      // OCN_ENS_OPT_PEAK_IN_LAUNCH
    bool run_in_launch = true;     // OCN_ENS_OPT_RUN_IN_LAUNCH (ocn_ens_run with a recorder and a peak and / or forced)
};

namespace ocn {

// ---- ocn_ens.hip: the members in use, the launch groups, the stepping loop, an array based like the members'
std::vector<ocn_ctx *> ens_in_use(const ocn_ens *e, const uint8_t *use);
int64_t ens_capacity(const ocn_ens *e);
int ens_groups(const ocn_ens *e, const std::vector<int32_t> &variant, int64_t capacity, std::vector<ocn_ens_group> &groups);
int32_t ens_variant(const ocn_ctx *c, double tau, bool check, bool multi);
// Every asked member's answer to the probe of a call of nsteps steps (step_probe; who: the entry, for guarded's
// message): variant[i], its variant if it would plan ONE multi-step launch (else -1), and go[i], whether it would
// go on with its open sequence at all.  only (null: everyone): the members that are asked
void ens_probe(ocn_ens *e, const char *who, double tau, int32_t nsteps, int32_t check_every, const uint8_t *only,
               std::vector<int32_t> &variant, std::vector<char> &go);
// one flag per member: it is in one of the groups
std::vector<char> ens_grouped(const ocn_ens *e, const std::vector<ocn_ens_group> &groups);
// What a call brings to ocn_ens_step's launches beyond the steps: the capacity in effect and rec, frc or frc with
// peak (the three entries) or rec with frc and / or peak (ocn_ens_run):
//   rec (ocn_ens_step_record's in-launch path): the members' columns (-1: not in use), the first due step, its slot;
//   frc (ocn_ens_step_forced's in-launch path): the time of the call's first step.  The groups that hold a forced
//       member go as forcing launches; the forcing of t0 is written behind the call's planning, ahead of the
//       launches, and the last step's comes home behind them
//   peak (an in-launch call of ocn_ens_step, ocn_ens_step_forced or ocn_ens_run with a peak active):
//       the groups that hold a tracked member go as launches with the peak update in them, from step count k0; the
//       last step's update is the caller's, behind the launches
// A group that holds a recorded member and a forced or tracked one goes as one launch with everything in it
// (sw_kernels.hip k_march_multi_all).  With rec and another, a recorded member that planned otherwise than its probe
// is an error, as a forced or tracked one always is.
struct EnsRecCall { std::vector<int> col; int due0; double *slot0; };
struct EnsFrcCall { double t0; };
struct EnsPeakCall { int32_t k0; };
struct EnsCall { int64_t capacity; const EnsRecCall *rec; const EnsFrcCall *frc; const EnsPeakCall *peak = nullptr; };
int ens_step_run(ocn_ens *e, double tau, int32_t nsteps, int32_t check_every, const EnsCall *call);
void *ens_based_alloc(const LBlock &b, int32_t field, size_t bytes, void **raw);

// The tail the three synchronous sampling entries share, in e->samp, reserved by the entry for up_b + res_b and
// its pinned side filled up to up_b: the tables up, launch(d) -- d the device side, the results to d + up_b --,
// the results down, one wait (nothing in flight reads the buffer afterwards), and out to `host`
template <class F> static int ens_samp_run(ocn_ens *e, size_t up_b, size_t res_b, double *host, F &&launch)
{
    char *d = (char *)e->samp.d, *h = (char *)e->samp.h;
    HIPCHK(hipMemcpyAsync(d, h, up_b, hipMemcpyHostToDevice, e->stream));
    RC(launch(d));
    HIPCHK(hipMemcpyAsync(h + up_b, d + up_b, res_b, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    memcpy(host, h + up_b, res_b);
    return OCN_OK;
}

// ---- ocn_ens_filter.hip: what the localized update, the serial filter and the recorder's entries check and resolve alike
int ens_lu_check(const ocn_ens *e, const std::string &who, const int32_t *field_ids, int32_t nfields,
                 const std::vector<ocn_ctx *> &in, int32_t nobs, const int32_t *io, const int32_t *jo,
                 const double *taper, int32_t ntaper);
int ens_lu_reach(int32_t ntaper);
size_t ens_lu_lists(const ocn_ctx *c0, int32_t nobs, const int32_t *io, const int32_t *jo, int reach,
                    std::vector<std::vector<EnsLuObs>> &lists);
void ens_lu_put_lists(const std::vector<std::vector<EnsLuObs>> &lists, char *h, size_t at, std::vector<size_t> &list_at);
int ens_lu_launches(const std::vector<ocn_ctx *> &in, const int32_t *field_ids, int32_t nfields,
                    const std::vector<std::vector<EnsLuObs>> &lists, const char *d, const std::vector<size_t> &list_at,
                    const double *d_y, const double *d_z, const double *d_taper, int32_t ntaper, int reach, hipStream_t s);
int ens_block_of(const ocn_ctx *c0, int32_t i, int32_t j);
int ens_as_check(const std::string &who, int32_t nobs, const double *value, const double *variance);
// A sparse linear observation operator (ocn_sw.h ocn_ens_sample_h), validated and resolved for n members in
// use: its distinct fields in the order of their first term, and each term's pointer-table slot
// (field slot * blocks + block) * n, element offset and weight.  Nothing is read beyond a bad row.
struct EnsObsHost { std::vector<int32_t> fields; std::vector<EnsObsTerm> term; };
int ens_obs_resolve(const ocn_ctx *c0, const std::string &who, size_t n, int32_t nobs, const int32_t *start,
                    const int32_t *tfield, const int32_t *ti, const int32_t *tj, const double *tw, EnsObsHost &h);
void ens_obs_table(const std::vector<ocn_ctx *> &in, const std::vector<int32_t> &fields, const double **tab);

// ---- ocn_ens_record.hip: the recorder's buffers and events (ocn_ens_record_end, ocn_ens_record_begin over an
// earlier one, ocn_ens_destroy), and what ocn_ens_record_sample and ocn_ens_assimilate_rec check alike
void ens_rec_free(ocn_ens *e);
// ocn_ens_step_record's two pieces, for ocn_ens_run (ocn_ens_run.hip): the stage of one recording call -- `need`
// bytes in the copy whose turn it is --, and record `index` gathered from the members `in` through the pointer
// table at `at` of that stage.  The caller marks the stage sent (rec.stage.sent) behind the call's last use
int ens_rec_stage(ocn_ens *e, size_t need);
int ens_rec_gather(ocn_ens *e, const std::vector<ocn_ctx *> &in, int32_t index, size_t at);
int ens_rec_members(const ocn_ens *e, const std::string &who, const uint8_t *use, std::vector<ocn_ctx *> &in,
                    std::vector<int> &col);
int ens_rec_obs(const ocn_ens *e, const std::string &who, int32_t nobs, const int32_t *row, const int32_t *rec,
                const double *wt, std::vector<EnsRecObs> &robs);

// ---- ocn_ens_forcing.hip: RHSx / RHSy of every forced member for time t into the fields' own arrays -- the table
// where it has changed, one launch per block, the known-constant verdicts dropped -- and nothing else: no tail is
// formed, no other bookkeeping touched (the caller knows the members' sequences go on, or does the rest itself)
int ens_frc_write(ocn_ens *e, double t);
// ocn_ens_step_forced's two pieces, for a forced call with a peak active (ocn_ens_peak.hip): the forced members'
// second buffers made where they are missing; ocn_ens_forcing_apply behind its checks (go: the forced members whose
// open sequence the next step goes on with)
int ens_frc_second(ocn_ens *e);
int ens_frc_apply(ocn_ens *e, double t, const char *who, const std::vector<char> *go);
// what every forced entry asks first: a storm attached and every member initialised (`who` opens the message)
int ens_frc_ready(const ocn_ens *e, const std::string &who);

// ---- ocn_ens_peak.hip: the peak map's buffers and events (ocn_ens_peak_end, ocn_ens_peak_begin over an earlier
// one, ocn_ens_destroy); `need` bytes of the launches' table stage, pinned side and device side (ens_step_run's
// in-launch tables, k_ens_peak's); the entry of member i's arrays of block k without its sources; and a call of
// ocn_ens_step / ocn_ens_step_forced (frc) while a peak is active, behind the entry's own checks
void ens_peak_free(ocn_ens *e);
int ens_peak_slot(ocn_ens *e, size_t need, void **h, void **d);
EnsPeakMember ens_peak_entry(const ocn_ens *e, size_t k, size_t i);
int ens_peak_step(ocn_ens *e, double tau, int32_t nsteps, int32_t check_every, const EnsFrcCall *frc);
// ens_peak_step's piece for ocn_ens_run: one k_ens_peak launch per local block over the tracked members with step k
int ens_peak_launch(ocn_ens *e, int32_t k);

}  // namespace ocn
