// ocn_ens.hip -- ensembles (ocn_sw.h ocn_ens_*): many members of a small basin as contexts that share
// one compute stream, their multi-step launches issued one per group (sw_kernels.hip k_march_multi_b),
// the statistics over the members (ens_stats.hip), their sampling and recombination
// (ens_transform.hip), their localized observation update (ens_local.hip), the serial filter's
// observation-space loop in front of it (ens_assim.hip), the inflation of their spread
// (ens_inflate.hip), their random perturbation (ens_perturb.hip) and the station recorder in their launches
// (sw_kernels.hip k_march_multi_rec).  The members' calls are planned by ocn_ctx.hip
// step_impl; ocn_ens_plan.h holds the grouping policy.
#include "ocn_ctx.h"
#include "ocn_ens_plan.h"

extern "C" {

// ------------------------------------------------------------------ ensembles (ocn_sw.h)
struct ocn_ens {
    std::vector<ocn_ctx *> m;
    int device = 0;
    hipStream_t stream = nullptr;
    unsigned *d_bar = nullptr;     // kMultiBarBytes of barrier words per member
    void *d_tab = nullptr;         // the launches' member table (sw_kernels.hip EnsEntry), tab_bytes
    size_t tab_bytes = 0;
    // the table's pinned host copies: a call's launches fill disjoint parts of one, the next call takes
    // the other; ev[i]: the stream has read copy i (awaited before it is written again)
    void *h_tab[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ev_set[2] = {false, false};
    int slot = 0;
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
    // ocn_ens_transform: the weights transposed (ens_wt_stride x ens_wt_cols of all the members) on the
    // device and in pinned host memory, made at first use; ev_w: the stream has read h_w (awaited before
    // it is written again).  stage: the staging arrays of the path beyond kEnsStatsReg members, stage_n of
    // them stage_bytes apart, each the size of the largest block's array plus its base shift
    void *d_w = nullptr, *h_w = nullptr;
    hipEvent_t ev_w = nullptr;
    bool ev_w_set = false;
    void *stage = nullptr;
    size_t stage_bytes = 0;
    int stage_n = 0;
    // ocn_ens_sample: the points' table, the members' arrays per block and the results, on the device and
    // in pinned host memory (samp_bytes each, grown when a call needs more)
    void *d_samp = nullptr, *h_samp = nullptr;
    size_t samp_bytes = 0;
    // ocn_ens_local_update: the y and z rows, the taper and the blocks' observation lists, on the device
    // and in pinned host memory (lu_bytes each, grown when a call needs more); ev_lu: the stream has read
    // h_lu (awaited before it is written again)
    void *d_lu = nullptr, *h_lu = nullptr;
    size_t lu_bytes = 0;
    hipEvent_t ev_lu = nullptr;
    bool ev_lu_set = false;
    // ocn_ens_assimilate: the call's tables (taper, lists, values, variances, offsets, indices, blocks, the
    // operator's or the recorder's observations, the members' arrays per block), then the device-formed rows hx, y, z and the innovation, prior and
    // posterior vectors, the count and the gate's accept flags, on the device and in pinned host memory (as_bytes each, grown when a
    // call needs more; the results come down into h_as at the offsets they have in d_as); ev_as: the stream
    // has read h_as's tables.  as_last: the last successful call's results (nobs 0: none yet)
    void *d_as = nullptr, *h_as = nullptr;
    size_t as_bytes = 0;
    hipEvent_t ev_as = nullptr;
    bool ev_as_set = false;
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
    // The tables a call brings -- the recording launches' EnsRecMember, one for every member, then one pointer
    // table per gather, tab_b bytes each -- go up through pinned memory as the launches' member table does: a
    // call fills one of h_stage's two copies, the next call the other; ev[i]: the stream has read copy i
    // (awaited before it is written again); d_stage: their place on the device (stream order keeps its users
    // apart).  steps, records: counted since ocn_ens_record_begin; in_launch: records a marching launch wrote
    struct Recorder {
        bool active = false;
        int32_t nobs = 0, n = 0, every = 0, max_records = 0, records = 0;
        int64_t steps = 0, in_launch = 0;
        std::vector<uint8_t> use;
        std::vector<int32_t> field;
        void *d_series = nullptr, *d_op = nullptr, *d_stage = nullptr, *h_stage[2] = {nullptr, nullptr};
        size_t start_at = 0, term_at = 0, lterm_at = 0, tab_b = 0, stage_bytes = 0;
        hipEvent_t ev[2] = {nullptr, nullptr};
        bool ev_set[2] = {false, false};
        int slot = 0;
    } rec;
    bool rec_in_launch = true;     // OCN_ENS_OPT_RECORD_IN_LAUNCH
};

// the recorder's buffers and events (ocn_ens_record_end, ocn_ens_record_begin over an earlier one, ocn_ens_destroy)
static void ens_rec_free(ocn_ens *e)
{
    ocn_ens::Recorder &r = e->rec;
    if (r.d_series) (void)hipFree(r.d_series);   // (waits for the launches that use them)
    if (r.d_op) (void)hipFree(r.d_op);
    if (r.d_stage) (void)hipFree(r.d_stage);
    for (int i = 0; i < 2; ++i) {
        if (r.h_stage[i]) (void)hipHostFree(r.h_stage[i]);
        if (r.ev[i]) (void)hipEventDestroy(r.ev[i]);
    }
    r = ocn_ens::Recorder{};
}

// ocn_ens_plan's policy: ocn_ens_plan.h (pure host code, also built stand-alone)
static int ens_plan(const ocn_block *g, const int32_t *variant, int members, int64_t capacity,
                    std::vector<ocn_ens_group> &out)
{
    const char *err = nullptr;
    const int rc = ens_plan_groups(g, variant, members, capacity, out, &err);
    return rc ? set_error(rc, std::string("ensemble plan: ") + err) : OCN_OK;
}

int ocn_ens_plan(const ocn_block *geom, const int32_t *variant, int32_t members, int64_t capacity, ocn_ens_group *out,
                 int32_t cap, int32_t *count)
{
    std::vector<ocn_ens_group> gs;
    RC(ens_plan(geom, variant, members, capacity, gs));
    if (count) *count = (int32_t)gs.size();
    for (size_t i = 0; i < gs.size() && (int32_t)i < cap && out; ++i) out[i] = gs[i];
    return OCN_OK;
}

int ocn_ens_destroy(ocn_ens *e)
{
    if (!e) return OCN_OK;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (ocn_ctx *c : e->m) (void)ctx_destroy(c);
    for (int i = 0; i < 2; ++i) {
        if (e->ev[i]) (void)hipEventDestroy(e->ev[i]);
        if (e->h_tab[i]) (void)hipHostFree(e->h_tab[i]);
    }
    if (e->d_tab) (void)hipFree(e->d_tab);
    if (e->d_bar) (void)hipFree(e->d_bar);
    for (ocn_ens::Stats &q : e->stats)
        for (void *r : q.raw)
            if (r) (void)hipFree(r);
    if (e->d_ext) (void)hipFree(e->d_ext);
    if (e->h_ext) (void)hipHostFree(e->h_ext);
    if (e->ev_w) (void)hipEventDestroy(e->ev_w);
    if (e->d_w) (void)hipFree(e->d_w);
    if (e->h_w) (void)hipHostFree(e->h_w);
    if (e->stage) (void)hipFree(e->stage);
    if (e->d_samp) (void)hipFree(e->d_samp);
    if (e->h_samp) (void)hipHostFree(e->h_samp);
    if (e->ev_lu) (void)hipEventDestroy(e->ev_lu);
    if (e->d_lu) (void)hipFree(e->d_lu);
    if (e->h_lu) (void)hipHostFree(e->h_lu);
    if (e->ev_as) (void)hipEventDestroy(e->ev_as);
    for (hipEvent_t t : e->ev_t)
        if (t) (void)hipEventDestroy(t);
    if (e->d_as) (void)hipFree(e->d_as);
    if (e->h_as) (void)hipHostFree(e->h_as);
    for (ocn_ens::Inflate &q : e->inflate)
        for (std::vector<void *> &raw : q.raw)
            for (void *r : raw)
                if (r) (void)hipFree(r);
    for (void *r : e->perturb.raw)
        if (r) (void)hipFree(r);
    ens_rec_free(e);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return OCN_OK;
}

int ocn_ens_create(const ocn_basin *basin, const ocn_sw_params *sw, const ocn_decomp *dec, const int32_t *mask,
                   int32_t members, ocn_ens **out)
{
    if (!basin || !sw || !dec || !out) return set_error(OCN_ERR_ARG, "null argument");
    if (members < 1 || members > OCN_ENS_MAX_MEMBERS)
        return set_error(OCN_ERR_ARG, "ensemble: 1.." + std::to_string(OCN_ENS_MAX_MEMBERS) + " members");
    if (dec->nranks != 1) return set_error(OCN_ERR_ARG, "ensemble: one rank (dec->nranks = 1)");
    ocn_ens *e = new ocn_ens();
    e->device = dec->device;
    int rc = check_hip(hipSetDevice(dec->device), "hipSetDevice");
    if (!rc) rc = check_hip(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking), "hipStreamCreate");
    for (int i = 0; i < members && !rc; ++i) {
        ocn_ctx *c = nullptr;
        rc = ctx_create(basin, sw, dec, mask, e->stream, e, &c);
        if (!rc) e->m.push_back(c);
    }
    e->tab_bytes = (size_t)members * onepass_multi_b_entry_bytes();
    if (!rc) rc = check_hip(hipMalloc((void **)&e->d_bar, (size_t)members * kMultiBarBytes), "hipMalloc");
    if (!rc) rc = check_hip(hipMalloc(&e->d_tab, e->tab_bytes), "hipMalloc");
    for (int i = 0; i < 2 && !rc; ++i) {
        rc = check_hip(hipHostMalloc(&e->h_tab[i], e->tab_bytes, hipHostMallocDefault), "hipHostMalloc");
        if (!rc) rc = check_hip(hipEventCreateWithFlags(&e->ev[i], hipEventDisableTiming), "hipEventCreate");
    }
    if (rc) { ocn_ens_destroy(e); return rc; }
    e->last.members = members;
    *out = e;
    return OCN_OK;
}

int ocn_ens_size(const ocn_ens *e) { return e ? (int)e->m.size() : -1; }

int ocn_ens_member(ocn_ens *e, int32_t i, ocn_ctx **out)
{
    if (!e || !out || i < 0 || i >= (int32_t)e->m.size()) return set_error(OCN_ERR_ARG, "ensemble: bad member index");
    *out = e->m[(size_t)i];
    return OCN_OK;
}

int ocn_ens_init_state(ocn_ens *e)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    for (ocn_ctx *c : e->m) RC(ocn_ctx_init_state(c));
    return OCN_OK;
}

int ocn_ens_complete(ocn_ens *e)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    int first = OCN_OK;
    for (ocn_ctx *c : e->m)
        if (const int rc = ocn_ctx_complete(c); rc && !first) first = rc;
    return first;
}

static int64_t ens_capacity(const ocn_ens *e)
{
    const int64_t dev = onepass_multi_b_capacity();
    return e->cap_opt > 0 ? std::min(dev, e->cap_opt) : dev;
}

// a member's planned multi-step launch did not go out: its call fails as step_impl's would
static int ens_fail(ocn_ctx *c, int rc)
{
    c->open = false; c->deferred = 0; c->open_pair = false;
    return fail_fatal(c, finish_call(c, rc));
}

// the launch groups of a call: ocn_ens_plan's of the members with a variant, within `capacity`
static int ens_groups(const ocn_ens *e, const std::vector<int32_t> &variant, int64_t capacity, std::vector<ocn_ens_group> &groups)
{
    const int M = (int)e->m.size();
    int first = OCN_OK;
    auto note = [&](int rc) { if (rc && !first) first = rc; };
    groups.clear();
    if (capacity >= 1 && e->max_group < 1) {
        note(ens_plan(&e->m[0]->blocks[0].g, variant.data(), M, capacity, groups));
    } else if (capacity >= 1) {   // OCN_ENS_OPT_MAX_GROUP: the plan of every max_group planned members
        std::vector<ocn_ens_group> part;
        std::vector<int32_t> v((size_t)M, -1);
        int n = 0;
        for (int i = 0; i < M; ++i) {
            if (variant[(size_t)i] >= 0) { v[(size_t)i] = variant[(size_t)i]; ++n; }
            if (n && (n == e->max_group || i == M - 1)) {
                note(ens_plan(&e->m[0]->blocks[0].g, v.data(), M, capacity, part));
                groups.insert(groups.end(), part.begin(), part.end());
                std::fill(v.begin(), v.end(), -1);
                n = 0;
            }
        }
    }
    return first;
}

// the variant of a member whose call is planned as a multi-step launch (ens_pending), or -1: the launch takes
// the library's fused path with the sw switches it needs; else the member's own launch
static int32_t ens_variant(const ocn_ctx *c, double tau, bool check)
{
    if (c->ens_pending && c->fused && c->sw.full_free_surface == 1 && c->sw.trans_terms > 0 && c->sw.ksw_lat > 0)
        return onepass_multi_variant(c->kc_mode, tau, check);
    return -1;
}

// A recording call's part in ocn_ens_step's launches (ocn_ens_step_record's in-launch path): the capacity
// in effect, the members' columns (-1: not in use), the first due step and its slot
struct EnsRecCall { int64_t capacity; std::vector<int> col; int due0; double *slot0; };

// ocn_ens_step, and with `rec` the same call with the recorder in its launches
static int ens_step_run(ocn_ens *e, double tau, int32_t nsteps, int32_t check_every, const EnsRecCall *rec)
{
    const int M = (int)e->m.size();
    e->last = ocn_ens_info_t{};
    e->last.members = M;
    int first = OCN_OK;
    auto note = [&](int rc) { if (rc && !first) first = rc; };
    // every member plans its call as ocn_ctx_step does and runs whatever is not a multi-step launch
    std::vector<int32_t> variant((size_t)M, -1);
    for (int i = 0; i < M; ++i) {
        ocn_ctx *c = e->m[(size_t)i];
        c->ens_pending = false;
        c->ens_collect = true;
        note(guarded(c, "ocn_ens_step", [&] { return step_entry(c, tau, nsteps, check_every); }));
        c->ens_collect = false;
        variant[(size_t)i] = ens_variant(c, tau, c->ens_k.check);
    }
    HIPCHK(hipSetDevice(e->device));
    e->last.capacity = rec ? rec->capacity : ens_capacity(e);
    std::vector<ocn_ens_group> groups;
    note(ens_groups(e, variant, e->last.capacity, groups));
    std::vector<char> done((size_t)M, 0);
    size_t rec_off = 0;   // (members of the recording launches so far: their EnsRecMember in the call's stage)
    if (!groups.empty()) {
        const int sl = e->slot;
        e->slot ^= 1;
        if (e->ev_set[sl]) HIPCHK(hipEventSynchronize(e->ev[sl]));
        HIPCHK(hipMemsetAsync(e->d_bar, 0, (size_t)M * kMultiBarBytes, e->stream));
        const size_t eb = onepass_multi_b_entry_bytes();
        size_t off = 0;
        for (const ocn_ens_group &q : groups) {
            std::vector<Compact> cps((size_t)q.members);
            std::vector<EnsMember> ms((size_t)q.members);
            std::vector<ocn_ctx::Rec> recs((size_t)q.members);
            int rc = OCN_OK;
            for (int j = 0; j < q.members; ++j) {
                ocn_ctx *c = e->m[(size_t)q.member[j]];
                const LBlock &b = c->blocks[0];
                cps[(size_t)j] = Compact{b.bits, b.rows, c->march};
                const OnepassKC kc = kc_of(c, b);
                ms[(size_t)j] = EnsMember{&b.g, b.ptr.data(), (int)b.ptr.size(), &cps[(size_t)j],
                                          c->ens_k.check ? c->d_nbad : nullptr,
                                          {(double *)b.sshp_alt, (double *)b.up_alt, (double *)b.vp_alt},
                                          e->d_bar + (size_t)q.member[j] * (kMultiBarBytes / sizeof(unsigned)),
                                          c->d_nbad + 61, kc.kc, c->multi_spin};
                if (!c->fused) c->hn_fresh = false;
                if (!rc) rc = timer_begin(c, OCN_TIMER_ONEPASS_MULTI, recs[(size_t)j]);
            }
            std::vector<int> col((size_t)q.members, -1);
            bool recording = false;
            for (int j = 0; j < q.members && rec && rec->due0 < nsteps; ++j)
                if ((col[(size_t)j] = rec->col[(size_t)q.member[j]]) >= 0) recording = true;
            if (!rc && recording) {   // (the call's stage: ens_rec_stage; its other copy's turn at the next call)
                const ocn_ens::Recorder &r = e->rec;
                const char *d = (const char *)r.d_op;
                const EnsRecLaunch rl{col.data(), r.field.data(), (int)r.field.size(), (const int *)(d + r.start_at),
                                      (const EnsObsTerm *)(d + r.lterm_at), rec->slot0, rec->due0, r.every, r.nobs, r.n,
                                      (EnsRecMember *)r.h_stage[r.slot] + rec_off, (EnsRecMember *)r.d_stage + rec_off};
                rec_off += (size_t)q.members;
                rc = launch_onepass_multi_rec(ms.data(), q.members, q.variant, q.rows, e->m[(size_t)q.member[0]]->sw, tau,
                                              nsteps, e->d_tab, (char *)e->h_tab[sl] + off, eb * (size_t)q.members,
                                              (long)e->last.capacity, rl, e->stream);
            } else if (!rc) {
                rc = launch_onepass_multi_b(ms.data(), q.members, q.variant, q.rows, e->m[(size_t)q.member[0]]->sw, tau,
                                            nsteps, e->d_tab, (char *)e->h_tab[sl] + off, eb * (size_t)q.members,
                                            (long)e->last.capacity, e->stream);
            }
            off += eb * (size_t)q.members;
            for (int j = 0; j < q.members; ++j) {
                ocn_ctx *c = e->m[(size_t)q.member[j]];
                done[(size_t)q.member[j]] = 1;
                c->ens_pending = false;
                if (!rc) {   // the host side of one_step_multi
                    const int rt = timer_end(c, recs[(size_t)j]);
                    if (c->ens_k.multi & 1) {
                        swap_alt3(c);
                        swap_roles(c);
                    }
                    if (rt) note(ens_fail(c, rt));
                } else {
                    note(ens_fail(c, rc));
                }
            }
            if (!rc) {
                ++e->last.groups;
                e->last.batched += q.members;
                if (q.members > e->last.max_group) {
                    e->last.max_group = q.members; e->last.rows = q.rows; e->last.tiles = q.tiles;
                }
            }
        }
        HIPCHK(hipEventRecord(e->ev[sl], e->stream));
        e->ev_set[sl] = true;
    }
    // planned members in no group (no variant the launch takes, or too many tiles for the capacity in
    // effect): their own multi-step launch, as ocn_ctx_step issues it
    for (int i = 0; i < M; ++i) {
        ocn_ctx *c = e->m[(size_t)i];
        if (!c->ens_pending || done[(size_t)i]) continue;
        c->ens_pending = false;
        if (const int rc = run_step(c, tau, c->ens_k)) note(ens_fail(c, rc));
    }
    return first;
}

int ocn_ens_step(ocn_ens *e, double tau, int32_t nsteps, int32_t check_every)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    return ens_step_run(e, tau, nsteps, check_every, nullptr);
}

int ocn_ens_synchronize(ocn_ens *e, int32_t *status)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    int first = OCN_OK;
    std::string msg;
    for (size_t i = 0; i < e->m.size(); ++i) {   // (the first member's wait is the wait: one stream)
        const int rc = ocn_ctx_synchronize(e->m[i]);
        if (status) status[i] = rc;
        if (rc && !first) { first = rc; msg = "member " + std::to_string(i) + ": " + ocn_last_error(); }
    }
    return first ? set_error(first, msg) : OCN_OK;
}

int ocn_ens_info(ocn_ens *e, ocn_ens_info_t *out)
{
    if (!e || !out) return set_error(OCN_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(e->device));
    *out = e->last;
    out->members = (int32_t)e->m.size();
    out->capacity = ens_capacity(e);
    return OCN_OK;
}

int ocn_ens_set_option(ocn_ens *e, int32_t key, int64_t value)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    switch (key) {
    case OCN_ENS_OPT_CAPACITY:
        if (value < 0) return set_error(OCN_ERR_ARG, "OCN_ENS_OPT_CAPACITY: >= 0");
        e->cap_opt = value;
        return OCN_OK;
    case OCN_ENS_OPT_MAX_GROUP:
        if (value < 0) return set_error(OCN_ERR_ARG, "OCN_ENS_OPT_MAX_GROUP: >= 0");
        e->max_group = value;
        return OCN_OK;
    case OCN_ENS_OPT_ASSIM_TIMING:
        if (value != 0 && value != 1) return set_error(OCN_ERR_ARG, "OCN_ENS_OPT_ASSIM_TIMING: 0 or 1");
        e->as_timing = value != 0;
        return OCN_OK;
    case OCN_ENS_OPT_RECORD_IN_LAUNCH:
        if (value != 0 && value != 1) return set_error(OCN_ERR_ARG, "OCN_ENS_OPT_RECORD_IN_LAUNCH: 0 or 1");
        e->rec_in_launch = value != 0;
        return OCN_OK;
    default: return set_error(OCN_ERR_ARG, "unknown ensemble option");
    }
}

// ------------------------------------------------------------------ ensemble statistics (ens_stats.hip)
constexpr int kEnsStatAll = OCN_ENS_STAT_MEAN | OCN_ENS_STAT_VAR | OCN_ENS_STAT_SPREAD | OCN_ENS_STAT_MIN | OCN_ENS_STAT_MAX;
static int ens_stat_index(int32_t stat)
{
    for (int i = 0; i < 5; ++i)
        if (stat == (1 << i)) return i;
    return -1;
}

int ocn_ens_stats(ocn_ens *e, int32_t k, int32_t field_id, const uint8_t *use, int32_t what)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    const ocn_ctx *c0 = e->m[0];
    if (k < 0 || k >= (int32_t)c0->blocks.size()) return set_error(OCN_ERR_ARG, "ens_stats: bad block index");
    if (!has_r8(c0, field_id)) return set_error(OCN_ERR_ARG, "ens_stats: not a real(8) field of the members");
    if (what == 0 || (what & ~kEnsStatAll)) return set_error(OCN_ERR_ARG, "ens_stats: what = OCN_ENS_STAT_* bits");
    std::vector<ocn_ctx *> in;
    for (size_t i = 0; i < e->m.size(); ++i)
        if (!use || use[i]) in.push_back(e->m[i]);
    const bool need_var = (what & (OCN_ENS_STAT_VAR | OCN_ENS_STAT_SPREAD)) != 0;
    if (in.empty()) return set_error(OCN_ERR_ARG, "ens_stats: no member in use");
    if (need_var && in.size() < 2) return set_error(OCN_ERR_ARG, "ens_stats: variance / spread of fewer than two members");
    HIPCHK(hipSetDevice(e->device));
    const LBlock &b0 = c0->blocks[(size_t)k];
    if (e->stats.empty()) e->stats.resize(c0->blocks.size());
    ocn_ens::Stats &st = e->stats[(size_t)k];
    // the buffers first (a failed allocation leaves the earlier results as they were)
    const size_t lead = (size_t)((uintptr_t)b0.ptr[field_slot(field_id)] & 255u);
    for (int i = 0; i < 5; ++i) {
        if (!(what & (1 << i)) || st.raw[i]) continue;
        HIPCHK(hipMalloc(&st.raw[i], field_bytes(b0) + 512));
        st.p[i] = (double *)((char *)st.raw[i] + 256 + lead);
    }
    // the members in use: their pending call tails formed, their arrays as the field tables name them now
    std::vector<const double *> src;
    for (ocn_ctx *c : in) {
        RC(guarded(c, "ocn_ens_stats", [&] { return complete_open(c); }));
        src.push_back((const double *)c->blocks[(size_t)k].ptr[field_slot(field_id)]);
    }
    double *out[5];
    for (int i = 0; i < 5; ++i) out[i] = (what & (1 << i)) ? st.p[i] : nullptr;
    st.formed = 0;
    RC(launch_ens_stats(&b0.g, src.data(), (int)src.size(), need_var, out, e->stream));
    st.formed = what;
    return OCN_OK;
}

// the statistic's buffer of block k, or an error
static int ens_stat_buffer(ocn_ens *e, int32_t k, int32_t stat, const void *host, const double **p)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    const int i = ens_stat_index(stat);
    if (!host || i < 0 || k < 0 || k >= (int32_t)e->m[0]->blocks.size())
        return set_error(OCN_ERR_ARG, "ens_stats: bad block index, statistic or host array");
    if (e->stats.empty() || !(e->stats[(size_t)k].formed & stat))
        return set_error(OCN_ERR_STATE, "ens_stats: the last ocn_ens_stats on this block did not form that statistic");
    *p = e->stats[(size_t)k].p[i];
    return OCN_OK;
}

int ocn_ens_stats_download(ocn_ens *e, int32_t k, int32_t stat, double *host)
{
    const double *p = nullptr;
    RC(ens_stat_buffer(e, k, stat, host, &p));
    HIPCHK(hipSetDevice(e->device));
    const ocn_block &g = e->m[0]->blocks[(size_t)k].g;
    const size_t w = (size_t)(g.bnd_x2 - g.bnd_x1 + 1), rows = (size_t)(g.bnd_y2 - g.bnd_y1 + 1);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy2D(host, w * 8, p, (size_t)g.pitch * 8, w * 8, rows, hipMemcpyDeviceToHost));
    return OCN_OK;
}

int ocn_ens_stats_output_r4(ocn_ens *e, int32_t k, int32_t stat, float undef, float *host)
{
    const double *p = nullptr;
    RC(ens_stat_buffer(e, k, stat, host, &p));
    HIPCHK(hipSetDevice(e->device));
    ocn_ctx *c0 = e->m[0];
    RC(guarded(c0, "ocn_ens_stats_output_r4", [&] { return complete_open(c0); }));   // (as ocn_ctx_output_r4 reads lu)
    const LBlock &b = c0->blocks[(size_t)k];
    const int w = b.g.nx_end - b.g.nx_start + 1, h = b.g.ny_end - b.g.ny_start + 1;
    if (w <= 0 || h <= 0) return OCN_OK;
    const long off = (long)(b.g.ny_start - b.g.bnd_y1) * b.g.pitch + (b.g.nx_start - b.g.bnd_x1);
    float *d = nullptr;
    HIPCHK(hipMallocAsync((void **)&d, (size_t)w * h * sizeof(float), e->stream));
    int rc = launch_output_r4(p + off, b.f<float>(OCN_LU) + off, (long)b.g.pitch, w, h, undef, d, e->stream);
    if (rc == OCN_OK && hipMemcpyAsync(host, d, (size_t)w * h * sizeof(float), hipMemcpyDeviceToHost, e->stream) != hipSuccess)
        rc = set_error(OCN_ERR_HIP, "ens_stats_output_r4: copy");
    (void)hipFreeAsync(d, e->stream);
    HIPCHK(hipStreamSynchronize(e->stream));
    return rc;
}

int ocn_ens_extrema(ocn_ens *e, int32_t field_id, ocn_ens_extrema_t *out)
{
    static_assert(sizeof(EnsPartial) == sizeof(ocn_ens_extrema_t), "EnsPartial is ocn_ens_extrema_t");
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    const ocn_ctx *c0 = e->m[0];
    if (!out || !has_r8(c0, field_id)) return set_error(OCN_ERR_ARG, "ens_extrema: null result or not a real(8) field of the members");
    HIPCHK(hipSetDevice(e->device));
    const size_t M = e->m.size(), nblk = c0->blocks.size();
    std::vector<EnsExtBlock> blk(nblk);
    int tiles = 0;
    for (size_t k = 0; k < nblk; ++k) {
        const ocn_block &g = c0->blocks[k].g;
        EnsExtBlock &q = blk[k];
        q.w = g.nx_end - g.nx_start + 1;
        q.h = g.ny_end - g.ny_start + 1;
        q.off = (long)(g.ny_start - g.bnd_y1) * g.pitch + (g.nx_start - g.bnd_x1);
        q.pitch = (long)g.pitch;
        q.first_tile = tiles;
        tiles += ens_extrema_tiles(q.w, q.h, &q.tiles_x);
    }
    for (size_t i = 0; i < M; ++i) {
        out[i].min = (double)INFINITY;
        out[i].max = -(double)INFINITY;
        out[i].nonfinite = out[i].count = 0;
    }
    if (tiles < 1) return OCN_OK;
    const size_t blk_b = ((sizeof(EnsExtBlock) * nblk + 255) / 256) * 256,
                 tab_b = ((sizeof(EnsExtSrc) * M * nblk + 255) / 256) * 256,
                 part_b = ((sizeof(EnsPartial) * M * (size_t)tiles + 255) / 256) * 256;
    const size_t res_b = sizeof(EnsPartial) * M;
    if (!e->d_ext) HIPCHK(hipMalloc(&e->d_ext, blk_b + tab_b + part_b + res_b));
    if (!e->h_ext) HIPCHK(hipHostMalloc(&e->h_ext, blk_b + tab_b + res_b, hipHostMallocDefault));
    int first = OCN_OK;
    char *d = (char *)e->d_ext, *h = (char *)e->h_ext;
    EnsExtSrc *tab = (EnsExtSrc *)(h + blk_b);
    for (size_t i = 0; i < M; ++i) {
        ocn_ctx *c = e->m[i];
        if (const int rc = guarded(c, "ocn_ens_extrema", [&] { return complete_open(c); }); rc && !first) first = rc;
        for (size_t k = 0; k < nblk; ++k)
            tab[i * nblk + k] = EnsExtSrc{c->blocks[k].f<double>(field_id), c->blocks[k].f<float>(OCN_LU)};
    }
    if (first) return first;
    // the tables up, the launches, the results down, all on the ensemble's stream, and one wait (a
    // synchronous entry: the previous call has ended, nothing reads the pinned tables now)
    memcpy(h, blk.data(), sizeof(EnsExtBlock) * nblk);
    HIPCHK(hipMemcpyAsync(d, h, blk_b + tab_b, hipMemcpyHostToDevice, e->stream));
    EnsPartial *res = (EnsPartial *)(d + blk_b + tab_b + part_b);
    RC(launch_ens_extrema((const EnsExtBlock *)d, (int)nblk, (const EnsExtSrc *)(d + blk_b), (int)M, tiles,
                          (EnsPartial *)(d + blk_b + tab_b), res, e->stream));
    HIPCHK(hipMemcpyAsync(h + blk_b + tab_b, res, res_b, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    memcpy(out, h + blk_b + tab_b, res_b);
    return OCN_OK;
}

// ------------------------------------------------------------------ sampling and recombination (ens_transform.hip)
// the members in use, in member order
static std::vector<ocn_ctx *> ens_in_use(const ocn_ens *e, const uint8_t *use)
{
    std::vector<ocn_ctx *> in;
    for (size_t i = 0; i < e->m.size(); ++i)
        if (!use || use[i]) in.push_back(e->m[i]);
    return in;
}

int ocn_ens_sample(ocn_ens *e, int32_t field_id, const uint8_t *use, int32_t npts, const int32_t *k, const int32_t *i,
                   const int32_t *j, double *host)
{
    if (!e || !k || !i || !j || !host) return set_error(OCN_ERR_ARG, "ens_sample: null argument");
    if (npts < 1 || npts > 65536) return set_error(OCN_ERR_ARG, "ens_sample: 1..65536 points");
    const ocn_ctx *c0 = e->m[0];
    if (!has_r8(c0, field_id)) return set_error(OCN_ERR_ARG, "ens_sample: not a real(8) field of the members");
    const std::vector<ocn_ctx *> in = ens_in_use(e, use);
    if (in.empty()) return set_error(OCN_ERR_ARG, "ens_sample: no member in use");
    const size_t n = in.size(), nblk = c0->blocks.size(), np = (size_t)npts;
    std::vector<long> off(np);
    for (size_t p = 0; p < np; ++p) {
        if (k[p] < 0 || k[p] >= (int32_t)nblk) return set_error(OCN_ERR_ARG, "ens_sample: bad block index");
        const ocn_block &g = c0->blocks[(size_t)k[p]].g;
        if (i[p] < g.bnd_x1 || i[p] > g.bnd_x2 || j[p] < g.bnd_y1 || j[p] > g.bnd_y2)
            return set_error(OCN_ERR_ARG, "ens_sample: a point outside its block's array");
        off[p] = (long)(j[p] - g.bnd_y1) * (long)g.pitch + (i[p] - g.bnd_x1);
    }
    HIPCHK(hipSetDevice(e->device));
    // one layout on both sides: the offsets, the blocks, the members' arrays per block (up), the results (down)
    const size_t off_b = np * sizeof(long), blk_b = (np * sizeof(int) + 7) / 8 * 8, tab_b = nblk * n * sizeof(double *),
                 up_b = off_b + blk_b + tab_b, res_b = np * n * sizeof(double);
    if (e->samp_bytes < up_b + res_b) {   // (a synchronous entry: nothing in flight reads the old ones)
        if (e->d_samp) (void)hipFree(e->d_samp);
        if (e->h_samp) (void)hipHostFree(e->h_samp);
        e->d_samp = e->h_samp = nullptr;
        e->samp_bytes = 0;
        HIPCHK(hipMalloc(&e->d_samp, up_b + res_b));
        HIPCHK(hipHostMalloc(&e->h_samp, up_b + res_b, hipHostMallocDefault));
        e->samp_bytes = up_b + res_b;
    }
    char *d = (char *)e->d_samp, *h = (char *)e->h_samp;
    memcpy(h, off.data(), off_b);
    for (size_t p = 0; p < np; ++p) ((int *)(h + off_b))[p] = k[p];
    // the members in use: their pending call tails formed, their arrays as the field tables name them now
    std::vector<const double *> src;
    for (size_t m = 0; m < n; ++m) {
        ocn_ctx *c = in[m];
        RC(guarded(c, "ocn_ens_sample", [&] { return complete_open(c); }));
        for (size_t b = 0; b < nblk; ++b)
            ((const double **)(h + off_b + blk_b))[b * n + m] = (const double *)c->blocks[b].ptr[field_slot(field_id)];
        src.push_back((const double *)c->blocks[0].ptr[field_slot(field_id)]);
    }
    HIPCHK(hipMemcpyAsync(d, h, up_b, hipMemcpyHostToDevice, e->stream));
    RC(launch_ens_sample(src.data(), nblk > 1 ? (const double *const *)(d + off_b + blk_b) : nullptr, (int)n,
                         (const long *)d, (const int *)(d + off_b), npts, (double *)(d + up_b), e->stream));
    HIPCHK(hipMemcpyAsync(h + up_b, d + up_b, res_b, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    memcpy(host, h + up_b, res_b);
    return OCN_OK;
}

int ocn_ens_transform(ocn_ens *e, const int32_t *field_ids, int32_t nfields, const uint8_t *use, const double *w)
{
    if (!e || !field_ids || !w) return set_error(OCN_ERR_ARG, "ens_transform: null argument");
    if (nfields < 1) return set_error(OCN_ERR_ARG, "ens_transform: no field");
    const ocn_ctx *c0 = e->m[0];
    for (int32_t f = 0; f < nfields; ++f) {
        if (!has_r8(c0, field_ids[f])) return set_error(OCN_ERR_ARG, "ens_transform: not a real(8) field of the members");
        for (int32_t q = 0; q < f; ++q)
            if (field_ids[q] == field_ids[f]) return set_error(OCN_ERR_ARG, "ens_transform: a field named twice");
    }
    const std::vector<ocn_ctx *> in = ens_in_use(e, use);
    if (in.empty()) return set_error(OCN_ERR_ARG, "ens_transform: no member in use");
    const int n = (int)in.size();
    for (size_t q = 0; q < (size_t)n * n; ++q)
        if (!std::isfinite(w[q])) return set_error(OCN_ERR_ARG, "ens_transform: a weight that is not finite");
    HIPCHK(hipSetDevice(e->device));
    // the buffers first (a failed allocation leaves the members as they were)
    const int M = (int)e->m.size();
    const size_t w_bytes = (size_t)ens_wt_stride(M) * ens_wt_cols(M) * sizeof(double);
    if (!e->d_w) HIPCHK(hipMalloc(&e->d_w, w_bytes));
    if (!e->h_w) HIPCHK(hipHostMalloc(&e->h_w, w_bytes, hipHostMallocDefault));
    if (!e->ev_w) HIPCHK(hipEventCreateWithFlags(&e->ev_w, hipEventDisableTiming));
    if (n > kEnsStatsReg && e->stage_n < n) {
        if (e->stage) (void)hipFree(e->stage);   // (waits for the launches that use it)
        e->stage = nullptr;
        e->stage_n = 0;
        size_t big = 0;
        for (const LBlock &b : c0->blocks) big = std::max(big, field_bytes(b));
        e->stage_bytes = (big + 512 + 255) / 256 * 256;
        HIPCHK(hipMalloc(&e->stage, e->stage_bytes * (size_t)n));
        e->stage_n = n;
    }
    for (ocn_ctx *c : in) RC(guarded(c, "ocn_ens_transform", [&] { return complete_open(c); }));
    // the weights transposed and zero-padded, up from pinned memory ahead of the launches
    if (e->ev_w_set) HIPCHK(hipEventSynchronize(e->ev_w));
    const int ws = ens_wt_stride(n), wc = ens_wt_cols(n);
    double *hw = (double *)e->h_w;
    std::fill(hw, hw + (size_t)ws * wc, 0.0);
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) hw[ens_wt_index(n, a, b)] = w[(size_t)a * n + b];
    HIPCHK(hipMemcpyAsync(e->d_w, hw, (size_t)ws * wc * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipEventRecord(e->ev_w, e->stream));
    e->ev_w_set = true;
    int rc = OCN_OK;
    std::vector<double *> mem((size_t)n);
    for (int32_t f = 0; f < nfields && !rc; ++f)
        for (size_t k = 0; k < c0->blocks.size() && !rc; ++k) {
            for (int a = 0; a < n; ++a) mem[(size_t)a] = (double *)in[(size_t)a]->blocks[k].ptr[field_slot(field_ids[f])];
            double *stage = e->stage ? (double *)((char *)e->stage + 256 + ((uintptr_t)mem[0] & 255u)) : nullptr;
            rc = launch_ens_transform(&c0->blocks[k].g, mem.data(), n, (const double *)e->d_w, stage,
                                      (long)(e->stage_bytes / sizeof(double)), e->stream);
        }
    // what ocn_ctx_upload of each of these fields leaves behind (also after a failed launch: the arrays
    // may have changed)
    for (ocn_ctx *c : in)
        for (int32_t f = 0; f < nfields; ++f) field_uploaded(c, field_ids[f]);
    return rc;
}

// ------------------------------------------------------------------ inflation (ens_inflate.hip)
// What ocn_ens_spread_save and ocn_ens_inflate check alike: the list, the fields, the members in use (`in`,
// and one byte per member in `mask`).  `who` opens the message.
static int ens_inf_check(const ocn_ens *e, const std::string &who, const int32_t *field_ids, int32_t nfields,
                         const uint8_t *use, std::vector<ocn_ctx *> &in, std::vector<uint8_t> &mask)
{
    if (!e || !field_ids) return set_error(OCN_ERR_ARG, who + ": null argument");
    if (nfields < 1) return set_error(OCN_ERR_ARG, who + ": no field");
    const ocn_ctx *c0 = e->m[0];
    for (int32_t f = 0; f < nfields; ++f) {
        if (!has_r8(c0, field_ids[f])) return set_error(OCN_ERR_ARG, who + ": not a real(8) field of the members");
        for (int32_t q = 0; q < f; ++q)
            if (field_ids[q] == field_ids[f]) return set_error(OCN_ERR_ARG, who + ": a field named twice");
    }
    in = ens_in_use(e, use);
    if (in.size() < 2) return set_error(OCN_ERR_ARG, who + ": fewer than two members in use");
    mask.assign(e->m.size(), 0);
    for (size_t i = 0; i < e->m.size(); ++i) mask[i] = (!use || use[i]) ? 1 : 0;
    return OCN_OK;
}

static ocn_ens::Inflate *ens_inf_find(ocn_ens *e, int32_t field)
{
    for (ocn_ens::Inflate &q : e->inflate)
        if (q.field == field) return &q;
    return nullptr;
}

// buffer `which` (0: saved spread, 1: factor) of every listed field on every block, made where it is missing
static int ens_inf_buffers(ocn_ens *e, const int32_t *field_ids, int32_t nfields, int which)
{
    const ocn_ctx *c0 = e->m[0];
    const size_t nblk = c0->blocks.size();
    for (int32_t f = 0; f < nfields; ++f) {
        if (!ens_inf_find(e, field_ids[f])) {
            e->inflate.emplace_back();
            ocn_ens::Inflate &q = e->inflate.back();
            q.field = field_ids[f];
            for (int i = 0; i < 2; ++i) { q.raw[i].assign(nblk, nullptr); q.buf[i].assign(nblk, nullptr); }
        }
        ocn_ens::Inflate *q = ens_inf_find(e, field_ids[f]);
        for (size_t k = 0; k < nblk; ++k) {
            if (q->raw[which][k]) continue;
            const LBlock &b = c0->blocks[k];
            const size_t lead = (size_t)((uintptr_t)b.ptr[field_slot(field_ids[f])] & 255u);   // (as ocn_ens_stats' buffers)
            HIPCHK(hipMalloc(&q->raw[which][k], field_bytes(b) + 512));
            q->buf[which][k] = (double *)((char *)q->raw[which][k] + 256 + lead);
        }
    }
    return OCN_OK;
}

int ocn_ens_spread_save(ocn_ens *e, const int32_t *field_ids, int32_t nfields, const uint8_t *use)
{
    std::vector<ocn_ctx *> in;
    std::vector<uint8_t> mask;
    RC(ens_inf_check(e, "ens_spread_save", field_ids, nfields, use, in, mask));
    HIPCHK(hipSetDevice(e->device));
    // the buffers first (a failed allocation leaves the members and the earlier saves as they were)
    RC(ens_inf_buffers(e, field_ids, nfields, 0));
    for (ocn_ctx *c : in) RC(guarded(c, "ocn_ens_spread_save", [&] { return complete_open(c); }));
    const ocn_ctx *c0 = e->m[0];
    int rc = OCN_OK;
    std::vector<const double *> src(in.size());
    for (int32_t f = 0; f < nfields && !rc; ++f) {
        ocn_ens::Inflate *q = ens_inf_find(e, field_ids[f]);
        q->formed[0] = false;
        for (size_t k = 0; k < c0->blocks.size() && !rc; ++k) {
            for (size_t a = 0; a < in.size(); ++a) src[a] = (const double *)in[a]->blocks[k].ptr[field_slot(field_ids[f])];
            double *const out[5] = {nullptr, nullptr, q->buf[0][k], nullptr, nullptr};   // (SPREAD alone)
            rc = launch_ens_stats(&c0->blocks[k].g, src.data(), (int)src.size(), true, out, e->stream);
        }
        if (!rc) { q->formed[0] = true; q->in_use = mask; }
    }
    return rc;
}

int ocn_ens_inflate(ocn_ens *e, const int32_t *field_ids, int32_t nfields, const uint8_t *use, int32_t mode, double alpha)
{
    std::vector<ocn_ctx *> in;
    std::vector<uint8_t> mask;
    RC(ens_inf_check(e, "ens_inflate", field_ids, nfields, use, in, mask));
    if (mode != OCN_ENS_INFLATE_CONST && mode != OCN_ENS_INFLATE_RTPS) return set_error(OCN_ERR_ARG, "ens_inflate: mode = OCN_ENS_INFLATE_*");
    if (!std::isfinite(alpha)) return set_error(OCN_ERR_ARG, "ens_inflate: an alpha that is not finite");
    if (mode == OCN_ENS_INFLATE_RTPS && alpha < 0.0) return set_error(OCN_ERR_ARG, "ens_inflate: RTPS with alpha < 0");
    for (int32_t f = 0; f < nfields && mode == OCN_ENS_INFLATE_RTPS; ++f) {
        const ocn_ens::Inflate *q = ens_inf_find(e, field_ids[f]);
        if (!q || !q->formed[0]) return set_error(OCN_ERR_STATE, "ens_inflate: RTPS on a field with no saved spread (ocn_ens_spread_save)");
        if (q->in_use != mask) return set_error(OCN_ERR_STATE, "ens_inflate: the spread was saved over a different set of members");
    }
    HIPCHK(hipSetDevice(e->device));
    // the buffers first (a failed allocation leaves the members as they were)
    RC(ens_inf_buffers(e, field_ids, nfields, 1));
    for (ocn_ctx *c : in) RC(guarded(c, "ocn_ens_inflate", [&] { return complete_open(c); }));
    const ocn_ctx *c0 = e->m[0];
    const int n = (int)in.size();
    int rc = OCN_OK;
    std::vector<double *> mem((size_t)n);
    for (int32_t f = 0; f < nfields && !rc; ++f) {
        ocn_ens::Inflate *q = ens_inf_find(e, field_ids[f]);
        q->formed[1] = false;
        for (size_t k = 0; k < c0->blocks.size() && !rc; ++k) {
            for (int a = 0; a < n; ++a) mem[(size_t)a] = (double *)in[(size_t)a]->blocks[k].ptr[field_slot(field_ids[f])];
            rc = launch_ens_inflate(&c0->blocks[k].g, mem.data(), n, mode, alpha,
                                    mode == OCN_ENS_INFLATE_RTPS ? q->buf[0][k] : nullptr, q->buf[1][k], e->stream);
        }
        if (!rc) q->formed[1] = true;
    }
    // what ocn_ctx_upload of each of these fields leaves behind (also after a failed launch: the arrays
    // may have changed)
    for (ocn_ctx *c : in)
        for (int32_t f = 0; f < nfields; ++f) field_uploaded(c, field_ids[f]);
    return rc;
}

int ocn_ens_inflate_download(ocn_ens *e, int32_t k, int32_t field_id, int32_t what, double *host)
{
    if (!e || !host) return set_error(OCN_ERR_ARG, "ens_inflate_download: null argument");
    const ocn_ctx *c0 = e->m[0];
    if (k < 0 || k >= (int32_t)c0->blocks.size()) return set_error(OCN_ERR_ARG, "ens_inflate_download: bad block index");
    if (!has_r8(c0, field_id)) return set_error(OCN_ERR_ARG, "ens_inflate_download: not a real(8) field of the members");
    if (what != OCN_ENS_INFLATE_PRIOR_SPREAD && what != OCN_ENS_INFLATE_FACTOR)
        return set_error(OCN_ERR_ARG, "ens_inflate_download: what = OCN_ENS_INFLATE_PRIOR_SPREAD or OCN_ENS_INFLATE_FACTOR");
    const ocn_ens::Inflate *q = ens_inf_find(e, field_id);
    if (!q || !q->formed[what]) return set_error(OCN_ERR_STATE, "ens_inflate_download: that buffer of this field was never formed");
    HIPCHK(hipSetDevice(e->device));
    const ocn_block &g = c0->blocks[(size_t)k].g;
    const size_t w = (size_t)(g.bnd_x2 - g.bnd_x1 + 1), rows = (size_t)(g.bnd_y2 - g.bnd_y1 + 1);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy2D(host, w * 8, q->buf[what][(size_t)k], (size_t)g.pitch * 8, w * 8, rows, hipMemcpyDeviceToHost));
    return OCN_OK;
}

// ------------------------------------------------------------------ correlated perturbations (ens_perturb.hip)
// the sum of the squares of the box of width 2R+1 convolved with itself P times (the delta for P = 0)
static uint64_t ens_perturb_q(int reach, int passes)
{
    std::vector<uint64_t> k{1};
    for (int p = 0; p < passes; ++p) {
        std::vector<uint64_t> next(k.size() + 2 * (size_t)reach, 0);
        for (size_t t = 0; t < k.size(); ++t)
            for (int d = 0; d <= 2 * reach; ++d) next[t + (size_t)d] += k[t];
        k.swap(next);
    }
    uint64_t q = 0;
    for (uint64_t v : k) q += v * v;
    return q;
}

int ocn_ens_perturb(ocn_ens *e, const int32_t *field_ids, const int32_t *mask_ids, const uint32_t *draw, int32_t nfields,
                    const uint8_t *use, uint64_t seed, int32_t reach, int32_t passes, int32_t centre, double amplitude)
{
    if (!e || !field_ids || !mask_ids || !draw) return set_error(OCN_ERR_ARG, "ens_perturb: null argument");
    if (nfields < 1) return set_error(OCN_ERR_ARG, "ens_perturb: no field");
    const ocn_ctx *c0 = e->m[0];
    for (int32_t f = 0; f < nfields; ++f) {
        if (!has_r8(c0, field_ids[f])) return set_error(OCN_ERR_ARG, "ens_perturb: not a real(8) field of the members");
        for (int32_t q = 0; q < f; ++q)
            if (field_ids[q] == field_ids[f]) return set_error(OCN_ERR_ARG, "ens_perturb: a field named twice");
        if (mask_ids[f] != -1 && !is_r4(mask_ids[f])) return set_error(OCN_ERR_ARG, "ens_perturb: a mask that is neither -1 nor a real(4) field");
    }
    if (reach < 0 || reach > OCN_ENS_PERTURB_MAX_REACH) return set_error(OCN_ERR_ARG, "ens_perturb: reach outside 0..16");
    if (passes < 0 || passes > OCN_ENS_PERTURB_MAX_PASSES) return set_error(OCN_ERR_ARG, "ens_perturb: passes outside 0..3");
    if (!std::isfinite(amplitude) || !(amplitude > 0.0)) return set_error(OCN_ERR_ARG, "ens_perturb: an amplitude that is not finite and > 0");
    const std::vector<ocn_ctx *> in = ens_in_use(e, use);
    const int n = (int)in.size();
    if (n < 1) return set_error(OCN_ERR_ARG, "ens_perturb: no member in use");
    if (centre && n < 2) return set_error(OCN_ERR_ARG, "ens_perturb: centring with fewer than two members in use");
    uint64_t bound = (uint64_t)n << 19;   // n (2R+1)^(2P) 2^19: below 2^58 for every n, R and P allowed
    for (int p = 0; p < 2 * passes; ++p) bound *= (uint64_t)(2 * reach + 1);
    if (bound > (1ull << 53)) return set_error(OCN_ERR_ARG, "ens_perturb: n (2 reach + 1)^(2 passes) 2^19 > 2^53: not exact in double");
    HIPCHK(hipSetDevice(e->device));
    // the scratch first (a failed allocation leaves the members as they were)
    const size_t M = e->m.size(), nblk = c0->blocks.size();
    ocn_ens::Perturb &pt = e->perturb;
    if (pt.raw.empty()) { pt.raw.assign(nblk, nullptr); pt.z.assign(nblk, nullptr); pt.stride.assign(nblk, 0); pt.n.assign(nblk, 0); }
    for (size_t k = 0; k < nblk; ++k) {
        if (pt.raw[k]) continue;
        const LBlock &b = c0->blocks[k];
        const size_t lead = (size_t)((uintptr_t)b.ptr[field_slot(OCN_SSH)] & 255u);   // (as ocn_ens_stats' buffers)
        const size_t stride = (field_bytes(b) + 255) / 256 * 256;                     // (every member's array based alike)
        HIPCHK(hipMalloc(&pt.raw[k], stride * M + 512));
        pt.z[k] = (long long *)((char *)pt.raw[k] + 256 + lead);
        pt.stride[k] = (long)(stride / 8);
    }
    for (ocn_ctx *c : in) RC(guarded(c, "ocn_ens_perturb", [&] { return complete_open(c); }));
    std::vector<uint8_t> members;   // the members in use: their indices in the ensemble
    for (size_t i = 0; i < M; ++i)
        if (!use || use[i]) members.push_back((uint8_t)i);
    const double q = (double)ens_perturb_q(reach, passes);
    double den = 0x1.a20bd6fff1bdfp+15 * q;   // kSigma = sqrt(2 (2^32 - 1) / 3)
    if (centre) den = den * (double)n;
    const double coef = amplitude / den;
    int rc = OCN_OK;
    std::vector<double *> mem((size_t)n);
    for (int32_t f0 = 0; f0 < nfields && !rc; ++f0) {
        bool first = true;   // field f0 opens its draw id
        for (int32_t q0 = 0; q0 < f0; ++q0) first = first && draw[q0] != draw[f0];
        if (!first) continue;
        for (size_t k = 0; k < nblk && !rc; ++k) {
            const LBlock &b0 = c0->blocks[k];
            const int lead = (int)(((uintptr_t)pt.z[k] & 255u) / 8u);
            pt.n[k] = 0;
            rc = launch_ens_noise(&b0.g, members.data(), n, seed, draw[f0], reach, passes, pt.z[k], pt.stride[k], lead, e->stream);
            if (!rc) pt.n[k] = n;
            for (int32_t f = f0; f < nfields && !rc; ++f) {
                if (draw[f] != draw[f0]) continue;
                for (int a = 0; a < n; ++a) mem[(size_t)a] = (double *)in[(size_t)a]->blocks[k].ptr[field_slot(field_ids[f])];
                rc = launch_ens_perturb_apply(&b0.g, mem.data(), n, pt.z[k], pt.stride[k], centre != 0, coef,
                                              mask_ids[f] < 0 ? nullptr : b0.f<float>(mask_ids[f]), e->stream);
            }
        }
    }
    // what ocn_ctx_upload of each of these fields leaves behind (also after a failed launch: the arrays
    // may have changed)
    for (ocn_ctx *c : in)
        for (int32_t f = 0; f < nfields; ++f) field_uploaded(c, field_ids[f]);
    return rc;
}

int ocn_ens_perturb_download(ocn_ens *e, int32_t k, int32_t a, int64_t *host)
{
    if (!e || !host) return set_error(OCN_ERR_ARG, "ens_perturb_download: null argument");
    const ocn_ctx *c0 = e->m[0];
    if (k < 0 || k >= (int32_t)c0->blocks.size()) return set_error(OCN_ERR_ARG, "ens_perturb_download: bad block index");
    const ocn_ens::Perturb &pt = e->perturb;
    if (pt.n.empty() || pt.n[(size_t)k] < 1) return set_error(OCN_ERR_STATE, "ens_perturb_download: no ocn_ens_perturb on this block yet");
    if (a < 0 || a >= pt.n[(size_t)k]) return set_error(OCN_ERR_ARG, "ens_perturb_download: not a member in use of the last call");
    HIPCHK(hipSetDevice(e->device));
    const ocn_block &g = c0->blocks[(size_t)k].g;
    const size_t w = (size_t)(g.bnd_x2 - g.bnd_x1 + 1), rows = (size_t)(g.bnd_y2 - g.bnd_y1 + 1);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy2D(host, w * 8, pt.z[(size_t)k] + (size_t)a * (size_t)pt.stride[(size_t)k], (size_t)g.pitch * 8, w * 8, rows,
                       hipMemcpyDeviceToHost));
    return OCN_OK;
}

// ------------------------------------------------------------------ localized observation update (ens_local.hip)
// What ocn_ens_local_update and ocn_ens_assimilate check alike: the fields, the members in use, the counts,
// the observations within the basin, the taper.  `who` opens the message.
static int ens_lu_check(const ocn_ens *e, const std::string &who, const int32_t *field_ids, int32_t nfields,
                        const std::vector<ocn_ctx *> &in, int32_t nobs, const int32_t *io, const int32_t *jo,
                        const double *taper, int32_t ntaper)
{
    if (nfields < 1) return set_error(OCN_ERR_ARG, who + ": no field");
    const ocn_ctx *c0 = e->m[0];
    for (int32_t f = 0; f < nfields; ++f) {
        if (!has_r8(c0, field_ids[f])) return set_error(OCN_ERR_ARG, who + ": not a real(8) field of the members");
        for (int32_t q = 0; q < f; ++q)
            if (field_ids[q] == field_ids[f]) return set_error(OCN_ERR_ARG, who + ": a field named twice");
    }
    if (in.size() < 2) return set_error(OCN_ERR_ARG, who + ": fewer than two members in use");
    if (nobs < 1 || nobs > 8192) return set_error(OCN_ERR_ARG, who + ": 1..8192 observations");
    if (ntaper < 1 || ntaper > 65536) return set_error(OCN_ERR_ARG, who + ": a taper of 1..65536 entries");
    for (int32_t k = 0; k < nobs; ++k)
        if (io[k] < 1 || io[k] > c0->basin.nx || jo[k] < 1 || jo[k] > c0->basin.ny)
            return set_error(OCN_ERR_ARG, who + ": an observation outside the basin");
    for (int32_t q = 0; q < ntaper; ++q)
        if (!std::isfinite(taper[q])) return set_error(OCN_ERR_ARG, who + ": a taper entry that is not finite");
    return OCN_OK;
}

static int ens_lu_reach(int32_t ntaper)   // the largest r with r * r < ntaper
{
    int reach = 0;
    while ((reach + 1) * (reach + 1) < ntaper) ++reach;
    return reach;
}

// each block's list: the observations whose box meets the block's array, in the caller's order, filled up
// to groups of kLuGroup.  Returns the entries of all lists.
static size_t ens_lu_lists(const ocn_ctx *c0, int32_t nobs, const int32_t *io, const int32_t *jo, int reach,
                           std::vector<std::vector<EnsLuObs>> &lists)
{
    const size_t nblk = c0->blocks.size();
    lists.assign(nblk, {});
    size_t list_n = 0;
    for (size_t b = 0; b < nblk; ++b) {
        const ocn_block &g = c0->blocks[b].g;
        for (int32_t k = 0; k < nobs; ++k)
            if (io[k] + reach >= g.bnd_x1 && io[k] - reach <= g.bnd_x2 && jo[k] + reach >= g.bnd_y1 && jo[k] - reach <= g.bnd_y2)
                lists[b].push_back(EnsLuObs{io[k], jo[k], k, 0});
        while (lists[b].size() % kLuGroup) lists[b].push_back(ens_lu_filler());
        list_n += lists[b].size();
    }
    return list_n;
}

// the lists into the pinned table h from byte `at` on, one after another: list_at[b] the first byte of block b's
static void ens_lu_put_lists(const std::vector<std::vector<EnsLuObs>> &lists, char *h, size_t at, std::vector<size_t> &list_at)
{
    list_at.resize(lists.size());
    for (size_t b = 0; b < lists.size(); ++b) {
        list_at[b] = at;
        if (!lists[b].empty()) memcpy(h + at, lists[b].data(), lists[b].size() * sizeof(EnsLuObs));
        at += lists[b].size() * sizeof(EnsLuObs);
    }
}

// one launch per field and block that an observation reaches (d: the device table the lists are in), then
// what ocn_ctx_upload of each of these fields leaves behind (also after a failed launch: the arrays may
// have changed)
static int ens_lu_launches(const std::vector<ocn_ctx *> &in, const int32_t *field_ids, int32_t nfields,
                           const std::vector<std::vector<EnsLuObs>> &lists, const char *d, const std::vector<size_t> &list_at,
                           const double *d_y, const double *d_z, const double *d_taper, int32_t ntaper, int reach, hipStream_t s)
{
    const ocn_ctx *c0 = in[0];
    const int n = (int)in.size();
    int rc = OCN_OK;
    std::vector<double *> mem((size_t)n);
    for (int32_t f = 0; f < nfields && !rc; ++f)
        for (size_t k = 0; k < lists.size() && !rc; ++k) {
            if (lists[k].empty()) continue;   // no observation reaches this block
            for (int a = 0; a < n; ++a) mem[(size_t)a] = (double *)in[(size_t)a]->blocks[k].ptr[field_slot(field_ids[f])];
            rc = launch_ens_local(&c0->blocks[k].g, mem.data(), n, (const EnsLuObs *)(d + list_at[k]),
                                  (int)(lists[k].size() / kLuGroup), d_y, d_z, d_taper, ntaper, reach, s);
        }
    for (ocn_ctx *c : in)
        for (int32_t f = 0; f < nfields; ++f) field_uploaded(c, field_ids[f]);
    return rc;
}

int ocn_ens_local_update(ocn_ens *e, const int32_t *field_ids, int32_t nfields, const uint8_t *use, int32_t nobs,
                         const int32_t *io, const int32_t *jo, const double *y, const double *z, const double *taper,
                         int32_t ntaper)
{
    if (!e || !field_ids || !io || !jo || !y || !z || !taper) return set_error(OCN_ERR_ARG, "ens_local_update: null argument");
    const ocn_ctx *c0 = e->m[0];
    const std::vector<ocn_ctx *> in = ens_in_use(e, use);
    RC(ens_lu_check(e, "ens_local_update", field_ids, nfields, in, nobs, io, jo, taper, ntaper));
    const int n = (int)in.size();
    for (size_t q = 0; q < (size_t)nobs * n; ++q)
        if (!std::isfinite(y[q]) || !std::isfinite(z[q])) return set_error(OCN_ERR_ARG, "ens_local_update: a y or z that is not finite");
    const int reach = ens_lu_reach(ntaper);
    std::vector<std::vector<EnsLuObs>> lists;
    const size_t list_n = ens_lu_lists(c0, nobs, io, jo, reach, lists);
    HIPCHK(hipSetDevice(e->device));
    // the buffers first (a failed allocation leaves the members as they were): rows, taper, lists
    const size_t rows_b = (size_t)nobs * ens_lu_row(n) * sizeof(double), tap_b = ((size_t)ntaper * sizeof(double) + 255) / 256 * 256,
                 need = 2 * rows_b + tap_b + list_n * sizeof(EnsLuObs);
    if (!e->ev_lu) HIPCHK(hipEventCreateWithFlags(&e->ev_lu, hipEventDisableTiming));
    if (e->lu_bytes < need) {
        if (e->ev_lu_set) HIPCHK(hipEventSynchronize(e->ev_lu));
        if (e->d_lu) (void)hipFree(e->d_lu);   // (waits for the launches that use it)
        if (e->h_lu) (void)hipHostFree(e->h_lu);
        e->d_lu = e->h_lu = nullptr;
        e->lu_bytes = 0;
        const size_t grown = (need + 65535) / 65536 * 65536;
        HIPCHK(hipMalloc(&e->d_lu, grown));
        HIPCHK(hipHostMalloc(&e->h_lu, grown, hipHostMallocDefault));
        e->lu_bytes = grown;
    }
    for (ocn_ctx *c : in) RC(guarded(c, "ocn_ens_local_update", [&] { return complete_open(c); }));
    // the tables up from pinned memory ahead of the launches
    if (e->ev_lu_set) HIPCHK(hipEventSynchronize(e->ev_lu));
    char *h = (char *)e->h_lu, *d = (char *)e->d_lu;
    const size_t row = ens_lu_row(n);
    double *hy = (double *)h, *hz = (double *)(h + rows_b);
    std::fill(hy, hy + 2 * (size_t)nobs * row, 0.0);   // (the padding of the rows: read, never used)
    for (int32_t k = 0; k < nobs; ++k)
        for (int m = 0; m < n; ++m) {
            hy[(size_t)k * row + m] = y[(size_t)k * n + m];
            hz[(size_t)k * row + m] = z[(size_t)k * n + m];
        }
    memcpy(h + 2 * rows_b, taper, (size_t)ntaper * sizeof(double));
    std::vector<size_t> list_at;
    ens_lu_put_lists(lists, h, 2 * rows_b + tap_b, list_at);
    HIPCHK(hipMemcpyAsync(d, h, need, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipEventRecord(e->ev_lu, e->stream));
    e->ev_lu_set = true;
    return ens_lu_launches(in, field_ids, nfields, lists, d, list_at, (const double *)d, (const double *)(d + rows_b),
                           (const double *)(d + 2 * rows_b), ntaper, reach, e->stream);
}

// ------------------------------------------------------------------ the serial filter on the device (ens_assim.hip)
// Launches per call: kAsLaunches for the observation-space stage (k_ens_obs_space, k_ens_obs_space_h behind a
// sparse linear observation operator, or k_ens_obs_space_r behind the recorder's series; whatever n and nobs; with
// ocn_ens_set_gate their _g, _hg, _rg instances, which also rewrite the update's lists on the device),
// then ocn_ens_local_update's: one per listed field and block that an observation reaches -- also with a gate: the
// host does not know what was rejected.
constexpr int kAsLaunches = 1;
static_assert(kAsLaunches == 1, "ocn_sw.h and DESIGN.md state this count");

// the local block a global point is read in -- the one whose interior holds it, else the first whose array
// does -- or -1
static int ens_block_of(const ocn_ctx *c0, int32_t i, int32_t j)
{
    const size_t nblk = c0->blocks.size();
    for (size_t b = 0; b < nblk; ++b) {
        const ocn_block &g = c0->blocks[b].g;
        if (i >= g.nx_start && i <= g.nx_end && j >= g.ny_start && j <= g.ny_end) return (int)b;
    }
    for (size_t b = 0; b < nblk; ++b) {
        const ocn_block &g = c0->blocks[b].g;
        if (i >= g.bnd_x1 && i <= g.bnd_x2 && j >= g.bnd_y1 && j <= g.bnd_y2) return (int)b;
    }
    return -1;
}

// What ocn_ens_assimilate and ocn_ens_assimilate_h check alike beyond ens_lu_check: the observed values
static int ens_as_check(const std::string &who, int32_t nobs, const double *value, const double *variance)
{
    for (int32_t k = 0; k < nobs; ++k) {
        if (!std::isfinite(value[k])) return set_error(OCN_ERR_ARG, who + ": a value that is not finite");
        if (!std::isfinite(variance[k]) || !(variance[k] > 0.0))
            return set_error(OCN_ERR_ARG, who + ": a variance that is not finite and positive");
    }
    return OCN_OK;
}

// A sparse linear observation operator (ocn_sw.h ocn_ens_sample_h), validated and resolved for n members in
// use: its distinct fields in the order of their first term, and each term's pointer-table slot
// (field slot * blocks + block) * n, element offset and weight.  Nothing is read beyond a bad row.
struct EnsObsHost { std::vector<int32_t> fields; std::vector<EnsObsTerm> term; };

static int ens_obs_resolve(const ocn_ctx *c0, const std::string &who, size_t n, int32_t nobs, const int32_t *start,
                           const int32_t *tfield, const int32_t *ti, const int32_t *tj, const double *tw, EnsObsHost &h)
{
    if (start[0] != 0) return set_error(OCN_ERR_ARG, who + ": start[0] is not 0");
    const size_t nblk = c0->blocks.size();
    for (int32_t j = 0; j < nobs; ++j) {
        const int64_t terms = (int64_t)start[j + 1] - start[j];
        if (terms < 1 || terms > OCN_ENS_OBS_MAX_TERMS)
            return set_error(OCN_ERR_ARG, who + ": an observation with 0 or more than 16 terms");
        for (int32_t t = start[j]; t < start[j + 1]; ++t) {
            if (!std::isfinite(tw[t]) || tw[t] == 0.0) return set_error(OCN_ERR_ARG, who + ": a weight that is zero or not finite");
            if (!has_r8(c0, tfield[t])) return set_error(OCN_ERR_ARG, who + ": a term's field is not a real(8) field of the members");
            size_t f = 0;
            while (f < h.fields.size() && h.fields[f] != tfield[t]) ++f;
            if (f == h.fields.size()) {
                if (f == OCN_ENS_OBS_MAX_FIELDS) return set_error(OCN_ERR_ARG, who + ": more than 4 distinct fields");
                h.fields.push_back(tfield[t]);
            }
            const int at = ens_block_of(c0, ti[t], tj[t]);
            if (at < 0) return set_error(OCN_ERR_ARG, who + ": a term in no local block's array");
            const ocn_block &g = c0->blocks[(size_t)at].g;
            h.term.push_back(EnsObsTerm{(long)((f * nblk + (size_t)at) * n),
                                        (long)(tj[t] - g.bnd_y1) * (long)g.pitch + (ti[t] - g.bnd_x1), tw[t]});
        }
    }
    return OCN_OK;
}

// the pointer table of `fields` over the blocks and the members in use, as the field tables name the arrays now
static void ens_obs_table(const std::vector<ocn_ctx *> &in, const std::vector<int32_t> &fields, const double **tab)
{
    const size_t n = in.size(), nblk = in[0]->blocks.size();
    for (size_t f = 0; f < fields.size(); ++f)
        for (size_t b = 0; b < nblk; ++b)
            for (size_t m = 0; m < n; ++m)
                tab[(f * nblk + b) * n + m] = (const double *)in[m]->blocks[b].ptr[field_slot(fields[f])];
}

// ocn_ens_assimilate, ocn_ens_assimilate_h and ocn_ens_assimilate_rec behind their checks.  The prologue reads
// `src`, the fields of the pointer table: one field at the points (off, blk), or with `start` the operator's
// terms; or, with `robs`, no field at all but the recorder's series at robs[j] in the columns `col`.
static int ens_as_run(ocn_ens *e, const char *entry, const std::vector<ocn_ctx *> &in, const int32_t *field_ids, int32_t nfields,
                      int32_t nobs, const int32_t *io, const int32_t *jo, const double *value, const double *variance,
                      const double *taper, int32_t ntaper, const std::vector<int32_t> &src, const std::vector<long> &off,
                      const std::vector<int> &blk, const int32_t *start, const std::vector<EnsObsTerm> &term,
                      const std::vector<EnsRecObs> &robs = {}, const std::vector<int> &col = {})
{
    const ocn_ctx *c0 = e->m[0];
    const size_t n = in.size(), nblk = c0->blocks.size(), no = (size_t)nobs;
    const int reach = ens_lu_reach(ntaper);
    std::vector<std::vector<EnsLuObs>> lists;
    const size_t list_n = ens_lu_lists(c0, nobs, io, jo, reach, lists);
    HIPCHK(hipSetDevice(e->device));
    // one layout on both sides, every part on a 256-B line: the tables that go up, then what the device forms
    auto part = [](size_t at, size_t bytes) { return at + (bytes + 255) / 256 * 256; };
    const size_t row = ens_lu_row((int)n), rows_b = no * row * sizeof(double);
    const size_t tap_at = 0, list_at0 = part(tap_at, (size_t)ntaper * sizeof(double)), val_at = part(list_at0, list_n * sizeof(EnsLuObs)),
                 var_at = part(val_at, no * 8), off_at = part(var_at, no * 8), io_at = part(off_at, off.size() * sizeof(long)),
                 jo_at = part(io_at, no * 4), blk_at = part(jo_at, no * 4), start_at = part(blk_at, blk.size() * 4),
                 term_at = part(start_at, start ? (no + 1) * 4 : 0), robs_at = part(term_at, term.size() * sizeof(EnsObsTerm)),
                 col_at = part(robs_at, robs.size() * sizeof(EnsRecObs)), tab_at = part(col_at, col.size() * sizeof(int)),
                 up_b = part(tab_at, src.size() * nblk * n * sizeof(double *)), hx_at = up_b, y_at = part(hx_at, rows_b),
                 z_at = part(y_at, rows_b), vec_at = part(z_at, rows_b), count_at = part(vec_at, 3 * no * 8),
                 accept_at = part(count_at, sizeof(long)), need = part(accept_at, no * 8);
    const bool gated = e->gate2 != 0.0;
    // the buffers first (a failed allocation leaves the members as they were, and no earlier result)
    if (!e->ev_as) HIPCHK(hipEventCreateWithFlags(&e->ev_as, hipEventDisableTiming));
    const bool timed = e->as_timing;
    for (int i = 0; i < 3 && timed; ++i)
        if (!e->ev_t[i]) HIPCHK(hipEventCreate(&e->ev_t[i]));
    if (e->as_bytes < need) {
        if (e->ev_as_set) HIPCHK(hipEventSynchronize(e->ev_as));
        if (e->d_as) (void)hipFree(e->d_as);   // (waits for the launches that use it)
        if (e->h_as) (void)hipHostFree(e->h_as);
        e->d_as = e->h_as = nullptr;
        e->as_bytes = 0;
        e->as_last = ocn_ens::AsLast{};
        const size_t grown = (need + 65535) / 65536 * 65536;
        HIPCHK(hipMalloc(&e->d_as, grown));
        HIPCHK(hipHostMalloc(&e->h_as, grown, hipHostMallocDefault));
        e->as_bytes = grown;
    }
    for (ocn_ctx *c : in) RC(guarded(c, entry, [&] { return complete_open(c); }));
    // the tables up from pinned memory in one copy, ahead of the launches; the members' arrays as the field
    // tables name them now
    if (e->ev_as_set) HIPCHK(hipEventSynchronize(e->ev_as));
    char *h = (char *)e->h_as, *d = (char *)e->d_as;
    memcpy(h + tap_at, taper, (size_t)ntaper * sizeof(double));
    std::vector<size_t> list_at;
    ens_lu_put_lists(lists, h, list_at0, list_at);
    memcpy(h + val_at, value, no * 8);
    memcpy(h + var_at, variance, no * 8);
    memcpy(h + io_at, io, no * 4);
    memcpy(h + jo_at, jo, no * 4);
    if (!robs.empty()) {
        memcpy(h + robs_at, robs.data(), robs.size() * sizeof(EnsRecObs));
        memcpy(h + col_at, col.data(), col.size() * sizeof(int));
    } else if (start) {
        memcpy(h + start_at, start, (no + 1) * 4);
        memcpy(h + term_at, term.data(), term.size() * sizeof(EnsObsTerm));
    } else {
        memcpy(h + off_at, off.data(), no * sizeof(long));
        memcpy(h + blk_at, blk.data(), no * 4);
    }
    ens_obs_table(in, src, (const double **)(h + tab_at));
    e->as_last = ocn_ens::AsLast{};   // (the results of the call before are overwritten from here on)
    HIPCHK(hipMemcpyAsync(d, h, up_b, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipEventRecord(e->ev_as, e->stream));
    e->ev_as_set = true;
    EnsAsArgs a{};
    a.tab = (const double *const *)(d + tab_at); a.off = (const long *)(d + off_at); a.blk = (const int *)(d + blk_at);
    a.io = (const int *)(d + io_at); a.jo = (const int *)(d + jo_at);
    a.value = (const double *)(d + val_at); a.variance = (const double *)(d + var_at); a.taper = (const double *)(d + tap_at);
    a.hx = (double *)(d + hx_at); a.y = (double *)(d + y_at); a.z = (double *)(d + z_at);
    a.innovation = (double *)(d + vec_at); a.prior = a.innovation + no; a.posterior = a.prior + no;
    a.nonfinite = (long *)(d + count_at);
    a.row = (long)row; a.n = (int)n; a.nobs = nobs; a.ntaper = ntaper; a.reach = reach;
    // the gate: the lists' device copy, every block's one after another, for the stage's epilogue to rewrite
    const EnsAsGate g{e->gate2, (double *)(d + accept_at), (EnsLuObs *)(d + list_at0), (int)list_n};
    if (timed) HIPCHK(hipEventRecord(e->ev_t[0], e->stream));
    if (!robs.empty()) {
        const ocn_ens::Recorder &r = e->rec;
        const EnsRecSrc rs{(const double *)r.d_series, (const EnsRecObs *)(d + robs_at), (const int *)(d + col_at),
                           (long)r.nobs * (long)r.n};
        RC(gated ? launch_ens_obs_space_rg(a, rs, g, e->stream) : launch_ens_obs_space_r(a, rs, e->stream));
    } else if (start) {
        const EnsObsOp op{a.tab, (const int *)(d + start_at), (const EnsObsTerm *)(d + term_at)};
        RC(gated ? launch_ens_obs_space_hg(a, op, g, e->stream) : launch_ens_obs_space_h(a, op, e->stream));
    } else {
        RC(gated ? launch_ens_obs_space_g(a, g, e->stream) : launch_ens_obs_space(a, e->stream));
    }
    if (timed) HIPCHK(hipEventRecord(e->ev_t[1], e->stream));
    const int rc = ens_lu_launches(in, field_ids, nfields, lists, d, list_at, a.y, a.z, a.taper, ntaper, reach, e->stream);
    if (timed) HIPCHK(hipEventRecord(e->ev_t[2], e->stream));
    if (!rc) e->as_last = ocn_ens::AsLast{nobs, (int)n, row, hx_at, vec_at, count_at, timed, accept_at, gated};
    return rc;
}

int ocn_ens_assimilate(ocn_ens *e, int32_t obs_field, const int32_t *field_ids, int32_t nfields, const uint8_t *use,
                       int32_t nobs, const int32_t *io, const int32_t *jo, const double *value, const double *variance,
                       const double *taper, int32_t ntaper)
{
    if (!e || !field_ids || !io || !jo || !value || !variance || !taper) return set_error(OCN_ERR_ARG, "ens_assimilate: null argument");
    const ocn_ctx *c0 = e->m[0];
    const std::vector<ocn_ctx *> in = ens_in_use(e, use);
    RC(ens_lu_check(e, "ens_assimilate", field_ids, nfields, in, nobs, io, jo, taper, ntaper));
    if (!has_r8(c0, obs_field)) return set_error(OCN_ERR_ARG, "ens_assimilate: the observed field is not a real(8) field of the members");
    RC(ens_as_check("ens_assimilate", nobs, value, variance));
    // each observation's block and its element there
    const size_t no = (size_t)nobs;
    std::vector<long> off(no);
    std::vector<int> blk(no);
    for (size_t k = 0; k < no; ++k) {
        const int at = ens_block_of(c0, io[k], jo[k]);
        if (at < 0) return set_error(OCN_ERR_ARG, "ens_assimilate: an observation in no local block's array");
        const ocn_block &g = c0->blocks[(size_t)at].g;
        blk[k] = at;
        off[k] = (long)(jo[k] - g.bnd_y1) * (long)g.pitch + (io[k] - g.bnd_x1);
    }
    return ens_as_run(e, "ocn_ens_assimilate", in, field_ids, nfields, nobs, io, jo, value, variance, taper, ntaper, {obs_field},
                      off, blk, nullptr, {});
}

int ocn_ens_assimilate_h(ocn_ens *e, const int32_t *field_ids, int32_t nfields, const uint8_t *use, int32_t nobs,
                         const int32_t *io, const int32_t *jo, const int32_t *start, const int32_t *tfield, const int32_t *ti,
                         const int32_t *tj, const double *tw, const double *value, const double *variance, const double *taper,
                         int32_t ntaper)
{
    if (!e || !field_ids || !io || !jo || !start || !tfield || !ti || !tj || !tw || !value || !variance || !taper)
        return set_error(OCN_ERR_ARG, "ens_assimilate_h: null argument");
    const std::vector<ocn_ctx *> in = ens_in_use(e, use);
    RC(ens_lu_check(e, "ens_assimilate_h", field_ids, nfields, in, nobs, io, jo, taper, ntaper));
    RC(ens_as_check("ens_assimilate_h", nobs, value, variance));
    EnsObsHost h;
    RC(ens_obs_resolve(e->m[0], "ens_assimilate_h", in.size(), nobs, start, tfield, ti, tj, tw, h));
    return ens_as_run(e, "ocn_ens_assimilate_h", in, field_ids, nfields, nobs, io, jo, value, variance, taper, ntaper, h.fields,
                      {}, {}, start, h.term);
}

// ocn_ens_sample with the operator in the points' place, in ocn_ens_sample's buffers
int ocn_ens_sample_h(ocn_ens *e, const uint8_t *use, int32_t nobs, const int32_t *start, const int32_t *tfield,
                     const int32_t *ti, const int32_t *tj, const double *tw, double *host)
{
    if (!e || !start || !tfield || !ti || !tj || !tw || !host) return set_error(OCN_ERR_ARG, "ens_sample_h: null argument");
    if (nobs < 1 || nobs > 65536) return set_error(OCN_ERR_ARG, "ens_sample_h: 1..65536 observations");
    const ocn_ctx *c0 = e->m[0];
    const std::vector<ocn_ctx *> in = ens_in_use(e, use);
    if (in.empty()) return set_error(OCN_ERR_ARG, "ens_sample_h: no member in use");
    const size_t n = in.size(), nblk = c0->blocks.size(), no = (size_t)nobs;
    EnsObsHost h;
    RC(ens_obs_resolve(c0, "ens_sample_h", n, nobs, start, tfield, ti, tj, tw, h));
    HIPCHK(hipSetDevice(e->device));
    // one layout on both sides: the rows' starts, the terms, the members' arrays per field and block (up), the
    // results (down)
    const size_t start_b = ((no + 1) * 4 + 7) / 8 * 8, term_b = h.term.size() * sizeof(EnsObsTerm),
                 tab_b = h.fields.size() * nblk * n * sizeof(double *), up_b = start_b + term_b + tab_b, res_b = no * n * sizeof(double);
    if (e->samp_bytes < up_b + res_b) {   // (a synchronous entry: nothing in flight reads the old ones)
        if (e->d_samp) (void)hipFree(e->d_samp);
        if (e->h_samp) (void)hipHostFree(e->h_samp);
        e->d_samp = e->h_samp = nullptr;
        e->samp_bytes = 0;
        HIPCHK(hipMalloc(&e->d_samp, up_b + res_b));
        HIPCHK(hipHostMalloc(&e->h_samp, up_b + res_b, hipHostMallocDefault));
        e->samp_bytes = up_b + res_b;
    }
    char *d = (char *)e->d_samp, *hp = (char *)e->h_samp;
    memcpy(hp, start, (no + 1) * 4);
    memcpy(hp + start_b, h.term.data(), term_b);
    // the members in use: their pending call tails formed, their arrays as the field tables name them now
    for (ocn_ctx *c : in) RC(guarded(c, "ocn_ens_sample_h", [&] { return complete_open(c); }));
    ens_obs_table(in, h.fields, (const double **)(hp + start_b + term_b));
    HIPCHK(hipMemcpyAsync(d, hp, up_b, hipMemcpyHostToDevice, e->stream));
    const EnsObsOp op{(const double *const *)(d + start_b + term_b), (const int *)d, (const EnsObsTerm *)(d + start_b)};
    RC(launch_ens_sample_h(op, (int)n, nobs, (double *)(d + up_b), e->stream));
    HIPCHK(hipMemcpyAsync(hp + up_b, d + up_b, res_b, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    memcpy(host, hp + up_b, res_b);
    return OCN_OK;
}

// ------------------------------------------------------------------ the station recorder (ocn_sw.h ocn_ens_record_*)
int ocn_ens_record_due(int64_t counted, int32_t nsteps, int32_t every, int32_t *steps, int32_t cap, int32_t *count)
{
    if (counted < 0 || nsteps < 0 || every < 1 || cap < 0 || (cap > 0 && !steps))
        return set_error(OCN_ERR_ARG, "ens_record_due: counted >= 0, nsteps >= 0, every >= 1, cap >= 0 with an array");
    std::vector<int32_t> due;
    ens_record_due(counted, nsteps, every, due);
    if (count) *count = (int32_t)due.size();
    for (size_t i = 0; i < due.size() && (int32_t)i < cap; ++i) steps[i] = due[i];
    return OCN_OK;
}

int ocn_ens_record_begin(ocn_ens *e, const uint8_t *use, int32_t nobs, const int32_t *start, const int32_t *tfield,
                         const int32_t *ti, const int32_t *tj, const double *tw, int32_t every, int32_t max_records)
{
    if (!e || !start || !tfield || !ti || !tj || !tw) return set_error(OCN_ERR_ARG, "ens_record_begin: null argument");
    if (nobs < 1 || nobs > 65536) return set_error(OCN_ERR_ARG, "ens_record_begin: 1..65536 observations");
    if (every < 1 || max_records < 1) return set_error(OCN_ERR_ARG, "ens_record_begin: every >= 1 and max_records >= 1");
    const ocn_ctx *c0 = e->m[0];
    const std::vector<ocn_ctx *> in = ens_in_use(e, use);
    if (in.empty()) return set_error(OCN_ERR_ARG, "ens_record_begin: no member in use");
    const size_t n = in.size(), nblk = c0->blocks.size(), no = (size_t)nobs, M = e->m.size();
    EnsObsHost h;
    RC(ens_obs_resolve(c0, "ens_record_begin", n, nobs, start, tfield, ti, tj, tw, h));
    for (int32_t f : h.fields)   // (everything else is formed by a call's tail only)
        if (f != OCN_SSH && f != OCN_SSHP && f != OCN_UBRTR && f != OCN_UBRTRP && f != OCN_VBRTR && f != OCN_VBRTRP)
            return set_error(OCN_ERR_ARG, "ens_record_begin: a term's field is not one of ssh, sshp, ubrtr, ubrtrp, vbrtr, vbrtrp");
    const size_t series_b = (size_t)max_records * no * n * sizeof(double);
    if (series_b > ((size_t)1 << 30)) return set_error(OCN_ERR_ARG, "ens_record_begin: a series above 1 GiB");
    HIPCHK(hipSetDevice(e->device));
    // the new recorder whole before the earlier one goes (a failed allocation keeps that one)
    ocn_ens::Recorder r;
    const size_t nt = h.term.size(), start_b = ((no + 1) * 4 + 255) / 256 * 256, term_b = (nt * sizeof(EnsObsTerm) + 255) / 256 * 256;
    r.start_at = 0; r.term_at = start_b; r.lterm_at = start_b + term_b;
    r.tab_b = (h.fields.size() * nblk * n * sizeof(double *) + 255) / 256 * 256;
    // (the stage: the launches' tables and 16 gathers' to begin with; a call that needs more grows it)
    r.stage_bytes = (M * sizeof(EnsRecMember) + 255) / 256 * 256 + 16 * r.tab_b;
    int rc = check_hip(hipMalloc(&r.d_series, series_b), "hipMalloc");
    if (!rc) rc = check_hip(hipMalloc(&r.d_op, start_b + 2 * term_b), "hipMalloc");
    if (!rc) rc = check_hip(hipMalloc(&r.d_stage, r.stage_bytes), "hipMalloc");
    for (int i = 0; i < 2 && !rc; ++i) {
        rc = check_hip(hipHostMalloc(&r.h_stage[i], r.stage_bytes, hipHostMallocDefault), "hipHostMalloc");
        if (!rc) rc = check_hip(hipEventCreateWithFlags(&r.ev[i], hipEventDisableTiming), "hipEventCreate");
    }
    // the operator up (synchronous: new memory that nothing in flight reads); the launch's terms name the field
    // by its index in `field` (one block: slot = index * n)
    std::vector<EnsObsTerm> lterm(h.term);
    for (EnsObsTerm &q : lterm) q.slot = nblk == 1 ? q.slot / (long)n : 0;
    if (!rc) rc = check_hip(hipMemcpy((char *)r.d_op + r.start_at, start, (no + 1) * 4, hipMemcpyHostToDevice), "hipMemcpy");
    if (!rc) rc = check_hip(hipMemcpy((char *)r.d_op + r.term_at, h.term.data(), nt * sizeof(EnsObsTerm), hipMemcpyHostToDevice), "hipMemcpy");
    if (!rc) rc = check_hip(hipMemcpy((char *)r.d_op + r.lterm_at, lterm.data(), nt * sizeof(EnsObsTerm), hipMemcpyHostToDevice), "hipMemcpy");
    if (rc) {
        ocn_ens::Recorder keep = std::move(e->rec);
        e->rec = std::move(r);
        ens_rec_free(e);
        e->rec = std::move(keep);
        return rc;
    }
    ens_rec_free(e);
    r.active = true;
    r.nobs = nobs; r.n = (int32_t)n; r.every = every; r.max_records = max_records;
    r.use.assign(M, 0);
    for (size_t i = 0; i < M; ++i) r.use[i] = (!use || use[i]) ? 1 : 0;
    r.field = h.fields;
    e->rec = std::move(r);
    return OCN_OK;
}

int ocn_ens_record_end(ocn_ens *e)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    if (!e->rec.active) return set_error(OCN_ERR_STATE, "ens_record_end: no recorder (ocn_ens_record_begin)");
    HIPCHK(hipSetDevice(e->device));
    ens_rec_free(e);
    return OCN_OK;
}

int ocn_ens_record_info(ocn_ens *e, ocn_ens_record_info_t *out)
{
    if (!e || !out) return set_error(OCN_ERR_ARG, "ens_record_info: null argument");
    const ocn_ens::Recorder &r = e->rec;
    *out = ocn_ens_record_info_t{r.active ? 1 : 0, r.nobs, r.n, r.every, r.max_records, 0, r.steps, (int64_t)r.records, r.in_launch};
    return OCN_OK;
}

int ocn_ens_record_download(ocn_ens *e, int32_t first, int32_t count, double *host)
{
    if (!e || !host) return set_error(OCN_ERR_ARG, "ens_record_download: null argument");
    const ocn_ens::Recorder &r = e->rec;
    if (!r.active) return set_error(OCN_ERR_STATE, "ens_record_download: no recorder (ocn_ens_record_begin)");
    if (first < 0 || count < 0 || (int64_t)first + count > r.records)
        return set_error(OCN_ERR_ARG, "ens_record_download: a range outside the records taken");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const size_t rb = (size_t)r.nobs * (size_t)r.n * sizeof(double);
    if (count) HIPCHK(hipMemcpy(host, (const char *)r.d_series + (size_t)first * rb, (size_t)count * rb, hipMemcpyDeviceToHost));
    return OCN_OK;
}

// The stage of one recording call: `need` bytes in the copy whose turn it is, read by the stream no more.
// Growing it waits for the device (rare: a call with more than 16 gathers after ocn_ens_record_begin).
static int ens_rec_stage(ocn_ens *e, size_t need)
{
    ocn_ens::Recorder &r = e->rec;
    if (need > r.stage_bytes) {
        for (int i = 0; i < 2; ++i)
            if (r.ev_set[i]) HIPCHK(hipEventSynchronize(r.ev[i]));
        const size_t grown = (need + 65535) / 65536 * 65536;
        void *d = nullptr, *h[2] = {nullptr, nullptr};
        int rc = check_hip(hipMalloc(&d, grown), "hipMalloc");
        for (int i = 0; i < 2 && !rc; ++i) rc = check_hip(hipHostMalloc(&h[i], grown, hipHostMallocDefault), "hipHostMalloc");
        if (rc) {
            if (d) (void)hipFree(d);
            for (void *p : h)
                if (p) (void)hipHostFree(p);
            return rc;
        }
        (void)hipFree(r.d_stage);   // (waits for the launches that use it)
        for (int i = 0; i < 2; ++i) { (void)hipHostFree(r.h_stage[i]); r.h_stage[i] = h[i]; r.ev_set[i] = false; }
        r.d_stage = d;
        r.stage_bytes = grown;
    }
    r.slot ^= 1;
    if (r.ev_set[r.slot]) HIPCHK(hipEventSynchronize(r.ev[r.slot]));
    return OCN_OK;
}

// record `index` gathered from the members in use as their field tables name the arrays now: the pointer table
// at `at` of the call's stage up, then k_ens_sample_h into the record's slot.  No wait.
static int ens_rec_gather(ocn_ens *e, const std::vector<ocn_ctx *> &in, int32_t index, size_t at)
{
    const ocn_ens::Recorder &r = e->rec;
    ens_obs_table(in, r.field, (const double **)((char *)r.h_stage[r.slot] + at));
    HIPCHK(hipMemcpyAsync((char *)r.d_stage + at, (const char *)r.h_stage[r.slot] + at, r.tab_b, hipMemcpyHostToDevice, e->stream));
    const char *d = (const char *)r.d_op;
    const EnsObsOp op{(const double *const *)((const char *)r.d_stage + at), (const int *)(d + r.start_at),
                      (const EnsObsTerm *)(d + r.term_at)};
    return launch_ens_sample_h(op, r.n, r.nobs, (double *)r.d_series + (size_t)index * (size_t)r.nobs * (size_t)r.n, e->stream);
}

int ocn_ens_step_record(ocn_ens *e, double tau, int32_t nsteps, int32_t check_every)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    ocn_ens::Recorder &r = e->rec;
    if (!r.active) return set_error(OCN_ERR_STATE, "ens_step_record: no recorder (ocn_ens_record_begin)");
    if (nsteps < 0) return set_error(OCN_ERR_ARG, "nsteps < 0");
    for (const ocn_ctx *c : e->m)
        if (!c->initialized) return set_error(OCN_ERR_STATE, "ocn_ctx_init_state not called");
    std::vector<int32_t> due;
    ens_record_due(r.steps, nsteps, r.every, due);
    if ((int64_t)r.records + (int64_t)due.size() > r.max_records)
        return set_error(OCN_ERR_ARG, "ens_step_record: the call's records would pass max_records");
    if (nsteps == 0) return OCN_OK;
    HIPCHK(hipSetDevice(e->device));
    const int M = (int)e->m.size();
    const std::vector<ocn_ctx *> in = ens_in_use(e, r.use.data());
    int first = OCN_OK;
    auto note = [&](int rc) { if (rc && !first) first = rc; };
    const size_t mem_b = ((size_t)M * sizeof(EnsRecMember) + 255) / 256 * 256;

    // In the launch only if every member in use would go in a recording launch -- known before any step of
    // the call runs (a member that has stepped without its records cannot be repaired): each member says
    // whether it would plan a multi-step launch (step_impl's probe), the planner whether it lands in a group
    // under the recording capacity.  The call itself then plans the same way.
    EnsRecCall rc_call{std::min<int64_t>(ens_capacity(e), onepass_multi_rec_capacity()), std::vector<int>((size_t)M, -1), 0, nullptr};
    bool in_launch = e->rec_in_launch && nsteps >= 2 && e->m[0]->blocks.size() == 1;
    if (in_launch) {
        std::vector<int32_t> variant((size_t)M, -1);
        for (int i = 0; i < M; ++i) {
            ocn_ctx *c = e->m[(size_t)i];
            c->ens_probe = true;
            const int rc = guarded(c, "ocn_ens_step_record", [&] { return step_entry(c, tau, nsteps, check_every); });
            c->ens_probe = false;
            if (!rc) variant[(size_t)i] = ens_variant(c, tau, check_every == 1);
            c->ens_pending = false;
        }
        std::vector<ocn_ens_group> groups;
        if (ens_groups(e, variant, rc_call.capacity, groups)) in_launch = false;
        std::vector<char> grouped((size_t)M, 0);
        for (const ocn_ens_group &q : groups)
            for (int j = 0; j < q.members; ++j) grouped[(size_t)q.member[j]] = 1;
        for (int i = 0, col = 0; i < M; ++i) {
            if (!r.use[(size_t)i]) continue;
            rc_call.col[(size_t)i] = col++;
            if (!grouped[(size_t)i]) in_launch = false;
        }
    }
    if (in_launch) {
        const bool tail = !due.empty() && due.back() == nsteps;
        RC(ens_rec_stage(e, mem_b + (tail ? r.tab_b : 0)));
        rc_call.due0 = due.empty() ? nsteps : due[0];   // (nsteps: nothing due inside the launch)
        rc_call.slot0 = (double *)r.d_series + (size_t)r.records * (size_t)r.nobs * (size_t)r.n;
        note(ens_step_run(e, tau, nsteps, check_every, &rc_call));
        // the last step's record: no barrier behind it in the launch, so a gather behind the launch, from the
        // tables after the host's role swap (the six state fields are current in an open sequence: no tail)
        if (tail) note(ens_rec_gather(e, in, r.records + (int32_t)due.size() - 1, mem_b));
        r.in_launch += (int64_t)due.size() - (tail ? 1 : 0);
    } else {
        // chunked: up to each due step a plain call, then a gather, all on the stream.
        // A stretch is split further where check_every > 1 would lose its phase: the checks stay at the
        // steps s of THIS call with s % check_every == 0
        RC(ens_rec_stage(e, mem_b + due.size() * r.tab_b));
        int32_t pos = 0;
        for (size_t k = 0; k <= due.size() && pos < nsteps; ++k) {
            const int32_t upto = k < due.size() ? due[k] : nsteps;
            while (pos < upto) {
                int32_t len = upto - pos, ce = check_every;
                if (check_every > 1 && pos % check_every) {
                    const int32_t to_check = check_every - pos % check_every;
                    len = std::min(len, to_check);
                    ce = len == to_check ? len : 0;
                }
                note(ens_step_run(e, tau, len, ce, nullptr));
                pos += len;
            }
            if (k == due.size()) break;
            // (the six state fields are current after any call, its tail pending or not -- the next call starts
            // from them -- so the sequences stay open and the next call may be one launch; only steps that pair
            // launches deferred are still to run: they run now, as the tail does)
            int rt = OCN_OK;
            for (ocn_ctx *c : in)
                if (c->open && c->deferred)
                    if (const int rq = guarded(c, "ocn_ens_step_record", [&] { return complete_open(c); }); rq && !rt) rt = rq;
            note(rt);
            note(ens_rec_gather(e, in, r.records + (int32_t)k, mem_b + k * r.tab_b));
        }
    }
    HIPCHK(hipEventRecord(r.ev[r.slot], e->stream));
    r.ev_set[r.slot] = true;
    r.steps += nsteps;
    r.records += (int32_t)due.size();
    return first;
}

// ------------------------------------------------------------------ observations at their own times (ocn_sw.h)
// What ocn_ens_record_sample and ocn_ens_assimilate_rec check alike.  ens_rec_members: the members of the call
// (`use`, or the recorder's) among the recorder's, each one's column of the series in `col`.  ens_rec_obs: each
// observation's row, record and weight against the records taken, resolved into its series offset; nothing is
// read beyond a bad entry.  `who` opens the message.
static int ens_rec_members(const ocn_ens *e, const std::string &who, const uint8_t *use, std::vector<ocn_ctx *> &in,
                           std::vector<int> &col)
{
    const ocn_ens::Recorder &r = e->rec;
    int held = 0;
    for (size_t i = 0; i < e->m.size(); ++i) {
        if (use && use[i] && !r.use[i]) return set_error(OCN_ERR_ARG, who + ": a member in use that the recorder does not hold");
        if (r.use[i] && (!use || use[i])) { in.push_back(e->m[i]); col.push_back(held); }
        held += r.use[i] ? 1 : 0;
    }
    return OCN_OK;
}

static int ens_rec_obs(const ocn_ens *e, const std::string &who, int32_t nobs, const int32_t *row, const int32_t *rec,
                       const double *wt, std::vector<EnsRecObs> &robs)
{
    const ocn_ens::Recorder &r = e->rec;
    if (r.records < 1) return set_error(OCN_ERR_ARG, who + ": no record taken yet");
    robs.resize((size_t)nobs);
    for (int32_t j = 0; j < nobs; ++j) {
        if (row[j] < 0 || row[j] >= r.nobs) return set_error(OCN_ERR_ARG, who + ": a row outside the recorder's operator");
        if (rec[j] < 0 || rec[j] >= r.records) return set_error(OCN_ERR_ARG, who + ": a record outside the records taken");
        if (!std::isfinite(wt[j]) || !(wt[j] >= 0.0) || !(wt[j] < 1.0))
            return set_error(OCN_ERR_ARG, who + ": a weight that is not finite and in [0, 1)");
        if (wt[j] != 0.0 && rec[j] + 1 >= r.records) return set_error(OCN_ERR_ARG, who + ": a nonzero weight at the last record");
        robs[(size_t)j] = EnsRecObs{((long)rec[j] * (long)r.nobs + (long)row[j]) * (long)r.n, wt[j]};
    }
    return OCN_OK;
}

// ocn_ens_sample_h with the series in the members' place, in ocn_ens_sample's buffers: no member is read
int ocn_ens_record_sample(ocn_ens *e, const uint8_t *use, int32_t nobs, const int32_t *row, const int32_t *rec,
                          const double *wt, double *host)
{
    if (!e || !row || !rec || !wt || !host) return set_error(OCN_ERR_ARG, "ens_record_sample: null argument");
    const ocn_ens::Recorder &r = e->rec;
    if (!r.active) return set_error(OCN_ERR_STATE, "ens_record_sample: no recorder (ocn_ens_record_begin)");
    if (nobs < 1 || nobs > 65536) return set_error(OCN_ERR_ARG, "ens_record_sample: 1..65536 observations");
    std::vector<ocn_ctx *> in;
    std::vector<int> col;
    RC(ens_rec_members(e, "ens_record_sample", use, in, col));
    if (in.size() < 2) return set_error(OCN_ERR_ARG, "ens_record_sample: fewer than two members in use");
    std::vector<EnsRecObs> robs;
    RC(ens_rec_obs(e, "ens_record_sample", nobs, row, rec, wt, robs));
    HIPCHK(hipSetDevice(e->device));
    // one layout on both sides: the observations' table, the columns (up), the results (down)
    const size_t n = in.size(), no = (size_t)nobs, obs_b = no * sizeof(EnsRecObs), col_b = (n * sizeof(int) + 7) / 8 * 8,
                 up_b = obs_b + col_b, res_b = no * n * sizeof(double);
    if (e->samp_bytes < up_b + res_b) {   // (a synchronous entry: nothing in flight reads the old ones)
        if (e->d_samp) (void)hipFree(e->d_samp);
        if (e->h_samp) (void)hipHostFree(e->h_samp);
        e->d_samp = e->h_samp = nullptr;
        e->samp_bytes = 0;
        HIPCHK(hipMalloc(&e->d_samp, up_b + res_b));
        HIPCHK(hipHostMalloc(&e->h_samp, up_b + res_b, hipHostMallocDefault));
        e->samp_bytes = up_b + res_b;
    }
    char *d = (char *)e->d_samp, *hp = (char *)e->h_samp;
    memcpy(hp, robs.data(), obs_b);
    memcpy(hp + obs_b, col.data(), n * sizeof(int));
    HIPCHK(hipMemcpyAsync(d, hp, up_b, hipMemcpyHostToDevice, e->stream));
    const EnsRecSrc rs{(const double *)r.d_series, (const EnsRecObs *)d, (const int *)(d + obs_b), (long)r.nobs * (long)r.n};
    RC(launch_ens_record_sample(rs, (int)n, nobs, (double *)(d + up_b), e->stream));
    HIPCHK(hipMemcpyAsync(hp + up_b, d + up_b, res_b, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    memcpy(host, hp + up_b, res_b);
    return OCN_OK;
}

int ocn_ens_assimilate_rec(ocn_ens *e, const int32_t *field_ids, int32_t nfields, const uint8_t *use, int32_t nobs,
                           const int32_t *io, const int32_t *jo, const int32_t *row, const int32_t *rec, const double *wt,
                           const double *value, const double *variance, const double *taper, int32_t ntaper)
{
    if (!e || !field_ids || !io || !jo || !row || !rec || !wt || !value || !variance || !taper)
        return set_error(OCN_ERR_ARG, "ens_assimilate_rec: null argument");
    if (!e->rec.active) return set_error(OCN_ERR_STATE, "ens_assimilate_rec: no recorder (ocn_ens_record_begin)");
    std::vector<ocn_ctx *> in;
    std::vector<int> col;
    RC(ens_rec_members(e, "ens_assimilate_rec", use, in, col));
    RC(ens_lu_check(e, "ens_assimilate_rec", field_ids, nfields, in, nobs, io, jo, taper, ntaper));
    RC(ens_as_check("ens_assimilate_rec", nobs, value, variance));
    std::vector<EnsRecObs> robs;
    RC(ens_rec_obs(e, "ens_assimilate_rec", nobs, row, rec, wt, robs));
    return ens_as_run(e, "ocn_ens_assimilate_rec", in, field_ids, nfields, nobs, io, jo, value, variance, taper, ntaper, {}, {}, {},
                      nullptr, {}, robs, col);
}

// bytes [at, at + bytes) of the last call's results into the pinned copy, with one wait
static int ens_as_down(ocn_ens *e, size_t at, size_t bytes)
{
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync((char *)e->h_as + at, (const char *)e->d_as + at, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return OCN_OK;
}

int ocn_ens_assimilate_info(ocn_ens *e, ocn_ens_assim_info_t *out)
{
    if (!e || !out) return set_error(OCN_ERR_ARG, "ens_assimilate_info: null argument");
    const ocn_ens::AsLast &l = e->as_last;
    if (l.nobs < 1) return set_error(OCN_ERR_ARG, "ens_assimilate_info: no successful ocn_ens_assimilate yet");
    RC(ens_as_down(e, l.count_at, sizeof(long)));
    out->nobs = l.nobs;
    out->n = l.n;
    out->nonfinite = (int64_t) * (const long *)((const char *)e->h_as + l.count_at);
    return OCN_OK;
}

int ocn_ens_assimilate_result(ocn_ens *e, int32_t what, double *host)
{
    if (!e || !host) return set_error(OCN_ERR_ARG, "ens_assimilate_result: null argument");
    const ocn_ens::AsLast &l = e->as_last;
    if (l.nobs < 1) return set_error(OCN_ERR_ARG, "ens_assimilate_result: no successful ocn_ens_assimilate yet");
    const size_t no = (size_t)l.nobs, n = (size_t)l.n;
    if (what >= OCN_ENS_ASSIM_HX && what <= OCN_ENS_ASSIM_Z) {   // hx, y, z: one after another, each on a 256-B line
        const size_t rows_b = (no * l.row * sizeof(double) + 255) / 256 * 256, at = l.hx_at + (size_t)(what - OCN_ENS_ASSIM_HX) * rows_b;
        RC(ens_as_down(e, at, no * l.row * sizeof(double)));
        const double *src = (const double *)((const char *)e->h_as + at);
        for (size_t k = 0; k < no; ++k) memcpy(host + k * n, src + k * l.row, n * sizeof(double));
        return OCN_OK;
    }
    if (what >= OCN_ENS_ASSIM_INNOVATION && what <= OCN_ENS_ASSIM_POSTERIOR_SPREAD) {
        const size_t at = l.vec_at + (size_t)(what - OCN_ENS_ASSIM_INNOVATION) * no * 8;
        RC(ens_as_down(e, at, no * 8));
        memcpy(host, (const char *)e->h_as + at, no * 8);
        return OCN_OK;
    }
    if (what == OCN_ENS_ASSIM_ACCEPTED) {   // (a call made with the gate off accepted everything: nothing to bring down)
        if (!l.gated) { std::fill(host, host + no, 1.0); return OCN_OK; }
        RC(ens_as_down(e, l.accept_at, no * 8));
        memcpy(host, (const char *)e->h_as + l.accept_at, no * 8);
        return OCN_OK;
    }
    if (what == OCN_ENS_ASSIM_SPANS && l.timed) {   // (measurements: the two spans between the call's events, ms)
        HIPCHK(hipSetDevice(e->device));
        HIPCHK(hipEventSynchronize(e->ev_t[2]));
        float ms[2] = {0.f, 0.f};
        HIPCHK(hipEventElapsedTime(&ms[0], e->ev_t[0], e->ev_t[1]));
        HIPCHK(hipEventElapsedTime(&ms[1], e->ev_t[1], e->ev_t[2]));
        host[0] = (double)ms[0];
        host[1] = (double)ms[1];
        return OCN_OK;
    }
    return set_error(OCN_ERR_ARG, "ens_assimilate_result: what = OCN_ENS_ASSIM_*");
}

int ocn_ens_set_gate(ocn_ens *e, double gate2)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    if (gate2 == 0.0) { e->gate2 = 0.0; return OCN_OK; }   // (either sign: off)
    if (!(gate2 > 0.0)) return set_error(OCN_ERR_ARG, "ens_set_gate: a squared threshold > 0 (+inf allowed), or 0.0 for off");
    e->gate2 = gate2;
    return OCN_OK;
}

int ocn_ens_gate_info(ocn_ens *e, ocn_ens_gate_info_t *out)
{
    if (!e || !out) return set_error(OCN_ERR_ARG, "ens_gate_info: null argument");
    const ocn_ens::AsLast &l = e->as_last;
    int64_t rejected = 0;
    if (l.nobs >= 1 && l.gated) {
        RC(ens_as_down(e, l.accept_at, (size_t)l.nobs * 8));
        const double *acc = (const double *)((const char *)e->h_as + l.accept_at);
        for (int k = 0; k < l.nobs; ++k) rejected += acc[k] == 0.0;
    }
    out->gate2 = e->gate2;
    out->rejected = rejected;
    return OCN_OK;
}

}  // extern "C"
