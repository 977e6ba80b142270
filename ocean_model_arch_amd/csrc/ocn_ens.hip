// ocn_ens.hip -- ensembles (ocn_sw.h ocn_ens_*): many members of a small basin as contexts that share
// one compute stream, their multi-step launches issued one per group (sw_kernels.hip k_march_multi_b).
// The members' calls are planned by ocn_ctx.hip step_impl; ocn_ens_plan.h holds the grouping policy.
// The other host sources of the layer, each over ocn_ens.h (the ensemble itself and its buffers):
//   ocn_ens_diag.hip    the statistics over the members (ens_stats.hip) and their sampling (ens_transform.hip)
//   ocn_ens_modify.hip  their recombination (ens_transform.hip), the inflation of their spread
//                       (ens_inflate.hip) and their random perturbation (ens_perturb.hip)
//   ocn_ens_filter.hip  their localized observation update (ens_local.hip) and the serial filter's
//                       observation-space loop in front of it (ens_assim.hip)
//   ocn_ens_record.hip  the station recorder in their launches (sw_kernels.hip k_march_multi_rec)
//   ocn_ens_forcing.hip the moving-storm forcing of their momentum equations (ens_forcing.hip)
//   ocn_ens_run.hip     the one entry that steps with everything that is active (sw_kernels.hip k_march_multi_all)
//   ocn_ens_peak.hip    the peak map kept between their steps (ens_peak.hip, sw_kernels.hip k_march_multi_pk)
#include "ocn_ens.h"

namespace ocn {

// the members in use, in member order
std::vector<ocn_ctx *> ens_in_use(const ocn_ens *e, const uint8_t *use)
{
    std::vector<ocn_ctx *> in;
    for (size_t i = 0; i < e->m.size(); ++i)
        if (!use || use[i]) in.push_back(e->m[i]);
    return in;
}

// ocn_ens_plan's policy: ocn_ens_plan.h (pure host code, also built stand-alone)
static int ens_plan(const ocn_block *g, const int32_t *variant, int members, int64_t capacity,
                    std::vector<ocn_ens_group> &out)
{
    const char *err = nullptr;
    const int rc = ens_plan_groups(g, variant, members, capacity, out, &err);
    return rc ? set_error(rc, std::string("ensemble plan: ") + err) : OCN_OK;
}

// `bytes` of device memory based like block b's array of `field` -- 256 + (that array's address & 255) into an
// allocation of bytes + 512, which *raw keeps -- or null with the error set
void *ens_based_alloc(const LBlock &b, int32_t field, size_t bytes, void **raw)
{
    if (check_hip(hipMalloc(raw, bytes + 512), "hipMalloc")) return nullptr;
    return (char *)*raw + 256 + ((uintptr_t)b.ptr[field_slot(field)] & 255u);
}

int64_t ens_capacity(const ocn_ens *e)
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
int ens_groups(const ocn_ens *e, const std::vector<int32_t> &variant, int64_t capacity, std::vector<ocn_ens_group> &groups)
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

// the variant of a member whose call is planned as a multi-step launch (multi), or -1: the launch takes
// the library's fused path with the sw switches it needs; else the member's own launch
int32_t ens_variant(const ocn_ctx *c, double tau, bool check, bool multi)
{
    if (multi && c->fused && c->sw.full_free_surface == 1 && c->sw.trans_terms > 0 && c->sw.ksw_lat > 0)
        return onepass_multi_variant(c->kc_mode, tau, check);
    return -1;
}

void ens_probe(ocn_ens *e, const char *who, double tau, int32_t nsteps, int32_t check_every, const uint8_t *only,
               std::vector<int32_t> &variant, std::vector<char> &go)
{
    const size_t M = e->m.size();
    variant.assign(M, -1);
    go.assign(M, 0);
    for (size_t i = 0; i < M; ++i) {
        ocn_ctx *c = e->m[i];
        if (only && !only[i]) continue;
        bool multi = false, goes = false;
        if (!guarded(c, who, [&] { return step_probe(c, tau, nsteps, check_every, &multi, &goes); })) {
            variant[i] = ens_variant(c, tau, check_every == 1, multi);
            go[i] = goes ? 1 : 0;
        }
    }
}

std::vector<char> ens_grouped(const ocn_ens *e, const std::vector<ocn_ens_group> &groups)
{
    std::vector<char> grouped(e->m.size(), 0);
    for (const ocn_ens_group &q : groups)
        for (int j = 0; j < q.members; ++j) grouped[(size_t)q.member[j]] = 1;
    return grouped;
}

// ocn_ens_step; with `call` the same call with the recorder (call->rec), the forcing (call->frc) and / or the peak
// update (call->peak) in its launches
int ens_step_run(ocn_ens *e, double tau, int32_t nsteps, int32_t check_every, const EnsCall *call)
{
    const EnsRecCall *const rec = call ? call->rec : nullptr;
    const EnsFrcCall *const frc = call ? call->frc : nullptr;
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
        note(guarded(c, "ocn_ens_step", [&] { return step_entry(c, tau, nsteps, check_every, true); }));
        variant[(size_t)i] = ens_variant(c, tau, c->ens_k.check, c->ens_pending);
    }
    HIPCHK(hipSetDevice(e->device));
    e->last.capacity = call ? call->capacity : ens_capacity(e);
    std::vector<ocn_ens_group> groups;
    note(ens_groups(e, variant, e->last.capacity, groups));
    std::vector<char> done((size_t)M, 0);
    if (frc) {
        // every forced member must be in a launch, as ocn_ens_step_forced's probe found it: one that planned
        // otherwise has run its steps already, all under one forcing -- an error, never a silent result
        const std::vector<char> grouped = ens_grouped(e, groups);
        for (int i = 0; i < M; ++i)
            if (e->frc.forced[(size_t)i] && !grouped[(size_t)i])
                note(set_error(OCN_ERR_STATE, "ens_step_forced: member " + std::to_string(i) + " planned its call otherwise than its probe"));
        RC(ens_frc_write(e, frc->t0));   // (behind the planning, into the arrays step 0 reads)
    }
    const EnsPeakCall *const peak = call ? call->peak : nullptr;
    EnsPeakMember *pk_h = nullptr, *pk_d = nullptr;   // (the call's part of the peak stage: one entry per member)
    if (peak) {
        // every tracked member must be in a launch, as the entry's probe found it: one that planned otherwise has
        // run its steps already with no update between them -- an error, never a silent result
        const std::vector<char> grouped = ens_grouped(e, groups);
        for (int i = 0; i < M; ++i)
            if (e->pk.use[(size_t)i] && !grouped[(size_t)i])
                note(set_error(OCN_ERR_STATE, "ens_step: tracked member " + std::to_string(i) + " planned its call otherwise than its probe"));
        RC(ens_peak_slot(e, (size_t)M * sizeof(EnsPeakMember), (void **)&pk_h, (void **)&pk_d));
    }
    if (rec && (frc || peak)) {
        // (ocn_ens_run) likewise every recorded member: one that planned otherwise has run its steps already with
        // no record between them
        const std::vector<char> grouped = ens_grouped(e, groups);
        for (int i = 0; i < M; ++i)
            if (rec->col[(size_t)i] >= 0 && !grouped[(size_t)i])
                note(set_error(OCN_ERR_STATE, "ens_run: recorded member " + std::to_string(i) + " planned its call otherwise than its probe"));
    }
    size_t rec_off = 0;   // (members of the recording launches so far: their EnsRecMember in the call's stage)
    size_t pk_off = 0;    // (likewise the launches with the peak update and their EnsPeakMember)
    if (!groups.empty()) {
        const int sl = e->tab.slot;
        e->tab.slot ^= 1;
        RC(e->tab.await(sl));
        HIPCHK(hipMemsetAsync(e->d_bar, 0, (size_t)M * kMultiBarBytes, e->stream));
        const size_t eb = onepass_multi_b_entry_bytes();
        size_t off = 0;
        for (const ocn_ens_group &q : groups) {
            std::vector<Compact> cps((size_t)q.members);
            std::vector<EnsMember> ms((size_t)q.members);
            std::vector<ocn_ctx::Rec> recs((size_t)q.members);
            int rc = OCN_OK;
            bool forcing = false;   // (the group holds a forced member of a forced call)
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
                if (frc) ms[(size_t)j].index = q.member[j];
                if (frc && e->frc.forced[(size_t)q.member[j]]) {
                    const ocn_ens::Forcing::Second &sec = e->frc.second[(size_t)q.member[j]];
                    ms[(size_t)j].frc2[0] = sec.p[0];
                    ms[(size_t)j].frc2[1] = sec.p[1];
                    forcing = true;
                }
                if (!c->fused) c->hn_fresh = false;
                if (!rc) rc = timer_begin(c, OCN_TIMER_ONEPASS_MULTI, recs[(size_t)j]);
            }
            std::vector<int> col((size_t)q.members, -1);
            bool recording = false;
            for (int j = 0; j < q.members && rec && rec->due0 < nsteps; ++j)
                if ((col[(size_t)j] = rec->col[(size_t)q.member[j]]) >= 0) recording = true;
            const EnsLaunch L{ms.data(), q.members, q.variant, q.rows, e->m[(size_t)q.member[0]]->sw, tau, nsteps, e->tab.d,
                              (char *)e->tab.h[sl] + off, eb * (size_t)q.members, (long)e->last.capacity};
            EnsRecLaunch rl{};
            EnsFrcLaunch fl{};
            if (!rc && recording) {   // (the call's stage: ens_rec_stage; its other copy's turn at the next call)
                const ocn_ens::Recorder &r = e->rec;
                const char *d = (const char *)r.d_op;
                rl = EnsRecLaunch{col.data(), r.field.data(), (int)r.field.size(), (const int *)(d + r.start_at),
                                  (const EnsObsTerm *)(d + r.lterm_at), rec->slot0, rec->due0, r.every, r.nobs, r.n,
                                  (EnsRecMember *)r.stage.h[r.stage.slot] + rec_off, (EnsRecMember *)r.stage.d + rec_off};
                rec_off += (size_t)q.members;
            }
            if (forcing) fl = EnsFrcLaunch{(const EnsFrcMember *)e->frc.tab.d, e->frc.model, frc->t0};
            EnsPeakLaunch pl{};
            bool tracking = false;   // (the group holds a tracked member of a call with a peak active)
            for (int j = 0; j < q.members && peak; ++j)
                if (e->pk.use[(size_t)q.member[j]]) tracking = true;
            if (tracking) {   // (the launch adds the sources: the field in both parities' buffers)
                for (int j = 0; j < q.members; ++j) {
                    pk_h[pk_off + (size_t)j] = ens_peak_entry(e, 0, (size_t)q.member[j]);
                    pk_h[pk_off + (size_t)j].k0 = peak->k0;
                }
                pl = EnsPeakLaunch{e->pk.field, pk_h + pk_off, pk_d + pk_off};
                pk_off += (size_t)q.members;
            }
            if (!rc) rc = launch_onepass_multi_ens(L, recording ? &rl : nullptr, forcing ? &fl : nullptr, e->stream,
                                                   tracking ? &pl : nullptr);
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
        RC(e->tab.sent(sl, e->stream));
    }
    // the last step's forcing home: after an even number of steps it is in the second buffers; formed again into
    // the fields' own arrays behind the launches (the same operations: the same bits), where a later tail finds it
    if (frc && ((nsteps - 1) & 1)) note(ens_frc_write(e, frc->t0 + (double)(nsteps - 1) * tau));
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

}  // namespace ocn

extern "C" {

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
    e->tab.release();
    if (e->d_bar) (void)hipFree(e->d_bar);
    for (ocn_ens::Stats &q : e->stats)
        for (void *r : q.raw)
            if (r) (void)hipFree(r);
    if (e->d_ext) (void)hipFree(e->d_ext);
    if (e->h_ext) (void)hipHostFree(e->h_ext);
    e->w.release();
    if (e->stage) (void)hipFree(e->stage);
    e->samp.release();
    e->lu.release();
    e->as.release();
    for (hipEvent_t t : e->ev_t)
        if (t) (void)hipEventDestroy(t);
    for (ocn_ens::Inflate &q : e->inflate)
        for (std::vector<void *> &raw : q.raw)
            for (void *r : raw)
                if (r) (void)hipFree(r);
    for (void *r : e->perturb.raw)
        if (r) (void)hipFree(r);
    ens_rec_free(e);
    ens_peak_free(e);
    e->frc.tab.release();
    for (ocn_ens::Forcing::Second &q : e->frc.second)
        for (void *r : q.raw)
            if (r) (void)hipFree(r);
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
    if (!rc) rc = check_hip(hipMalloc((void **)&e->d_bar, (size_t)members * kMultiBarBytes), "hipMalloc");
    if (!rc) rc = e->tab.reserve((size_t)members * onepass_multi_b_entry_bytes(), 1);   // (once: it never grows)
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

int ocn_ens_step(ocn_ens *e, double tau, int32_t nsteps, int32_t check_every)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    if (e->pk.active && nsteps >= 1) {   // (ocn_ens_peak_*: the tracked members' peaks follow every step)
        if (e->pk.k + nsteps > INT32_MAX) return set_error(OCN_ERR_ARG, "ens_step: the peak's step count would pass INT32_MAX");
        HIPCHK(hipSetDevice(e->device));
        return ens_peak_step(e, tau, nsteps, check_every, nullptr);
    }
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
    case OCN_ENS_OPT_FORCING_IN_LAUNCH:
        if (value != 0 && value != 1) return set_error(OCN_ERR_ARG, "OCN_ENS_OPT_FORCING_IN_LAUNCH: 0 or 1");
        e->frc_in_launch = value != 0;
        return OCN_OK;
    case OCN_ENS_OPT_PEAK_IN_LAUNCH:
        if (value != 0 && value != 1) return set_error(OCN_ERR_ARG, "OCN_ENS_OPT_PEAK_IN_LAUNCH: 0 or 1");
        e->pk_in_launch = value != 0;
        return OCN_OK;
    case OCN_ENS_OPT_RUN_IN_LAUNCH:
        if (value != 0 && value != 1) return set_error(OCN_ERR_ARG, "OCN_ENS_OPT_RUN_IN_LAUNCH: 0 or 1");
        e->run_in_launch = value != 0;
        return OCN_OK;
    default: return set_error(OCN_ERR_ARG, "unknown ensemble option");
    }
}

}  // extern "C"
