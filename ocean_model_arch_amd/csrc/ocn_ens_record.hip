// ocn_ens_record.hip -- the station recorder of an ensemble (ocn_sw.h ocn_ens_record_*, ocn_ens_step_record): its
// series, written by the marching launches themselves (sw_kernels.hip k_march_multi_rec through ocn_ens.hip
// ens_step_run) or by a gather behind each stretch of steps (ens_transform.hip k_ens_sample_h), and the series
// sampled at the observations' own times (ens_assim.hip k_ens_record_sample).
#include "ocn_ens.h"

namespace ocn {

// the recorder's buffers and events (ocn_ens_record_end, ocn_ens_record_begin over an earlier one, ocn_ens_destroy)
void ens_rec_free(ocn_ens *e)
{
    ocn_ens::Recorder &r = e->rec;
    if (r.d_series) (void)hipFree(r.d_series);   // (waits for the launches that use them)
    if (r.d_op) (void)hipFree(r.d_op);
    r.stage.release();
    r = ocn_ens::Recorder{};
}

// ------------------------------------------------------------------ observations at their own times (ocn_sw.h)
// What ocn_ens_record_sample and ocn_ens_assimilate_rec check alike.  ens_rec_members: the members of the call
// (`use`, or the recorder's) among the recorder's, each one's column of the series in `col`.  ens_rec_obs: each
// observation's row, record and weight against the records taken, resolved into its series offset; nothing is
// read beyond a bad entry.  `who` opens the message.
int ens_rec_members(const ocn_ens *e, const std::string &who, const uint8_t *use, std::vector<ocn_ctx *> &in,
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

int ens_rec_obs(const ocn_ens *e, const std::string &who, int32_t nobs, const int32_t *row, const int32_t *rec,
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

// The stage of one recording call: `need` bytes in the copy whose turn it is, read by the stream no more.
// Growing it waits for the device (rare: a call with more than 16 gathers after ocn_ens_record_begin).
int ens_rec_stage(ocn_ens *e, size_t need)
{
    EnsStage2 &st = e->rec.stage;
    RC(st.reserve(need, 65536));
    st.slot ^= 1;
    return st.await(st.slot);
}

// record `index` gathered from the members in use as their field tables name the arrays now: the pointer table
// at `at` of the call's stage up, then k_ens_sample_h into the record's slot.  No wait.
int ens_rec_gather(ocn_ens *e, const std::vector<ocn_ctx *> &in, int32_t index, size_t at)
{
    const ocn_ens::Recorder &r = e->rec;
    char *h = (char *)r.stage.h[r.stage.slot] + at, *dt = (char *)r.stage.d + at;
    ens_obs_table(in, r.field, (const double **)h);
    HIPCHK(hipMemcpyAsync(dt, h, r.tab_b, hipMemcpyHostToDevice, e->stream));
    const char *d = (const char *)r.d_op;
    const EnsObsOp op{(const double *const *)dt, (const int *)(d + r.start_at),
                      (const EnsObsTerm *)(d + r.term_at)};
    return launch_ens_sample_h(op, r.n, r.nobs, (double *)r.d_series + (size_t)index * (size_t)r.nobs * (size_t)r.n, e->stream);
}

}  // namespace ocn

extern "C" {

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
    int rc = check_hip(hipMalloc(&r.d_series, series_b), "hipMalloc");
    if (!rc) rc = check_hip(hipMalloc(&r.d_op, start_b + 2 * term_b), "hipMalloc");
    if (!rc) rc = r.stage.reserve((M * sizeof(EnsRecMember) + 255) / 256 * 256 + 16 * r.tab_b, 1);
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

int ocn_ens_step_record(ocn_ens *e, double tau, int32_t nsteps, int32_t check_every)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    ocn_ens::Recorder &r = e->rec;
    if (!r.active) return set_error(OCN_ERR_STATE, "ens_step_record: no recorder (ocn_ens_record_begin)");
    if (e->pk.active) return set_error(OCN_ERR_STATE, "ens_step_record: a peak is active (recording and peaks in one launch are not built)");
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
    // whether it would plan a multi-step launch (step_probe), the planner whether it lands in a group
    // under the recording capacity.  The call itself then plans the same way.
    EnsRecCall rc_call{std::vector<int>((size_t)M, -1), 0, nullptr};
    const EnsCall call{std::min<int64_t>(ens_capacity(e), onepass_multi_rec_capacity()), &rc_call, nullptr};
    bool in_launch = e->rec_in_launch && nsteps >= 2 && e->m[0]->blocks.size() == 1;
    if (in_launch) {
        std::vector<int32_t> variant;
        std::vector<char> go;
        ens_probe(e, "ocn_ens_step_record", tau, nsteps, check_every, nullptr, variant, go);
        std::vector<ocn_ens_group> groups;
        if (ens_groups(e, variant, call.capacity, groups)) in_launch = false;
        const std::vector<char> grouped = ens_grouped(e, groups);
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
        note(ens_step_run(e, tau, nsteps, check_every, &call));
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
    RC(r.stage.sent(r.stage.slot, e->stream));
    r.steps += nsteps;
    r.records += (int32_t)due.size();
    return first;
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
    RC(e->samp.reserve(up_b + res_b, 1));   // (a synchronous entry: nothing in flight reads the old ones)
    char *hp = (char *)e->samp.h;
    memcpy(hp, robs.data(), obs_b);
    memcpy(hp + obs_b, col.data(), n * sizeof(int));
    return ens_samp_run(e, up_b, res_b, host, [&](char *d) {
        const EnsRecSrc rs{(const double *)r.d_series, (const EnsRecObs *)d, (const int *)(d + obs_b), (long)r.nobs * (long)r.n};
        return launch_ens_record_sample(rs, (int)n, nobs, (double *)(d + up_b), e->stream);
    });
}

}  // extern "C"
