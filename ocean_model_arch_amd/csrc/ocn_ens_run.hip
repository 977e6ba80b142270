// ocn_ens_run.hip -- the one entry that steps an ensemble with everything that is active (ocn_sw.h ocn_ens_run):
// the moving-storm forcing, the station recorder and the peak map in one marching launch (sw_kernels.hip
// k_march_multi_all through ocn_ens.hip ens_step_run), or chunked per step from the three entries' own pieces.
// Without a recorder, or with a recorder alone, the call is one of the three entries itself.
#include "ocn_ens.h"

extern "C" {

int ocn_ens_run(ocn_ens *e, double tau, int32_t nsteps, int32_t check_every, int32_t forced, double t0)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    if (nsteps < 0) return set_error(OCN_ERR_ARG, "nsteps < 0");
    if (!std::isfinite(tau) || (forced && !std::isfinite(t0))) return set_error(OCN_ERR_ARG, "ens_run: a tau or t0 that is not finite");
    ocn_ens::Recorder &r = e->rec;
    ocn_ens::Peak &p = e->pk;
    ocn_ens::Forcing &f = e->frc;
    // what an existing entry does is that entry's, byte for byte
    if (!r.active) return forced ? ocn_ens_step_forced(e, tau, nsteps, check_every, t0) : ocn_ens_step(e, tau, nsteps, check_every);
    if (!forced && !p.active) return ocn_ens_step_record(e, tau, nsteps, check_every);

    // a recorder together with a peak and / or a forced call: every refusal before anything is stepped or counted
    const char *const who = "ocn_ens_run";
    if (forced) {
        RC(ens_frc_ready(e, "ens_run"));
    } else {
        for (const ocn_ctx *c : e->m)
            if (!c->initialized) return set_error(OCN_ERR_STATE, "ocn_ctx_init_state not called");
    }
    if (p.active && p.k + nsteps > INT32_MAX) return set_error(OCN_ERR_ARG, "ens_run: the peak's step count would pass INT32_MAX");
    std::vector<int32_t> due;
    ens_record_due(r.steps, nsteps, r.every, due);
    if ((int64_t)r.records + (int64_t)due.size() > r.max_records)
        return set_error(OCN_ERR_ARG, "ens_run: the call's records would pass max_records");
    HIPCHK(hipSetDevice(e->device));
    if (forced) f.in_launch = 0;
    if (nsteps == 0) return OCN_OK;
    const int M = (int)e->m.size();
    const std::vector<ocn_ctx *> in = ens_in_use(e, r.use.data());
    int first = OCN_OK;
    auto note = [&](int rc) { if (rc && !first) first = rc; };
    const size_t mem_b = ((size_t)M * sizeof(EnsRecMember) + 255) / 256 * 256;
    std::vector<int32_t> variant;
    std::vector<char> go;

    // In the launch only if every member that is recorded, tracked or forced would go in a launch -- known before
    // any step of the call runs, as the three entries decide it: each member says whether it would plan ONE
    // multi-step launch (step_probe), the planner whether it lands in a group under the least of the capacities
    // involved; a forced member must also go on with its open sequence.  The call itself then plans the same way.
    EnsRecCall rc_call{std::vector<int>((size_t)M, -1), 0, nullptr};
    const EnsFrcCall frc_call{t0};
    const EnsPeakCall pk_call{(int32_t)p.k};
    int64_t cap = std::min<int64_t>(ens_capacity(e), onepass_multi_rec_capacity());
    if (p.active) cap = std::min<int64_t>(cap, onepass_multi_pk_capacity());
    if (forced) cap = std::min<int64_t>(cap, onepass_multi_frc_capacity());
    cap = std::min<int64_t>(cap, onepass_multi_all_capacity());
    const EnsCall call{cap, &rc_call, forced ? &frc_call : nullptr, p.active ? &pk_call : nullptr};
    bool in_launch = e->run_in_launch && e->rec_in_launch && (!p.active || e->pk_in_launch) && (!forced || e->frc_in_launch) &&
                     nsteps >= 2 && e->m[0]->blocks.size() == 1;
    if (in_launch) {
        ens_probe(e, who, tau, nsteps, check_every, nullptr, variant, go);
        std::vector<ocn_ens_group> groups;
        if (ens_groups(e, variant, call.capacity, groups)) in_launch = false;
        const std::vector<char> grouped = ens_grouped(e, groups);
        for (int i = 0, col = 0; i < M; ++i) {
            const bool is_forced = forced && f.forced[(size_t)i];
            if (r.use[(size_t)i]) rc_call.col[(size_t)i] = col++;
            if ((r.use[(size_t)i] || (p.active && p.use[(size_t)i]) || is_forced) && !grouped[(size_t)i]) in_launch = false;
            if (is_forced && !go[(size_t)i]) in_launch = false;
        }
    }
    if (in_launch) {
        if (forced) RC(ens_frc_second(e));
        const bool tail = !due.empty() && due.back() == nsteps;
        RC(ens_rec_stage(e, mem_b + (tail ? r.tab_b : 0)));
        rc_call.due0 = due.empty() ? nsteps : due[0];   // (nsteps: nothing due inside the launch)
        rc_call.slot0 = (double *)r.d_series + (size_t)r.records * (size_t)r.nobs * (size_t)r.n;
        note(ens_step_run(e, tau, nsteps, check_every, &call));   // (with the forcing's home-coming write behind the groups)
        // what has no barrier behind it in the launch: the last step's peak update, then its record, behind the
        // groups on the stream, from the tables after the host's role swap (the six state fields are current in an
        // open sequence: no tail)
        if (p.active) {
            p.k += nsteps;
            note(ens_peak_launch(e, (int32_t)p.k));
            p.in_launch += nsteps - 1;
        }
        if (tail) note(ens_rec_gather(e, in, r.records + (int32_t)due.size() - 1, mem_b));
        r.in_launch += (int64_t)due.size() - (tail ? 1 : 0);
        if (forced) { f.in_launch = 1; f.steps += nsteps; }
    } else {
        // chunked: per step the forcing of its own time (a forced call), the step as a 1-step call (the checks stay
        // at the steps of THIS call that check_every divides), the deferred steps of the members that are tracked
        // or recorded, the peak update, the record if the step is due -- all on the stream
        RC(ens_rec_stage(e, mem_b + due.size() * r.tab_b));
        size_t k = 0;
        for (int32_t s = 0; s < nsteps; ++s) {
            const int32_t ce = check_every > 0 && (s + 1) % check_every == 0 ? 1 : 0;
            if (forced) {
                ens_probe(e, who, tau, 1, ce, f.forced.data(), variant, go);
                note(ens_frc_apply(e, t0 + (double)s * tau, who, &go));
            }
            note(ens_step_run(e, tau, 1, ce, nullptr));
            if (forced) ++f.steps;
            for (int i = 0; i < M; ++i) {
                ocn_ctx *c = e->m[(size_t)i];
                if ((r.use[(size_t)i] || (p.active && p.use[(size_t)i])) && c->open && c->deferred)
                    note(guarded(c, who, [&] { return complete_open(c); }));
            }
            if (p.active) {
                ++p.k;
                note(ens_peak_launch(e, (int32_t)p.k));
            }
            if (k < due.size() && due[k] == s + 1) {
                note(ens_rec_gather(e, in, r.records + (int32_t)k, mem_b + k * r.tab_b));
                ++k;
            }
        }
    }
    RC(r.stage.sent(r.stage.slot, e->stream));
    r.steps += nsteps;
    r.records += (int32_t)due.size();
    return first;
}

}  // extern "C"
