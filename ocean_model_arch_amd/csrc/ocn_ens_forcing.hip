// ocn_ens_forcing.hip -- the moving-storm forcing of an ensemble (ocn_sw.h ocn_ens_forcing_*, ocn_ens_step_forced):
// the members' storms, the table the launches read them from, and the stepping loop that gives every step the
// forcing of its own time (ens_forcing.hip k_ens_forcing ahead of each step's launches).
#include "ocn_ens.h"

namespace ocn {

// what ocn_ens_forcing_check and ocn_ens_forcing_set refuse; `who` opens the message
static int frc_check(const std::string &who, const ocn_ens_storm *storms, const uint8_t *use, int32_t n,
                     const ocn_ens_forcing_model *mo)
{
    if (!storms || !mo) return set_error(OCN_ERR_ARG, who + ": null argument");
    if (n < 1) return set_error(OCN_ERR_ARG, who + ": no storm");
    const double mv[7] = {mo->rho_air, mo->rho_water, mo->cd0, mo->cd1, mo->cd_max, mo->ub, mo->vb};
    for (double v : mv)
        if (!std::isfinite(v)) return set_error(OCN_ERR_ARG, who + ": a model value that is not finite");
    if (mo->rho_air < 0.0 || !(mo->rho_water > 0.0)) return set_error(OCN_ERR_ARG, who + ": rho_air < 0 or rho_water <= 0");
    if (mo->cd0 < 0.0 || mo->cd1 < 0.0 || mo->cd_max < 0.0) return set_error(OCN_ERR_ARG, who + ": a negative drag coefficient");
    for (int32_t i = 0; i < n; ++i) {
        if (use && !use[i]) continue;
        const ocn_ens_storm &s = storms[i];
        const std::string at = who + ": storm " + std::to_string(i);
        const double sv[10] = {s.x0, s.y0, s.cx, s.cy, s.radius, s.vmax, s.dp, s.cos_in, s.sin_in, s.turn};
        for (double v : sv)
            if (!std::isfinite(v)) return set_error(OCN_ERR_ARG, at + ": a value that is not finite");
        if (!(s.radius > 0.0)) return set_error(OCN_ERR_ARG, at + ": radius <= 0");
        if (s.vmax < 0.0 || s.dp < 0.0) return set_error(OCN_ERR_ARG, at + ": vmax or dp negative");
        if (s.turn != 1.0 && s.turn != -1.0) return set_error(OCN_ERR_ARG, at + ": turn is neither +1 nor -1");
        if (std::fabs(s.cos_in * s.cos_in + s.sin_in * s.sin_in - 1.0) > 1e-12)
            return set_error(OCN_ERR_ARG, at + ": cos_in^2 + sin_in^2 is not 1");
    }
    return OCN_OK;
}

// the launches' table as the members' field tables name the arrays now, sent where the device side differs
static int frc_table(ocn_ens *e)
{
    ocn_ens::Forcing &f = e->frc;
    const size_t M = e->m.size(), nblk = e->m[0]->blocks.size();
    std::vector<EnsFrcMember> now(nblk * M);
    std::memset((void *)now.data(), 0, now.size() * sizeof(EnsFrcMember));
    for (size_t k = 0; k < nblk; ++k)
        for (size_t i = 0; i < M; ++i) {
            const LBlock &b = e->m[i]->blocks[k];
            EnsFrcMember &q = now[k * M + i];
            q.s = f.storm[i];
            q.lcu = b.f<float>(OCN_LCU); q.lcv = b.f<float>(OCN_LCV);
            q.dx = b.f<float>(OCN_DX); q.dy = b.f<float>(OCN_DY);
            q.dxt = b.f<float>(OCN_DXT); q.dyt = b.f<float>(OCN_DYT);
            q.dxh = b.f<float>(OCN_DXH); q.dyh = b.f<float>(OCN_DYH);
            q.hr = b.f<double>(OCN_HHQ_REST);
            q.rx = b.f<double>(OCN_RHSX); q.ry = b.f<double>(OCN_RHSY);
            if (k == 0 && i < f.second.size()) { q.rx2 = f.second[i].p[0]; q.ry2 = f.second[i].p[1]; }
            q.forced = f.forced[i] ? 1 : 0;
        }
    const size_t bytes = now.size() * sizeof(EnsFrcMember);
    if (f.held.size() == now.size() && !std::memcmp((const void *)f.held.data(), (const void *)now.data(), bytes)) return OCN_OK;
    f.held.clear();
    RC(f.tab.reserve(bytes, 256));
    f.tab.slot ^= 1;
    const int sl = f.tab.slot;
    RC(f.tab.await(sl));
    std::memcpy(f.tab.h[sl], (const void *)now.data(), bytes);
    HIPCHK(hipMemcpyAsync(f.tab.d, f.tab.h[sl], bytes, hipMemcpyHostToDevice, e->stream));
    RC(f.tab.sent(sl, e->stream));
    f.held = std::move(now);
    return OCN_OK;
}

int ens_frc_write(ocn_ens *e, double t)
{
    ocn_ens::Forcing &f = e->frc;
    const size_t M = e->m.size();
    RC(frc_table(e));
    const ocn_ctx *c0 = e->m[0];
    int rc = OCN_OK;
    for (size_t k = 0; k < c0->blocks.size() && !rc; ++k) {
        const int lead = (int)(((uintptr_t)f.held[k * M].rx & 255u) / 8u);
        rc = launch_ens_forcing(&c0->blocks[k].g, (const EnsFrcMember *)f.tab.d + k * M, (int)M, f.model, t, lead, e->stream);
    }
    // (the forcing is no longer the +0.0 a known-constant verdict may have found: after ocn_ens_forcing_clear
    // the next call checks again)
    for (size_t i = 0; i < M; ++i)
        if (f.forced[i]) e->m[i]->fb_state = kFbUnchecked;
    ++f.applies;
    return rc;
}

// ocn_ens_forcing_apply behind its checks.  go (ocn_ens_step_forced's loop; null: no member): the forced members
// whose open sequence the next step goes on with -- their six state fields are current and the pending tail will
// be that step's, so the arrays are rewritten under them with no tail formed and nothing dropped
static int frc_apply(ocn_ens *e, double t, const char *who, const std::vector<char> *go = nullptr)
{
    ocn_ens::Forcing &f = e->frc;
    const size_t M = e->m.size();
    auto full = [&](size_t i) { return f.forced[i] && !(go && (*go)[i]); };
    // a pending tail re-runs the last step: it must find that step's forcing
    for (size_t i = 0; i < M; ++i)
        if (full(i)) RC(guarded(e->m[i], who, [&] { return complete_open(e->m[i]); }));
    const int rc = ens_frc_write(e, t);
    // what ocn_ctx_upload of the two fields leaves behind (also after a failed launch: the arrays may have changed)
    for (size_t i = 0; i < M; ++i)
        if (full(i)) { field_uploaded(e->m[i], OCN_RHSX); field_uploaded(e->m[i], OCN_RHSY); }
    return rc;
}

// the second RHSx / RHSy buffers of the forced members (one block), made where they are missing: zeroed, on the stream
static int frc_second(ocn_ens *e)
{
    ocn_ens::Forcing &f = e->frc;
    const size_t M = e->m.size();
    if (f.second.empty()) f.second.resize(M);
    for (size_t i = 0; i < M; ++i) {
        if (!f.forced[i]) continue;
        const LBlock &b = e->m[i]->blocks[0];
        const int ids[2] = {OCN_RHSX, OCN_RHSY};
        for (int a = 0; a < 2; ++a) {
            if (f.second[i].raw[a]) continue;
            f.second[i].p[a] = (double *)ens_based_alloc(b, ids[a], field_bytes(b), &f.second[i].raw[a]);
            if (!f.second[i].p[a]) return OCN_ERR_HIP;
            HIPCHK(hipMemsetAsync(f.second[i].p[a], 0, field_bytes(b), e->stream));
        }
    }
    return OCN_OK;
}

// (ocn_ens_peak.hip ens_peak_step: a forced call with a peak active runs the same two pieces)
int ens_frc_second(ocn_ens *e) { return frc_second(e); }
int ens_frc_apply(ocn_ens *e, double t, const char *who, const std::vector<char> *go) { return frc_apply(e, t, who, go); }

static int frc_ready(const ocn_ens *e, const std::string &who)
{
    if (!e->frc.attached) return set_error(OCN_ERR_STATE, who + ": no forced member (ocn_ens_forcing_set)");
    for (const ocn_ctx *c : e->m)
        if (!c->initialized) return set_error(OCN_ERR_STATE, "ocn_ctx_init_state not called");
    return OCN_OK;
}

int ens_frc_ready(const ocn_ens *e, const std::string &who) { return frc_ready(e, who); }

}  // namespace ocn

extern "C" {

int ocn_ens_forcing_check(const ocn_ens_storm *storms, int32_t n, const ocn_ens_forcing_model *model)
{
    return frc_check("ens_forcing_check", storms, nullptr, n, model);
}

int ocn_ens_forcing_set(ocn_ens *e, const uint8_t *use, const ocn_ens_storm *storms, const ocn_ens_forcing_model *model)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    const size_t M = e->m.size();
    RC(frc_check("ens_forcing_set", storms, use, (int32_t)M, model));
    ocn_ens::Forcing &f = e->frc;
    if (f.storm.empty()) { f.storm.assign(M, ocn_ens_storm{}); f.forced.assign(M, 0); }
    f.model = *model;
    f.attached = 0;
    for (size_t i = 0; i < M; ++i) {
        if (!use || use[i]) { f.storm[i] = storms[i]; f.forced[i] = 1; e->m[i]->forced = true; }
        f.attached += f.forced[i] ? 1 : 0;
    }
    return OCN_OK;
}

int ocn_ens_forcing_clear(ocn_ens *e)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    std::fill(e->frc.forced.begin(), e->frc.forced.end(), (uint8_t)0);
    e->frc.attached = 0;
    for (ocn_ctx *c : e->m) c->forced = false;
    return OCN_OK;
}

int ocn_ens_forcing_apply(ocn_ens *e, double t)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    if (!std::isfinite(t)) return set_error(OCN_ERR_ARG, "ens_forcing_apply: a time that is not finite");
    RC(frc_ready(e, "ens_forcing_apply"));
    HIPCHK(hipSetDevice(e->device));
    return frc_apply(e, t, "ocn_ens_forcing_apply");
}

int ocn_ens_step_forced(ocn_ens *e, double tau, int32_t nsteps, int32_t check_every, double t0)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    if (nsteps < 0) return set_error(OCN_ERR_ARG, "nsteps < 0");
    if (!std::isfinite(tau) || !std::isfinite(t0)) return set_error(OCN_ERR_ARG, "ens_step_forced: a tau or t0 that is not finite");
    if (e->pk.active && e->pk.k + nsteps > INT32_MAX)
        return set_error(OCN_ERR_ARG, "ens_step_forced: the peak's step count would pass INT32_MAX");
    RC(frc_ready(e, "ens_step_forced"));
    HIPCHK(hipSetDevice(e->device));
    ocn_ens::Forcing &f = e->frc;
    f.in_launch = 0;
    if (nsteps == 0) return OCN_OK;
    // (ocn_ens_peak_*: the tracked members' peaks follow every step; the routes' conditions are this entry's own
    // and the peak's)
    const EnsFrcCall pk_frc{t0};
    if (e->pk.active) return ens_peak_step(e, tau, nsteps, check_every, &pk_frc);
    const int M = (int)e->m.size();
    int first = OCN_OK;
    auto note = [&](int rc) { if (rc && !first) first = rc; };
    std::vector<int32_t> variant;
    std::vector<char> go;

    // In the launch only if every forced member would go in a forcing launch -- known before any step of the call
    // runs, as ocn_ens_step_record decides it: each member says whether it would plan ONE multi-step launch that
    // goes on with its open sequence (no tail to form, no deferred step that belongs to another time), the planner
    // whether it lands in a group under the forcing launch's capacity.  The call itself then plans the same way.
    const EnsFrcCall frc_call{t0};
    const EnsCall call{std::min<int64_t>(ens_capacity(e), onepass_multi_frc_capacity()), nullptr, &frc_call};
    bool in_launch = e->frc_in_launch && nsteps >= 2 && e->m[0]->blocks.size() == 1;
    if (in_launch) {
        ens_probe(e, "ocn_ens_step_forced", tau, nsteps, check_every, nullptr, variant, go);
        std::vector<ocn_ens_group> groups;
        if (ens_groups(e, variant, call.capacity, groups)) in_launch = false;
        const std::vector<char> grouped = ens_grouped(e, groups);
        for (int i = 0; i < M; ++i)
            if (f.forced[(size_t)i] && !(grouped[(size_t)i] && go[(size_t)i])) in_launch = false;
    }
    if (in_launch) {
        RC(frc_second(e));
        note(ens_step_run(e, tau, nsteps, check_every, &call));
        f.in_launch = 1;
        f.steps += nsteps;
        return first;
    }
    // chunked: each step behind the forcing of its own time, all on the stream; the checks stay at the steps of
    // THIS call that check_every divides
    for (int32_t s = 0; s < nsteps; ++s) {
        const double ts = t0 + (double)s * tau;
        const int32_t ce = check_every > 0 && (s + 1) % check_every == 0 ? 1 : 0;
        ens_probe(e, "ocn_ens_step_forced", tau, 1, ce, f.forced.data(), variant, go);
        RC(frc_apply(e, ts, "ocn_ens_step_forced", &go));
        note(ens_step_run(e, tau, 1, ce, nullptr));
        ++f.steps;
    }
    return first;
}

int ocn_ens_forcing_info(ocn_ens *e, ocn_ens_forcing_info_t *out)
{
    if (!e || !out) return set_error(OCN_ERR_ARG, "ens_forcing_info: null argument");
    *out = ocn_ens_forcing_info_t{e->frc.attached, e->frc.in_launch, e->frc.applies, e->frc.steps};
    return OCN_OK;
}

}  // extern "C"
