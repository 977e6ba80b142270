// ocn_ens_peak.hip -- the peak map of an ensemble (ocn_sw.h ocn_ens_peak_*): per point and member the highest and
// lowest value a prognostic field has had after a step and that step's number, updated between the steps of the
// marching launches themselves (sw_kernels.hip k_march_multi_pk through ocn_ens.hip ens_step_run) or by a
// k_ens_peak launch behind each step (ens_peak.hip), and the products over the members' peaks.
#include "ocn_ens.h"

namespace ocn {

constexpr int kPeakAll = OCN_ENS_PEAK_MAX | OCN_ENS_PEAK_MIN;
constexpr size_t kPeakTables = 32;   // tables of every member of every block one pinned copy of the stage holds

static bool peak_field(int32_t f)
{
    return f == OCN_SSH || f == OCN_SSHP || f == OCN_UBRTR || f == OCN_UBRTRP || f == OCN_VBRTR || f == OCN_VBRTRP;
}

static void peak_release(ocn_ens::Peak &p)
{
    for (ocn_ens::Peak::Arr &a : p.arr)
        for (void *r : a.raw)
            if (r) (void)hipFree(r);   // (waits for the launches that use them)
    p.stage.release();
    p = ocn_ens::Peak{};
}

void ens_peak_free(ocn_ens *e) { peak_release(e->pk); }

// `need` bytes of the stage's pinned copy whose turn it is, and the device side's bytes of the same offset.  A full
// copy is left behind an event and the other one taken once the stream has read it: stream order keeps the users
// of the one device side apart
int ens_peak_slot(ocn_ens *e, size_t need, void **h, void **d)
{
    ocn_ens::Peak &p = e->pk;
    EnsStage2 &st = p.stage;
    need = (need + 255) / 256 * 256;
    if (need > st.bytes) return set_error(OCN_ERR_STATE, "ens_peak: a table larger than the stage");
    if (p.used + need > st.bytes) {
        RC(st.sent(st.slot, e->stream));
        st.slot ^= 1;
        RC(st.await(st.slot));
        p.used = 0;
    }
    *h = (char *)st.h[st.slot] + p.used;
    *d = (char *)st.d + p.used;
    p.used += need;
    return OCN_OK;
}

EnsPeakMember ens_peak_entry(const ocn_ens *e, size_t k, size_t i)
{
    const ocn_ens::Peak &p = e->pk;
    const size_t M = e->m.size();
    const ocn_block &g = e->m[i]->blocks[k].g;
    const ocn_ens::Peak::Arr &a = p.arr[k * M + i];
    EnsPeakMember q{};
    q.pmax = a.p[0]; q.smax = a.s[0];
    q.pmin = a.p[1]; q.smin = a.s[1];
    q.off = (long)(g.ny_start - g.bnd_y1) * g.pitch + (g.nx_start - g.bnd_x1);
    q.pitch = (long)g.pitch;
    q.w = g.nx_end - g.nx_start + 1;
    q.npts = q.w * (g.ny_end - g.ny_start + 1);
    q.tracked = p.use[i] && q.w > 0 && q.npts > 0 ? 1 : 0;
    return q;
}

// one k_ens_peak launch per local block over the tracked members, from the arrays as the field tables name them
// now: k = 0 the init, k >= 1 the update with step k.  The tracked members' deferred steps are the caller's.
static int peak_launch(ocn_ens *e, int32_t k)
{
    const ocn_ens::Peak &p = e->pk;
    const size_t M = e->m.size(), nblk = e->m[0]->blocks.size();
    void *h = nullptr, *d = nullptr;
    RC(ens_peak_slot(e, p.tab_b, &h, &d));
    EnsPeakMember *tab = (EnsPeakMember *)h;
    for (size_t kb = 0; kb < nblk; ++kb)
        for (size_t i = 0; i < M; ++i) {
            EnsPeakMember q = ens_peak_entry(e, kb, i);
            q.src[0] = q.src[1] = e->m[i]->blocks[kb].f<double>(p.field);
            tab[kb * M + i] = q;
        }
    HIPCHK(hipMemcpyAsync(d, h, nblk * M * sizeof(EnsPeakMember), hipMemcpyHostToDevice, e->stream));
    for (size_t kb = 0; kb < nblk; ++kb) {
        const LBlock &b = e->m[0]->blocks[kb];
        const int lead = (int)(((uintptr_t)b.ptr[field_slot(p.field)] & 255u) / 8u);
        RC(launch_ens_peak(&b.g, (const EnsPeakMember *)d + kb * M, (int)M, k, lead, e->stream));
    }
    return OCN_OK;
}

int ens_peak_launch(ocn_ens *e, int32_t k) { return peak_launch(e, k); }

// the tracked members' steps that pair launches deferred, run now as a call's tail runs them (the six state
// fields are current after any call otherwise: no other tail is formed, the sequences stay open)
static int peak_deferred(ocn_ens *e, const char *who)
{
    int first = OCN_OK;
    for (size_t i = 0; i < e->m.size(); ++i) {
        ocn_ctx *c = e->m[i];
        if (e->pk.use[i] && c->open && c->deferred)
            if (const int rc = guarded(c, who, [&] { return complete_open(c); }); rc && !first) first = rc;
    }
    return first;
}

int ens_peak_step(ocn_ens *e, double tau, int32_t nsteps, int32_t check_every, const EnsFrcCall *frc)
{
    ocn_ens::Peak &p = e->pk;
    const char *const who = frc ? "ocn_ens_step_forced" : "ocn_ens_step";
    const int M = (int)e->m.size();
    int first = OCN_OK;
    auto note = [&](int rc) { if (rc && !first) first = rc; };
    std::vector<int32_t> variant;
    std::vector<char> go;

    // In the launch only if every tracked member would go in a launch with the update in it -- known before any
    // step of the call runs, as ocn_ens_step_record decides it: each member says whether it would plan ONE
    // multi-step launch (step_probe), the planner whether it lands in a group under the capacity of those
    // kernels; a forced call keeps its own conditions (ocn_ens_step_forced).  The call itself then plans the same way.
    const EnsPeakCall pk_call{(int32_t)p.k};
    int64_t cap = std::min<int64_t>(ens_capacity(e), onepass_multi_pk_capacity());
    if (frc) cap = std::min<int64_t>(cap, onepass_multi_frc_capacity());
    const EnsCall call{cap, nullptr, frc, &pk_call};
    bool in_launch = e->pk_in_launch && (!frc || e->frc_in_launch) && nsteps >= 2 && e->m[0]->blocks.size() == 1;
    if (in_launch) {
        ens_probe(e, who, tau, nsteps, check_every, nullptr, variant, go);
        std::vector<ocn_ens_group> groups;
        if (ens_groups(e, variant, call.capacity, groups)) in_launch = false;
        const std::vector<char> grouped = ens_grouped(e, groups);
        for (int i = 0; i < M; ++i) {
            if (p.use[(size_t)i] && !grouped[(size_t)i]) in_launch = false;
            if (frc && e->frc.forced[(size_t)i] && !(grouped[(size_t)i] && go[(size_t)i])) in_launch = false;
        }
    }
    if (in_launch) {
        if (frc) RC(ens_frc_second(e));
        note(ens_step_run(e, tau, nsteps, check_every, &call));
        // the last step's update: no barrier behind it in the launch, so a launch behind the groups, from the
        // tables after the host's role swap (the six state fields are current in an open sequence: no tail)
        p.k += nsteps;
        note(peak_launch(e, (int32_t)p.k));
        p.in_launch += nsteps - 1;
        if (frc) { e->frc.in_launch = 1; e->frc.steps += nsteps; }
        return first;
    }
    // chunked: each step a 1-step call behind the forcing of its own time (a forced call), then the update, all on
    // the stream; the checks stay at the steps of THIS call that check_every divides
    for (int32_t s = 0; s < nsteps; ++s) {
        const int32_t ce = check_every > 0 && (s + 1) % check_every == 0 ? 1 : 0;
        if (frc) {
            ens_probe(e, who, tau, 1, ce, e->frc.forced.data(), variant, go);
            RC(ens_frc_apply(e, frc->t0 + (double)s * tau, who, &go));
        }
        note(ens_step_run(e, tau, 1, ce, nullptr));
        if (frc) ++e->frc.steps;
        note(peak_deferred(e, who));
        ++p.k;
        RC(peak_launch(e, (int32_t)p.k));
    }
    return first;
}

// what the products check alike: `which` one tracked extreme, block k, the members in use (null: the tracked ones)
// among the tracked ones -- their P arrays of that extreme on block k in member order
static int peak_sources(const ocn_ens *e, const std::string &who, int32_t k, int32_t which, const uint8_t *use,
                        std::vector<const double *> &src)
{
    const ocn_ens::Peak &p = e->pk;
    const size_t M = e->m.size();
    if (k < 0 || k >= (int32_t)e->m[0]->blocks.size()) return set_error(OCN_ERR_ARG, who + ": bad block index");
    if ((which != OCN_ENS_PEAK_MAX && which != OCN_ENS_PEAK_MIN) || !(p.what & which))
        return set_error(OCN_ERR_ARG, who + ": which is not one extreme that is tracked");
    const int x = which == OCN_ENS_PEAK_MAX ? 0 : 1;
    for (size_t i = 0; i < M; ++i) {
        if (use && use[i] && !p.use[i]) return set_error(OCN_ERR_ARG, who + ": a member in use that is not tracked");
        if (p.use[i] && (!use || use[i])) src.push_back(p.arr[(size_t)k * M + i].p[x]);
    }
    if (src.empty()) return set_error(OCN_ERR_ARG, who + ": no member in use");
    return OCN_OK;
}

}  // namespace ocn

extern "C" {

int ocn_ens_peak_begin(ocn_ens *e, const uint8_t *use, int32_t field_id, int32_t what)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    if (!peak_field(field_id))
        return set_error(OCN_ERR_ARG, "ens_peak_begin: the field is not one of ssh, sshp, ubrtr, ubrtrp, vbrtr, vbrtrp");
    if (what == 0 || (what & ~kPeakAll)) return set_error(OCN_ERR_ARG, "ens_peak_begin: what = OCN_ENS_PEAK_* bits");
    const size_t M = e->m.size(), nblk = e->m[0]->blocks.size();
    int tracked = 0;
    for (size_t i = 0; i < M; ++i) tracked += (!use || use[i]) ? 1 : 0;
    if (!tracked) return set_error(OCN_ERR_ARG, "ens_peak_begin: no member in use");
    for (const ocn_ctx *c : e->m)
        if (!c->initialized) return set_error(OCN_ERR_STATE, "ocn_ctx_init_state not called");
    HIPCHK(hipSetDevice(e->device));
    // the new peak whole before the earlier one goes (a failed allocation keeps that one)
    ocn_ens::Peak p;
    p.field = field_id; p.what = what; p.tracked = tracked;
    p.use.assign(M, 0);
    for (size_t i = 0; i < M; ++i) p.use[i] = (!use || use[i]) ? 1 : 0;
    p.arr.resize(nblk * M);
    p.tab_b = (nblk * M * sizeof(EnsPeakMember) + 255) / 256 * 256;
    int rc = p.stage.reserve(kPeakTables * p.tab_b, 1);
    for (size_t k = 0; k < nblk && !rc; ++k)
        for (size_t i = 0; i < M && !rc; ++i) {
            if (!p.use[i]) continue;
            const LBlock &b = e->m[i]->blocks[k];
            ocn_ens::Peak::Arr &a = p.arr[k * M + i];
            for (int x = 0; x < 2 && !rc; ++x) {
                if (!(what & (x ? OCN_ENS_PEAK_MIN : OCN_ENS_PEAK_MAX))) continue;
                a.p[x] = (double *)ens_based_alloc(b, field_id, field_bytes(b), &a.raw[2 * x]);
                if (a.p[x]) a.s[x] = (int32_t *)ens_based_alloc(b, field_id, field_bytes(b) / 2, &a.raw[2 * x + 1]);
                if (!a.p[x] || !a.s[x]) { rc = OCN_ERR_HIP; break; }
                // (+0.0 / 0 everywhere; the init below then writes the interior)
                rc = check_hip(hipMemsetAsync(a.p[x], 0, field_bytes(b), e->stream), "hipMemsetAsync");
                if (!rc) rc = check_hip(hipMemsetAsync(a.s[x], 0, field_bytes(b) / 2, e->stream), "hipMemsetAsync");
            }
        }
    if (rc) { peak_release(p); return rc; }
    peak_release(e->pk);
    p.active = true;
    e->pk = std::move(p);
    int first = peak_deferred(e, "ocn_ens_peak_begin");
    if (const int rq = peak_launch(e, 0); rq && !first) first = rq;
    return first;
}

int ocn_ens_peak_end(ocn_ens *e)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    if (!e->pk.active) return set_error(OCN_ERR_STATE, "ens_peak_end: no peak (ocn_ens_peak_begin)");
    HIPCHK(hipSetDevice(e->device));
    ens_peak_free(e);
    return OCN_OK;
}

int ocn_ens_peak_info(ocn_ens *e, ocn_ens_peak_info_t *out)
{
    if (!e || !out) return set_error(OCN_ERR_ARG, "ens_peak_info: null argument");
    const ocn_ens::Peak &p = e->pk;
    if (!p.active) return set_error(OCN_ERR_STATE, "ens_peak_info: no peak (ocn_ens_peak_begin)");
    *out = ocn_ens_peak_info_t{1, p.field, p.what, p.tracked, p.k, p.in_launch};
    return OCN_OK;
}

int ocn_ens_peak_download(ocn_ens *e, int32_t member, int32_t k, int32_t which, double *P_host, int32_t *S_host)
{
    if (!e || (!P_host && !S_host)) return set_error(OCN_ERR_ARG, "ens_peak_download: null argument");
    const ocn_ens::Peak &p = e->pk;
    if (!p.active) return set_error(OCN_ERR_STATE, "ens_peak_download: no peak (ocn_ens_peak_begin)");
    const size_t M = e->m.size();
    if (member < 0 || member >= (int32_t)M || !p.use[(size_t)member])
        return set_error(OCN_ERR_ARG, "ens_peak_download: a member outside the ensemble, or one that is not tracked");
    if (k < 0 || k >= (int32_t)e->m[0]->blocks.size()) return set_error(OCN_ERR_ARG, "ens_peak_download: bad block index");
    if ((which != OCN_ENS_PEAK_MAX && which != OCN_ENS_PEAK_MIN) || !(p.what & which))
        return set_error(OCN_ERR_ARG, "ens_peak_download: which is not one extreme that is tracked");
    HIPCHK(hipSetDevice(e->device));
    const ocn_ens::Peak::Arr &a = p.arr[(size_t)k * M + (size_t)member];
    const int x = which == OCN_ENS_PEAK_MAX ? 0 : 1;
    const ocn_block &g = e->m[0]->blocks[(size_t)k].g;
    const size_t w = (size_t)(g.bnd_x2 - g.bnd_x1 + 1), rows = (size_t)(g.bnd_y2 - g.bnd_y1 + 1);
    HIPCHK(hipStreamSynchronize(e->stream));
    if (P_host) HIPCHK(hipMemcpy2D(P_host, w * 8, a.p[x], (size_t)g.pitch * 8, w * 8, rows, hipMemcpyDeviceToHost));
    if (S_host) HIPCHK(hipMemcpy2D(S_host, w * 4, a.s[x], (size_t)g.pitch * 4, w * 4, rows, hipMemcpyDeviceToHost));
    return OCN_OK;
}

int ocn_ens_peak_stats(ocn_ens *e, int32_t k, int32_t which, const uint8_t *use, int32_t what)
{
    if (!e) return set_error(OCN_ERR_ARG, "null ensemble");
    const ocn_ens::Peak &p = e->pk;
    if (!p.active) return set_error(OCN_ERR_STATE, "ens_peak_stats: no peak (ocn_ens_peak_begin)");
    constexpr int kAll = OCN_ENS_STAT_MEAN | OCN_ENS_STAT_VAR | OCN_ENS_STAT_SPREAD | OCN_ENS_STAT_MIN | OCN_ENS_STAT_MAX;
    if (what == 0 || (what & ~kAll)) return set_error(OCN_ERR_ARG, "ens_peak_stats: what = OCN_ENS_STAT_* bits");
    std::vector<const double *> src;
    RC(peak_sources(e, "ens_peak_stats", k, which, use, src));
    const bool need_var = (what & (OCN_ENS_STAT_VAR | OCN_ENS_STAT_SPREAD)) != 0;
    if (need_var && src.size() < 2) return set_error(OCN_ERR_ARG, "ens_peak_stats: variance / spread of fewer than two members");
    HIPCHK(hipSetDevice(e->device));
    const LBlock &b0 = e->m[0]->blocks[(size_t)k];
    if (e->stats.empty()) e->stats.resize(e->m[0]->blocks.size());
    ocn_ens::Stats &st = e->stats[(size_t)k];
    // ocn_ens_stats' buffers (a failed allocation leaves the earlier results as they were)
    for (int i = 0; i < 5; ++i) {
        if (!(what & (1 << i)) || st.raw[i]) continue;
        st.p[i] = (double *)ens_based_alloc(b0, p.field, field_bytes(b0), &st.raw[i]);
        if (!st.p[i]) return OCN_ERR_HIP;
    }
    double *out[5];
    for (int i = 0; i < 5; ++i) out[i] = (what & (1 << i)) ? st.p[i] : nullptr;
    st.formed = 0;
    RC(launch_ens_stats(&b0.g, src.data(), (int)src.size(), need_var, out, e->stream));
    st.formed = what;
    return OCN_OK;
}

int ocn_ens_peak_exceed(ocn_ens *e, int32_t k, const uint8_t *use, double threshold, double *host)
{
    if (!e || !host) return set_error(OCN_ERR_ARG, "ens_peak_exceed: null argument");
    const ocn_ens::Peak &p = e->pk;
    if (!p.active) return set_error(OCN_ERR_STATE, "ens_peak_exceed: no peak (ocn_ens_peak_begin)");
    if (threshold != threshold) return set_error(OCN_ERR_ARG, "ens_peak_exceed: a threshold that is NaN");
    std::vector<const double *> src;
    RC(peak_sources(e, "ens_peak_exceed", k, OCN_ENS_PEAK_MAX, use, src));
    HIPCHK(hipSetDevice(e->device));
    const ocn_block &g = e->m[0]->blocks[(size_t)k].g;
    const size_t res_b = (size_t)(g.bnd_x2 - g.bnd_x1 + 1) * (size_t)(g.bnd_y2 - g.bnd_y1 + 1) * sizeof(double);
    RC(e->samp.reserve(res_b, 1));   // (a synchronous entry: nothing in flight reads the old ones)
    RC(launch_ens_exceed(&g, src.data(), (int)src.size(), threshold, (double *)e->samp.d, e->stream));
    HIPCHK(hipMemcpyAsync(e->samp.h, e->samp.d, res_b, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    memcpy(host, e->samp.h, res_b);
    return OCN_OK;
}

}  // extern "C"
