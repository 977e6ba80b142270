// ocn_ens_modify.hip -- what rewrites an ensemble's members in place (ocn_sw.h): their recombination
// (ens_transform.hip), the saved spread and the inflation (ens_stats.hip, ens_inflate.hip) and the correlated
// random perturbations (ens_perturb.hip).  Each entry ends with field_uploaded() of what it rewrote.
#include "ocn_ens.h"

extern "C" {

// ------------------------------------------------------------------ recombination (ens_transform.hip)
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
    RC(e->w.reserve((size_t)ens_wt_stride(M) * ens_wt_cols(M) * sizeof(double), 1, true));   // (once: all the members')
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
    RC(e->w.await());
    const int ws = ens_wt_stride(n), wc = ens_wt_cols(n);
    double *hw = (double *)e->w.h;
    std::fill(hw, hw + (size_t)ws * wc, 0.0);
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) hw[ens_wt_index(n, a, b)] = w[(size_t)a * n + b];
    HIPCHK(hipMemcpyAsync(e->w.d, hw, (size_t)ws * wc * sizeof(double), hipMemcpyHostToDevice, e->stream));
    RC(e->w.sent(e->stream));
    int rc = OCN_OK;
    std::vector<double *> mem((size_t)n);
    for (int32_t f = 0; f < nfields && !rc; ++f)
        for (size_t k = 0; k < c0->blocks.size() && !rc; ++k) {
            for (int a = 0; a < n; ++a) mem[(size_t)a] = (double *)in[(size_t)a]->blocks[k].ptr[field_slot(field_ids[f])];
            double *stage = e->stage ? (double *)((char *)e->stage + 256 + ((uintptr_t)mem[0] & 255u)) : nullptr;
            rc = launch_ens_transform(&c0->blocks[k].g, mem.data(), n, (const double *)e->w.d, stage,
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
            q->buf[which][k] = (double *)ens_based_alloc(b, field_ids[f], field_bytes(b), &q->raw[which][k]);
            if (!q->buf[which][k]) return OCN_ERR_HIP;
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
        const size_t stride = (field_bytes(b) + 255) / 256 * 256;   // (every member's array based alike)
        pt.z[k] = (long long *)ens_based_alloc(b, OCN_SSH, stride * M, &pt.raw[k]);
        if (!pt.z[k]) return OCN_ERR_HIP;
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

}  // extern "C"
