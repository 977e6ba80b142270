// ocn_ens_diag.hip -- what an ensemble's members are read for (ocn_sw.h): the statistics over them and the
// extrema per member (ens_stats.hip), their values at points and behind a sparse linear observation operator
// (ens_transform.hip k_ens_sample, k_ens_sample_h).  No entry here changes a member.
#include "ocn_ens.h"

extern "C" {

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
    const std::vector<ocn_ctx *> in = ens_in_use(e, use);
    const bool need_var = (what & (OCN_ENS_STAT_VAR | OCN_ENS_STAT_SPREAD)) != 0;
    if (in.empty()) return set_error(OCN_ERR_ARG, "ens_stats: no member in use");
    if (need_var && in.size() < 2) return set_error(OCN_ERR_ARG, "ens_stats: variance / spread of fewer than two members");
    HIPCHK(hipSetDevice(e->device));
    const LBlock &b0 = c0->blocks[(size_t)k];
    if (e->stats.empty()) e->stats.resize(c0->blocks.size());
    ocn_ens::Stats &st = e->stats[(size_t)k];
    // the buffers first (a failed allocation leaves the earlier results as they were)
    for (int i = 0; i < 5; ++i) {
        if (!(what & (1 << i)) || st.raw[i]) continue;
        st.p[i] = (double *)ens_based_alloc(b0, field_id, field_bytes(b0), &st.raw[i]);
        if (!st.p[i]) return OCN_ERR_HIP;
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

// ------------------------------------------------------------------ sampling (ens_transform.hip)
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
    RC(e->samp.reserve(up_b + res_b, 1));   // (a synchronous entry: nothing in flight reads the old ones)
    char *h = (char *)e->samp.h;
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
    return ens_samp_run(e, up_b, res_b, host, [&](char *d) {
        return launch_ens_sample(src.data(), nblk > 1 ? (const double *const *)(d + off_b + blk_b) : nullptr, (int)n,
                                 (const long *)d, (const int *)(d + off_b), npts, (double *)(d + up_b), e->stream);
    });
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
    RC(e->samp.reserve(up_b + res_b, 1));   // (a synchronous entry: nothing in flight reads the old ones)
    char *hp = (char *)e->samp.h;
    memcpy(hp, start, (no + 1) * 4);
    memcpy(hp + start_b, h.term.data(), term_b);
    // the members in use: their pending call tails formed, their arrays as the field tables name them now
    for (ocn_ctx *c : in) RC(guarded(c, "ocn_ens_sample_h", [&] { return complete_open(c); }));
    ens_obs_table(in, h.fields, (const double **)(hp + start_b + term_b));
    return ens_samp_run(e, up_b, res_b, host, [&](char *d) {
        const EnsObsOp op{(const double *const *)(d + start_b + term_b), (const int *)d, (const EnsObsTerm *)(d + start_b)};
        return launch_ens_sample_h(op, (int)n, nobs, (double *)(d + up_b), e->stream);
    });
}

}  // extern "C"
