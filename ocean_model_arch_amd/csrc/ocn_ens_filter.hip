// ocn_ens_filter.hip -- assimilation into an ensemble's members (ocn_sw.h): the localized observation update
// (ens_local.hip) and the serial filter's observation-space loop in front of it (ens_assim.hip), fed by one field
// at points, by a sparse linear observation operator or by the recorder's series; its results and its gate.
// What these entries check and resolve alike is shared with the sampling and recording entries (ocn_ens.h).
#include "ocn_ens.h"

namespace ocn {

// ------------------------------------------------------------------ localized observation update (ens_local.hip)
// What ocn_ens_local_update and ocn_ens_assimilate check alike: the fields, the members in use, the counts,
// the observations within the basin, the taper.  `who` opens the message.
int ens_lu_check(const ocn_ens *e, const std::string &who, const int32_t *field_ids, int32_t nfields,
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

int ens_lu_reach(int32_t ntaper)   // the largest r with r * r < ntaper
{
    int reach = 0;
    while ((reach + 1) * (reach + 1) < ntaper) ++reach;
    return reach;
}

// each block's list: the observations whose box meets the block's array, in the caller's order, filled up
// to groups of kLuGroup.  Returns the entries of all lists.
size_t ens_lu_lists(const ocn_ctx *c0, int32_t nobs, const int32_t *io, const int32_t *jo, int reach,
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
void ens_lu_put_lists(const std::vector<std::vector<EnsLuObs>> &lists, char *h, size_t at, std::vector<size_t> &list_at)
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
int ens_lu_launches(const std::vector<ocn_ctx *> &in, const int32_t *field_ids, int32_t nfields,
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

// the local block a global point is read in -- the one whose interior holds it, else the first whose array
// does -- or -1
int ens_block_of(const ocn_ctx *c0, int32_t i, int32_t j)
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
int ens_as_check(const std::string &who, int32_t nobs, const double *value, const double *variance)
{
    for (int32_t k = 0; k < nobs; ++k) {
        if (!std::isfinite(value[k])) return set_error(OCN_ERR_ARG, who + ": a value that is not finite");
        if (!std::isfinite(variance[k]) || !(variance[k] > 0.0))
            return set_error(OCN_ERR_ARG, who + ": a variance that is not finite and positive");
    }
    return OCN_OK;
}

// a sparse linear observation operator validated and resolved for n members in use (ocn_ens.h EnsObsHost)
int ens_obs_resolve(const ocn_ctx *c0, const std::string &who, size_t n, int32_t nobs, const int32_t *start,
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
void ens_obs_table(const std::vector<ocn_ctx *> &in, const std::vector<int32_t> &fields, const double **tab)
{
    const size_t n = in.size(), nblk = in[0]->blocks.size();
    for (size_t f = 0; f < fields.size(); ++f)
        for (size_t b = 0; b < nblk; ++b)
            for (size_t m = 0; m < n; ++m)
                tab[(f * nblk + b) * n + m] = (const double *)in[m]->blocks[b].ptr[field_slot(fields[f])];
}

}  // namespace ocn

extern "C" {

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
    RC(e->lu.reserve(need, 65536, true));
    for (ocn_ctx *c : in) RC(guarded(c, "ocn_ens_local_update", [&] { return complete_open(c); }));
    // the tables up from pinned memory ahead of the launches
    RC(e->lu.await());
    char *h = (char *)e->lu.h, *d = (char *)e->lu.d;
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
    RC(e->lu.sent(e->stream));
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

// What ens_as_run's prologue reads, by kind.  `fields`: the fields of the pointer table.  direct: one field at the
// points (off, blk); op: the terms (start, term) of a sparse linear operator over the fields; recorded: no field
// at all but the recorder's series at robs[j] in the columns `col`.  What a kind does not use stays empty.
struct EnsAsSrc {
    enum Kind { direct, op, recorded } kind;
    std::vector<int32_t> fields;
    std::vector<long> off;
    std::vector<int> blk;
    const int32_t *start = nullptr;
    std::vector<EnsObsTerm> term;
    std::vector<EnsRecObs> robs;
    std::vector<int> col;
};

// ocn_ens_assimilate, ocn_ens_assimilate_h and ocn_ens_assimilate_rec behind their checks
static int ens_as_run(ocn_ens *e, const char *entry, const std::vector<ocn_ctx *> &in, const int32_t *field_ids, int32_t nfields,
                      int32_t nobs, const int32_t *io, const int32_t *jo, const double *value, const double *variance,
                      const double *taper, int32_t ntaper, const EnsAsSrc &from)
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
                 var_at = part(val_at, no * 8), off_at = part(var_at, no * 8), io_at = part(off_at, from.off.size() * sizeof(long)),
                 jo_at = part(io_at, no * 4), blk_at = part(jo_at, no * 4), start_at = part(blk_at, from.blk.size() * 4),
                 term_at = part(start_at, from.kind == EnsAsSrc::op ? (no + 1) * 4 : 0),
                 robs_at = part(term_at, from.term.size() * sizeof(EnsObsTerm)),
                 col_at = part(robs_at, from.robs.size() * sizeof(EnsRecObs)), tab_at = part(col_at, from.col.size() * sizeof(int)),
                 up_b = part(tab_at, from.fields.size() * nblk * n * sizeof(double *)), hx_at = up_b, y_at = part(hx_at, rows_b),
                 z_at = part(y_at, rows_b), vec_at = part(z_at, rows_b), count_at = part(vec_at, 3 * no * 8),
                 accept_at = part(count_at, sizeof(long)), need = part(accept_at, no * 8);
    const bool gated = e->gate2 != 0.0;
    // the buffers first (a failed allocation leaves the members as they were, and no earlier result)
    const bool timed = e->as_timing;
    for (int i = 0; i < 3 && timed; ++i)
        if (!e->ev_t[i]) HIPCHK(hipEventCreate(&e->ev_t[i]));
    if (e->as.bytes < need) e->as_last = ocn_ens::AsLast{};   // (growing: the earlier results go with the old buffer)
    RC(e->as.reserve(need, 65536, true));
    for (ocn_ctx *c : in) RC(guarded(c, entry, [&] { return complete_open(c); }));
    // the tables up from pinned memory in one copy, ahead of the launches; the members' arrays as the field
    // tables name them now
    RC(e->as.await());
    char *h = (char *)e->as.h, *d = (char *)e->as.d;
    memcpy(h + tap_at, taper, (size_t)ntaper * sizeof(double));
    std::vector<size_t> list_at;
    ens_lu_put_lists(lists, h, list_at0, list_at);
    memcpy(h + val_at, value, no * 8);
    memcpy(h + var_at, variance, no * 8);
    memcpy(h + io_at, io, no * 4);
    memcpy(h + jo_at, jo, no * 4);
    if (from.kind == EnsAsSrc::recorded) {
        memcpy(h + robs_at, from.robs.data(), from.robs.size() * sizeof(EnsRecObs));
        memcpy(h + col_at, from.col.data(), from.col.size() * sizeof(int));
    } else if (from.kind == EnsAsSrc::op) {
        memcpy(h + start_at, from.start, (no + 1) * 4);
        memcpy(h + term_at, from.term.data(), from.term.size() * sizeof(EnsObsTerm));
    } else {
        memcpy(h + off_at, from.off.data(), no * sizeof(long));
        memcpy(h + blk_at, from.blk.data(), no * 4);
    }
    ens_obs_table(in, from.fields, (const double **)(h + tab_at));
    e->as_last = ocn_ens::AsLast{};   // (the results of the call before are overwritten from here on)
    HIPCHK(hipMemcpyAsync(d, h, up_b, hipMemcpyHostToDevice, e->stream));
    RC(e->as.sent(e->stream));
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
    if (from.kind == EnsAsSrc::recorded) {
        const ocn_ens::Recorder &r = e->rec;
        const EnsRecSrc rs{(const double *)r.d_series, (const EnsRecObs *)(d + robs_at), (const int *)(d + col_at),
                           (long)r.nobs * (long)r.n};
        RC(gated ? launch_ens_obs_space_rg(a, rs, g, e->stream) : launch_ens_obs_space_r(a, rs, e->stream));
    } else if (from.kind == EnsAsSrc::op) {
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
    EnsAsSrc src{EnsAsSrc::direct, {obs_field}, std::vector<long>(no), std::vector<int>(no)};
    for (size_t k = 0; k < no; ++k) {
        const int at = ens_block_of(c0, io[k], jo[k]);
        if (at < 0) return set_error(OCN_ERR_ARG, "ens_assimilate: an observation in no local block's array");
        const ocn_block &g = c0->blocks[(size_t)at].g;
        src.blk[k] = at;
        src.off[k] = (long)(jo[k] - g.bnd_y1) * (long)g.pitch + (io[k] - g.bnd_x1);
    }
    return ens_as_run(e, "ocn_ens_assimilate", in, field_ids, nfields, nobs, io, jo, value, variance, taper, ntaper, src);
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
    const EnsAsSrc src{EnsAsSrc::op, std::move(h.fields), {}, {}, start, std::move(h.term)};
    return ens_as_run(e, "ocn_ens_assimilate_h", in, field_ids, nfields, nobs, io, jo, value, variance, taper, ntaper, src);
}

int ocn_ens_assimilate_rec(ocn_ens *e, const int32_t *field_ids, int32_t nfields, const uint8_t *use, int32_t nobs,
                           const int32_t *io, const int32_t *jo, const int32_t *row, const int32_t *rec, const double *wt,
                           const double *value, const double *variance, const double *taper, int32_t ntaper)
{
    if (!e || !field_ids || !io || !jo || !row || !rec || !wt || !value || !variance || !taper)
        return set_error(OCN_ERR_ARG, "ens_assimilate_rec: null argument");
    if (!e->rec.active) return set_error(OCN_ERR_STATE, "ens_assimilate_rec: no recorder (ocn_ens_record_begin)");
    std::vector<ocn_ctx *> in;
    EnsAsSrc src{EnsAsSrc::recorded};
    RC(ens_rec_members(e, "ens_assimilate_rec", use, in, src.col));
    RC(ens_lu_check(e, "ens_assimilate_rec", field_ids, nfields, in, nobs, io, jo, taper, ntaper));
    RC(ens_as_check("ens_assimilate_rec", nobs, value, variance));
    RC(ens_rec_obs(e, "ens_assimilate_rec", nobs, row, rec, wt, src.robs));
    return ens_as_run(e, "ocn_ens_assimilate_rec", in, field_ids, nfields, nobs, io, jo, value, variance, taper, ntaper, src);
}

// bytes [at, at + bytes) of the last call's results into the pinned copy, with one wait
static int ens_as_down(ocn_ens *e, size_t at, size_t bytes)
{
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync((char *)e->as.h + at, (const char *)e->as.d + at, bytes, hipMemcpyDeviceToHost, e->stream));
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
    out->nonfinite = (int64_t) * (const long *)((const char *)e->as.h + l.count_at);
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
        const double *src = (const double *)((const char *)e->as.h + at);
        for (size_t k = 0; k < no; ++k) memcpy(host + k * n, src + k * l.row, n * sizeof(double));
        return OCN_OK;
    }
    if (what >= OCN_ENS_ASSIM_INNOVATION && what <= OCN_ENS_ASSIM_POSTERIOR_SPREAD) {
        const size_t at = l.vec_at + (size_t)(what - OCN_ENS_ASSIM_INNOVATION) * no * 8;
        RC(ens_as_down(e, at, no * 8));
        memcpy(host, (const char *)e->as.h + at, no * 8);
        return OCN_OK;
    }
    if (what == OCN_ENS_ASSIM_ACCEPTED) {   // (a call made with the gate off accepted everything: nothing to bring down)
        if (!l.gated) { std::fill(host, host + no, 1.0); return OCN_OK; }
        RC(ens_as_down(e, l.accept_at, no * 8));
        memcpy(host, (const char *)e->as.h + l.accept_at, no * 8);
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
        const double *acc = (const double *)((const char *)e->as.h + l.accept_at);
        for (int k = 0; k < l.nobs; ++k) rejected += acc[k] == 0.0;
    }
    out->gate2 = e->gate2;
    out->rejected = rejected;
    return OCN_OK;
}

}  // extern "C"
