// ctx_setup.hip -- what a model context (ocn_ctx.h) is made of before it steps: the decomposition
// into blocks, device storage, the initial state, the compact static tables (prepare_static).
//
// Reference counterparts (Andrcraft9/ocean_model_arch):
//   storage        core/data_types.f90:44-144, core/ocean.f90:14-48, core/grid.f90:23-90
//   decomposition  core/decomposition.f90:427-503 (uniform blocks), :614-669 (block -> rank),
//                  :672-760 (local numbering, _MPP_SORTED_BLOCKS_), :950-1062 (neighbour maps)
//   init           control/init_data.f90:29-125, kernel/service/grid_kernels.f90,
//                  kernel/service/grid_parameters.f90:80-181, kernel/shallow_water/vel_ssh.f90:15-38
#include "ocn_ctx.h"

namespace ocn {

// init_grid_data's bottom topography (control/init_data.f90:115-120): read_data2D_real4 fills the
// block's interior from the file (tools/io.f90:130-147; the file holds the (nx-4) x (ny-4) interior,
// Fortran order) and zeroes every point with |lu| < 0.5 (:158-171), the rest of the zero-initialised
// array stays 0, then copy_from_real4 promotes it (core/data_types.f90:638-652); the sync follows.
__global__ void k_topography(ocn_block g, double *h, const float *lu, const float *topo, int nxi)
{
    const int w = g.bnd_x2 - g.bnd_x1 + 1, rows = g.bnd_y2 - g.bnd_y1 + 1;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)w * rows) return;
    const int m = g.bnd_x1 + (int)(i % w), n = g.bnd_y1 + (int)(i / w);
    const long at = (long)(m - g.bnd_x1) + (long)(n - g.bnd_y1) * g.pitch;
    float v = 0.0f;
    if (m >= g.nx_start && m <= g.nx_end && n >= g.ny_start && n <= g.ny_end) v = topo[(long)(m - 3) + (long)(n - 3) * nxi];
    if (fabsf(lu[at]) < 0.5f) v = 0.0f;
    h[at] = (double)v;
}

__global__ void k_fill_r8(double *p, long n, double v)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ------------------------------------------------------------------ decomposition
// decomposition.f90:448-482: floor(real(remaining)/real(parts_left)) in default real(4)
static std::vector<int> uniform_sizes(int total, int parts, std::string &err)
{
    std::vector<int> s;
    int acc = 0;
    for (int i = 1; i <= parts; ++i) {
        int v = (i == parts) ? total - acc : (int)std::floor((float)(total - acc) / (float)(parts - i + 1));
        if (v <= 0) { err = "Error in decomposition to uniform blocks: size <= 0"; return {}; }
        s.push_back(v);
        acc += v;
    }
    return s;
}

// MPI_Dims_create(n, 2): balanced, non-increasing factors (mpp.f90:89).
static void dims_create(int n, int &d1, int &d2)
{
    d1 = n; d2 = 1;
    for (int f = (int)std::floor(std::sqrt((double)n)); f >= 1; --f)
        if (n % f == 0) { d1 = n / f; d2 = f; break; }
}

int decompose(ocn_ctx *c)
{
    const int nx = c->basin.nx, ny = c->basin.ny;
    std::string err;
    auto xs = uniform_sizes(nx - 4, c->bnx, err);
    auto ys = uniform_sizes(ny - 4, c->bny, err);
    if (!err.empty()) return set_error(OCN_ERR_ARG, err);
    int p1, p2;
    dims_create(c->dec.nranks, p1, p2);
    if (c->bnx % p1 || c->bny % p2)
        return set_error(OCN_ERR_ARG, "mod(bnx, p_size(1)) or mod(bny, p_size(2)) not equal 0 (decomposition.f90:628)");
    const int lbx = c->bnx / p1, lby = c->bny / p2;
    c->gblocks.assign((size_t)c->bnx * c->bny, GBlock{});
    int x0 = 0;
    for (int bm = 1; bm <= c->bnx; ++bm) {
        int y0 = 0;
        for (int bn = 1; bn <= c->bny; ++bn) {
            GBlock &g = c->gblocks[(size_t)(bm - 1) + (size_t)(bn - 1) * c->bnx];
            g.bm = bm; g.bn = bn;
            g.g.nx_start = 3 + x0; g.g.nx_end = g.g.nx_start + xs[bm - 1] - 1;
            g.g.ny_start = 3 + y0; g.g.ny_end = g.g.ny_start + ys[bn - 1] - 1;
            g.g.bnd_x1 = g.g.nx_start - 2; g.g.bnd_x2 = g.g.nx_end + 2;
            g.g.bnd_y1 = g.g.ny_start - 2; g.g.bnd_y2 = g.g.ny_end + 2;
            g.g.pitch = 0;
            double w = 0.0;
            for (int i = g.g.nx_start; i <= g.g.nx_end; ++i)
                for (int j = g.g.ny_start; j <= g.g.ny_end; ++j)
                    w += 1.0 - (double)c->mask[(size_t)(i - 1) + (size_t)(j - 1) * nx];
            g.weight = w;
            // create_uniform_decomposition: process coords (row-major cart), land blocks -> -1
            const int c1 = (bm - 1) / lbx, c2 = (bn - 1) / lby;
            g.rank = (w == 0.0) ? -1 : c1 * p2 + c2;
            g.k = -1;
            y0 += ys[bn - 1];
        }
        x0 += xs[bm - 1];
    }
    // local numbering per rank: _MPP_SORTED_BLOCKS_ = MINLOC over weight (column-major order)
    std::vector<int> next(c->dec.nranks, 0);
    std::vector<int> order(c->gblocks.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return c->gblocks[a].weight < c->gblocks[b].weight;
    });
    for (int gid : order) {
        GBlock &g = c->gblocks[gid];
        if (g.rank >= 0) g.k = next[g.rank]++;
    }
    // local blocks of this rank, k order
    std::vector<int> mine;
    for (int gid : order)
        if (c->gblocks[gid].rank == c->dec.rank) mine.push_back(gid);
    c->blocks.clear();
    for (int gid : mine) {
        const GBlock &g = c->gblocks[gid];
        LBlock lb;
        lb.g = g.g;
        lb.bm = g.bm; lb.bn = g.bn; lb.gid = gid;
        const int w = g.g.bnd_x2 - g.g.bnd_x1 + 1;
        // 512-B aligned rows for r8, with room for 2 * kXRing more columns (the extra halo rings of
        // one_step_x4 live in the row padding: column bnd_x1 - j is the previous row's tail)
        lb.g.pitch = (int64_t)((w + 2 * kXRing + 63) / 64 * 64);
        for (int d = 1; d <= 8; ++d) {
            const int m = g.bm + kDirDm[d], n = g.bn + kDirDn[d];
            if (m < 1 || m > c->bnx || n < 1 || n > c->bny) {
                lb.nbr_rank[d - 1] = -2; lb.nbr_k[d - 1] = -1; lb.nbr_gid[d - 1] = -1;
            } else {
                const int ng = (m - 1) + (n - 1) * c->bnx;
                lb.nbr_rank[d - 1] = c->gblocks[ng].rank;
                lb.nbr_k[d - 1] = c->gblocks[ng].k;
                lb.nbr_gid[d - 1] = c->gblocks[ng].rank >= 0 ? ng : -1;
            }
            if (lb.nbr_rank[d - 1] >= 0)   // own_class(m) * 3 + own_class(n) of direction d's halo points
                lb.own |= 1u << ((unsigned)(kDirDm[d] + 1) * 3u + (unsigned)(kDirDn[d] + 1));
        }
        c->blocks.push_back(lb);
    }
    return OCN_OK;
}

// ------------------------------------------------------------------ storage
// The state arrays of the one-pass step as groups of physical buffers that agree on the second
// halo ring (the reference never writes it; the pairs are coherent, the second buffers copies):
// the field's own buffer first.
static const int kStateIds[6] = {OCN_SSH, OCN_SSHP, OCN_UBRTR, OCN_UBRTRP, OCN_VBRTR, OCN_VBRTRP};
static void state_group(const LBlock &b, int g, void *out[2])
{
    const int id = kStateIds[g];
    out[0] = b.ptr[field_slot(id)];
    switch (id) {
    case OCN_SSH: out[1] = b.ptr[field_slot(OCN_SSHN)]; break;
    case OCN_UBRTR: out[1] = b.ptr[field_slot(OCN_UBRTRN)]; break;
    case OCN_VBRTR: out[1] = b.ptr[field_slot(OCN_VBRTRN)]; break;
    case OCN_SSHP: out[1] = b.sshp_alt; break;
    case OCN_UBRTRP: out[1] = b.up_alt; break;
    default: out[1] = b.vp_alt; break;
    }
}

// one_step_x2's per-block storage: the ext metric rows, the row table with them, the h_r copy, the
// save area of the state's second halo ring and the runs that save / restore it (pointers of the
// physical buffers: role independent)
static int allocate_x2(ocn_ctx *c, LBlock &b)
{
    const int w = b.g.bnd_x2 - b.g.bnd_x1 + 1, h = b.g.bnd_y2 - b.g.bnd_y1 + 1;
    const size_t nrow = row_table_size((unsigned)h);
    HIPCHK(hipMalloc(&b.ext, kExtRowFloats * sizeof(float)));
    c->allocs.push_back(b.ext);
    HIPCHK(hipMalloc(&b.rows_x, nrow * sizeof(float)));
    c->allocs.push_back(b.rows_x);
    {   // based like the real(8) fields (kXRing more rows each side): x4 pairs of the h_r-read variant
        // read it 4 rings deep
        char *d = nullptr;
        const size_t nb = sizeof(double) * (size_t)(b.g.pitch * (h + 2 * kXRing)) + 512;
        HIPCHK(hipMalloc(&d, nb));
        c->allocs.push_back(d);
        HIPCHK(hipMemsetAsync(d, 0, nb, c->stream));   // (rings no exchange fills: +0.0)
        b.hr_x = (double *)(d + 256) + (long)kXRing * b.g.pitch;
    }
    const long per = 2L * w + 2L * (h - 2);   // rows bnd_y1, bnd_y2; columns bnd_x1, bnd_x2 between them
    // the state's six groups, then two per tracer (ff1 / ff1n, ff1p / its second buffer: x4 pairs
    // exchange the tracers 2 deep)
    const int ntr = c->sw.use_tracers > 0 ? c->sw.tracer_num : 0, ngroups = 6 + 2 * ntr;
    HIPCHK(hipMalloc(&b.ring2, sizeof(double) * (size_t)(ngroups * per)));
    c->allocs.push_back(b.ring2);
    HIPCHK(hipMalloc(&b.bits_x4, (size_t)b.g.pitch * (h + 2 * kXRing)));
    c->allocs.push_back(b.bits_x4);
    HIPCHK(hipMalloc(&b.rows_x4, row_table_size((unsigned)(h + 2 * kXRing)) * sizeof(float)));
    c->allocs.push_back(b.rows_x4);
    if (ntr) {
        const long xr = (long)kXRing * b.g.pitch;
        for (double *&q : b.trs) {
            char *d = nullptr;
            HIPCHK(hipMalloc(&d, sizeof(double) * (size_t)(b.g.pitch * (h + 2 * kXRing)) + 512));
            c->allocs.push_back(d);
            q = (double *)(d + 256) + xr;
        }
    }
    std::vector<Seg> save, restore;
    const long p = (long)b.g.pitch;
    for (int g = 0; g < ngroups; ++g) {
        void *buf[2];
        if (g < 6) {
            state_group(b, g, buf);
        } else {
            const int t = 1 + (g - 6) / 2;
            buf[0] = b.ptr[field_slot((g - 6) % 2 ? OCN_FF1P(t) : OCN_FF1(t))];
            buf[1] = (g - 6) % 2 ? b.ffp_alt[(size_t)t - 1] : b.ptr[field_slot(OCN_FF1N(t))];
        }
        double *area = b.ring2 + g * per;
        // (offset in the array, stride, count, offset in the area)
        const long runs[4][4] = {{0, 1, w, 0}, {(long)(h - 1) * p, 1, w, w}, {p, p, h - 2, 2L * w},
                                 {p + w - 1, p, h - 2, 2L * w + h - 2}};
        for (const auto &r : runs) {
            if (r[2] <= 0) continue;
            save.push_back(Seg{(const double *)buf[0] + r[0], area + r[3], r[1], 1, (int)r[2]});
            for (void *q : buf) restore.push_back(Seg{area + r[3], (double *)q + r[0], 1, r[1], (int)r[2]});
        }
    }
    RC(make_seglist(c, save, b.save));
    RC(make_seglist(c, restore, b.restore));
    return OCN_OK;
}

int allocate(ocn_ctx *c)
{
    for (LBlock &b : c->blocks) {
        const long rows = b.g.bnd_y2 - b.g.bnd_y1 + 1;
        const long n = (long)b.g.pitch * rows;
        // every field padded to a 256-B multiple, based so that A(nx_start, :) rows are
        // 256-B aligned: base offset shifted by (nx_start - bnd_x1) = 2 elements.
        // OCN_FIELD_SKEW (bytes, multiple of 256): extra gap between consecutive fields.
        // real(8) fields: kXRing more rows above and below the array (one_step_x4's extra rings)
        const long xr = (long)kXRing * b.g.pitch * 8;
        const long r8b = ((n * 8 + 16 + 255) / 256) * 256 + 256 + OCN_FIELD_SKEW + 2 * xr;
        const long r4b = ((n * 4 + 8 + 255) / 256) * 256 + 256 + OCN_FIELD_SKEW;
        const int nr8 = num_r8(c), ntr = c->sw.use_tracers > 0 ? c->sw.tracer_num : 0;
        // + the three second buffers of the role-flip / one-pass steps, one per tracer (ff1p)
        const size_t total = (size_t)(nr8 + 3 + ntr) * r8b + (size_t)OCN_NUM_R4 * r4b + 256;
        HIPCHK(hipMalloc(&b.slab, total));
        c->allocs.push_back(b.slab);
        HIPCHK(hipMemsetAsync(b.slab, 0, total, c->stream));
        char *base = (char *)b.slab;
        size_t off = 0;
        b.ptr.assign((size_t)(OCN_NUM_R4 + nr8), nullptr);
        // r8 order in the slab: the one-pass step's state fields and their second buffers first,
        // next to each other (the arrays one march streams through share DRAM pages and TLB
        // entries), then the other SW fields, then the tracers'.  (Kernels address every field
        // through its own pointer; only byte offsets within one field are 32-bit.)
        std::vector<int> order = {OCN_SSH, OCN_SSHN, OCN_SSHP, OCN_UBRTR, OCN_UBRTRN, OCN_UBRTRP, OCN_VBRTR,
                                  OCN_VBRTRN, OCN_VBRTRP, -1, -2, -3, OCN_HHU, OCN_HHU_P, OCN_HHV, OCN_HHV_P, OCN_HHH,
                                  OCN_HHQ_REST, OCN_VORT, OCN_STR_T, OCN_STR_S, OCN_MU, OCN_RHSX, OCN_RHSY};
        for (int id = OCN_SSH; id < OCN_SSH + nr8; ++id)
            if (std::find(order.begin(), order.end(), id) == order.end()) order.push_back(id);
        for (int k = 1; k <= ntr; ++k) order.push_back(-3 - k);
        b.ffp_alt.assign((size_t)ntr, nullptr);
        for (int id : order) {
            char *p = base + off + 256 - 16 + xr;
            off += r8b;
            if (id == -1) b.sshp_alt = p;
            else if (id == -2) b.up_alt = p;
            else if (id == -3) b.vp_alt = p;
            else if (id < -3) b.ffp_alt[(size_t)(-4 - id)] = p;
            else b.ptr[field_slot(id)] = p;
        }
        for (int id = 0; id < OCN_NUM_R4; ++id) {
            b.ptr[field_slot(id)] = base + off + 256 - 8;
            off += r4b;
        }
    }
    for (LBlock &b : c->blocks) {
        const size_t n = (size_t)b.g.pitch * (b.g.bnd_y2 - b.g.bnd_y1 + 1);
        // metric row tables + ratios + reciprocals (sw_stencils.h kRowTable, recip_offset)
        const size_t nrow = row_table_size((unsigned)(b.g.bnd_y2 - b.g.bnd_y1 + 1));
        HIPCHK(hipMalloc(&b.bits, n));
        c->allocs.push_back(b.bits);
        HIPCHK(hipMalloc(&b.rows, nrow * sizeof(float)));
        c->allocs.push_back(b.rows);
        RC(allocate_x2(c, b));
    }
    // d_nbad words: 0 check_ssh_err's count, 16 the fallback check's verdict (d_fbz) and 17 its mu word, 32..47 flags and
    // the vote (d_flags), 56 the count's maximum over the ranks (sync_impl), 61 the multi-step launch's
    // barrier timeout flag; then per block h_r, mu (LBlock::kc); then the loopback vote's reduction
    // (d_red: 64 words)
    const size_t kcb = 16 * c->blocks.size();
    HIPCHK(hipMalloc(&c->d_nbad, 256 + kcb + 256));
    c->allocs.push_back(c->d_nbad);
    HIPCHK(hipMalloc(&c->d_bar, kMultiBarBytes));
    c->allocs.push_back(c->d_bar);
    HIPCHK(hipMemsetAsync(c->d_nbad, 0, 256 + kcb + 256, c->stream));
    c->d_red = (int32_t *)((char *)c->d_nbad + 256 + kcb);
    c->d_fbz = c->d_nbad + kFbzWord;   // (and kFbzWord + 1: its mu word)
    c->d_flags = c->d_nbad + 32;
    for (size_t i = 0; i < c->blocks.size(); ++i) c->blocks[i].kc = (double *)((char *)c->d_nbad + 256) + 2 * i;
    return OCN_OK;
}

// (Re)builds the compact static fields when the real(4) fields may have changed, and decides
// whether the fused step reads them (sw_stencils.h "compact static fields").  Synchronises
// only when a rebuild was needed (once after init / an upload of a real(4) field).
int prepare_static(ocn_ctx *c)
{
    if (!c->compact_req || c->r4_escaped) { c->compact = false; return OCN_OK; }
    if (!c->static_dirty) return OCN_OK;
    HIPCHK(hipMemsetAsync(c->d_flags, 0, 3 * sizeof(int32_t), c->stream));
    RC(each_block(c, c->stream, [&](const LBlock &b) { return launch_prepare(&b.g, b.ptr.data(), b.bits, b.rows, c->d_flags, c->stream, b.own); }));
    if (c->ext_ok)   // one_step_x2's row tables: the ext rows' divisor range into the second word
        for (const LBlock &b : c->blocks) RC(launch_rows_ext(&b.g, b.rows, b.rows_x, b.ext, c->d_flags + 1, c->stream));
    const bool x4_tabs = c->ext_ok && has_exchange(c);
    int32_t *d_mask = nullptr;
    if (x4_tabs) {   // one_step_x4's tables (the neighbours' mask bytes from the basin mask): the third word
        const size_t nxy = (size_t)c->basin.nx * c->basin.ny;
        HIPCHK(hipMallocAsync((void **)&d_mask, nxy * sizeof(int32_t), c->stream));
        HIPCHK(hipMemcpyAsync(d_mask, c->mask.data(), nxy * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        for (const LBlock &b : c->blocks)
            RC(launch_x4_tables(&b.g, b.bits, b.rows, b.ext, b.bits_x4, b.rows_x4, d_mask, c->basin.nx, c->basin.ny, b.own,
                                c->d_flags + 2, c->stream));
        HIPCHK(hipFreeAsync(d_mask, c->stream));
    }
    int32_t flags[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(flags, c->d_flags, sizeof(flags), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->ring_sea = (flags[0] & kCompactRingSea) != 0;
    c->edge_ring_sea = (flags[0] & kCompactEdgeRingSea) != 0;
    c->udiv_ok = (flags[0] & kCompactDivisorRange) == 0;
    c->rows_x_ok = c->ext_ok && flags[1] == 0;
    c->x4_tab_ok = x4_tabs && (flags[2] & ~kCompactViscousRow) == 0;
    // (the inviscid bodies: the block's rows, and the neighbours' rows in one_step_x4's tables)
    c->rdiss_zero = ((flags[0] | flags[2]) & kCompactViscousRow) == 0;
    c->compact = (flags[0] & ~(kCompactRingSea | kCompactDivisorRange | kCompactEdgeRingSea | kCompactViscousRow)) == 0;
    c->static_dirty = false;
    return OCN_OK;
}

// ------------------------------------------------------------------ initial state
// init_grid_data + init_ocean_data (control/init_data.f90:29-125) with every 2-D field formed on
// the device (init_kernels.hip); the host supplies the basin mask and the grid's O(nx + ny)
// trigonometric row / column factors from its libm, as the reference computes them.
static const float kPi = 3.1415926f;              // constants.f90:14
static const double kDPi = 3.14159265358979;      // constants.f90:17
static const double kLatExtr = 89.99999;          // constants.f90:20
static const float kRadEarth = 6371000.0f;        // constants.f90:22
static const float kEarthAngVel = 7.2921159e-5f;  // constants.f90:22
static double dsind(double x) { return std::sin((x / 180.0) * kDPi); }   // core/math_tools.f90
static double dcosd(double x) { return std::cos((x / 180.0) * kDPi); }

// One block's grid tables in one device allocation (freed by the caller after the launch ran):
// grid_base_init's coordinates xt / xu (columns) and yt / yv (rows) (grid_kernels.f90:94-202),
// then grid_geo_init's factors of them (grid_parameters.f90:80-181).
struct GridTables {
    std::vector<float> cos_t, cos_v;                   // (float) dcosd(lat_mod(yt)), of yv, per row
    std::vector<double> sin_v, cosy_v, cos_xu;         // dsind(yv), dcosd(yv) per row; dcosd(xu) per column
    // the same factors of rows bnd_y1 and bnd_y2 (outside the metric range) from the global row
    // formulas, as the neighbour blocks form them (GridInit ext)
    float ext_ct[kExtRows], ext_cv[kExtRows];
    double ext_sin_v[kExtRows], ext_cosy_v[kExtRows];
};
static void grid_tables(const ocn_ctx *c, const ocn_block &g, GridTables &t)
{
    const ocn_basin &bs = c->basin;
    const int w = g.bnd_x2 - g.bnd_x1 + 1, h = g.bnd_y2 - g.bnd_y1 + 1, mmm = 3, nnn = 3;
    std::vector<double> xt(w), xu(w, 0.0), yt(h), yv(h, 0.0);
    for (int m = g.bnd_x1; m <= g.bnd_x2; ++m) xt[m - g.bnd_x1] = bs.rlon + (double)(m - mmm) * bs.dxst;
    for (int n = g.bnd_y1; n <= g.bnd_y2; ++n) yt[n - g.bnd_y1] = bs.rlat + (double)(n - nnn) * bs.dyst;
    for (int i = 0; i + 1 < w; ++i) xu[i] = (xt[i] + xt[i + 1]) / 2.0;
    for (int i = 0; i + 1 < h; ++i) yv[i] = (yt[i] + yt[i + 1]) / 2.0;
    auto lat_mod = [](double y) { return std::max(std::min(y, kLatExtr), -kLatExtr); };
    t.cos_t.assign(h, 0.0f); t.cos_v.assign(h, 0.0f); t.sin_v.assign(h, 0.0); t.cosy_v.assign(h, 0.0);
    t.cos_xu.assign(w, 0.0);
    for (int n = g.ny_start - 1; n <= g.ny_end + 1; ++n) {   // the metric range's rows and columns
        const int r = n - g.bnd_y1;
        t.cos_t[r] = (float)dcosd(lat_mod(yt[r]));
        t.cos_v[r] = (float)dcosd(lat_mod(yv[r]));
        t.sin_v[r] = dsind(yv[r]);
        t.cosy_v[r] = dcosd(yv[r]);
    }
    for (int m = g.nx_start - 1; m <= g.nx_end + 1; ++m) t.cos_xu[m - g.bnd_x1] = dcosd(xu[m - g.bnd_x1]);
    // grid_base_init on the neighbour: yt(n), yv(n) = (yt(n) + yt(n + 1)) / 2 (GridInit ext's rows)
    const int ext_row[kExtRows] = {g.bnd_y1, g.bnd_y2, g.bnd_y1 - 1, g.bnd_y1 - 2, g.bnd_y2 + 1, g.bnd_y2 + 2};
    for (int i = 0; i < kExtRows; ++i) {
        const int n = ext_row[i];
        const double yt_n = bs.rlat + (double)(n - nnn) * bs.dyst, yt_n1 = bs.rlat + (double)(n + 1 - nnn) * bs.dyst;
        const double yv_n = (yt_n + yt_n1) / 2.0;
        t.ext_ct[i] = (float)dcosd(lat_mod(yt_n));
        t.ext_cv[i] = (float)dcosd(lat_mod(yv_n));
        t.ext_sin_v[i] = dsind(yv_n);
        t.ext_cosy_v[i] = dcosd(yv_n);
    }
}

int upload_field(ocn_ctx *c, const LBlock &b, int id, const void *host, bool async)
{
    const size_t es = is_r4(id) ? 4 : 8;
    const size_t w = (size_t)(b.g.bnd_x2 - b.g.bnd_x1 + 1), rows = (size_t)(b.g.bnd_y2 - b.g.bnd_y1 + 1);
    if (async)
        HIPCHK(hipMemcpy2DAsync(b.ptr[field_slot(id)], (size_t)b.g.pitch * es, host, w * es, w * es, rows,
                                hipMemcpyHostToDevice, c->stream));
    else
        HIPCHK(hipMemcpy2D(b.ptr[field_slot(id)], (size_t)b.g.pitch * es, host, w * es, w * es, rows,
                           hipMemcpyHostToDevice));
    return OCN_OK;
}

int init_state(ocn_ctx *c)
{
    HIPCHK(hipStreamSynchronize(c->stream));
    const ocn_basin &bs = c->basin;
    const size_t nxy = (size_t)bs.nx * bs.ny;
    // device scratch of this call: the basin mask, then per block its grid tables
    std::vector<GridTables> tabs(c->blocks.size());
    const size_t topo_at = (nxy * sizeof(int32_t) + 255) / 256 * 256;
    size_t bytes = topo_at + c->topo.size() * sizeof(float);
    std::vector<size_t> at(c->blocks.size());
    for (size_t i = 0; i < c->blocks.size(); ++i) {
        grid_tables(c, c->blocks[i].g, tabs[i]);
        at[i] = (bytes + 255) / 256 * 256;
        bytes = at[i] + tabs[i].cos_t.size() * 2 * 4 + 256 + (tabs[i].sin_v.size() * 2 + tabs[i].cos_xu.size()) * 8;
    }
    char *scratch = nullptr;
    HIPCHK(hipMalloc(&scratch, bytes));
    struct Free { char *p; ~Free() { if (p) (void)hipFree(p); } } free_scratch{scratch};
    HIPCHK(hipMemcpy(scratch, c->mask.data(), nxy * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!c->topo.empty())
        HIPCHK(hipMemcpy(scratch + topo_at, c->topo.data(), c->topo.size() * sizeof(float), hipMemcpyHostToDevice));
    const float pip180 = kPi / 180.0f;
    for (size_t i = 0; i < c->blocks.size(); ++i) {
        const LBlock &b = c->blocks[i];
        const GridTables &t = tabs[i];
        const size_t h = t.cos_t.size(), w = t.cos_xu.size();
        char *p = scratch + at[i];
        GridInit q{};
        q.g = b.g;
        q.mask = (const int32_t *)scratch;
        q.nx = bs.nx;
        for (int id = 0; id < OCN_NUM_R4; ++id) q.r4[id] = b.f<float>(id);
        q.cos_t = (const float *)p; q.cos_v = q.cos_t + h;
        p += (h * 2 * 4 + 255) / 256 * 256;
        q.sin_v = (const double *)p; q.cosy_v = q.sin_v + h; q.cos_xu = q.cosy_v + h;
        HIPCHK(hipMemcpy((void *)q.cos_t, t.cos_t.data(), h * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy((void *)q.cos_v, t.cos_v.data(), h * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy((void *)q.sin_v, t.sin_v.data(), h * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy((void *)q.cosy_v, t.cosy_v.data(), h * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy((void *)q.cos_xu, t.cos_xu.data(), w * 8, hipMemcpyHostToDevice));
        q.cos_rot = dcosd(bs.rotation_on_lat);
        q.sin_rot = dsind(bs.rotation_on_lat);
        q.sin_extr = dsind(kLatExtr);
        q.sx = (float)bs.dxst * pip180 * kRadEarth;
        q.sy = (float)bs.dyst * pip180 * kRadEarth;
        q.cor = 2.0f * kEarthAngVel;
        q.sqrt2 = std::sqrt(2.0f);
        q.curve = bs.curve_grid != 0;
        for (int j = 0; j < kExtRows; ++j) {
            q.ext_ct[j] = t.ext_ct[j]; q.ext_cv[j] = t.ext_cv[j];
            q.ext_sin_v[j] = t.ext_sin_v[j]; q.ext_cosy_v[j] = t.ext_cosy_v[j];
        }
        q.ext = b.ext;
        RC(launch_init_grid(q, c->stream));
        c->static_dirty = true;
        if (c->topo.empty()) {
            RC(launch_fill_field(b.g, b.f<double>(OCN_HHQ_REST), 100.0, c->stream));   // init_data.f90:112-114
        } else {
            const long pts = (long)(b.g.bnd_x2 - b.g.bnd_x1 + 1) * (b.g.bnd_y2 - b.g.bnd_y1 + 1);
            hipLaunchKernelGGL(k_topography, dim3((unsigned)((pts + 255) / 256)), dim3(256), 0, c->stream, b.g,
                               b.f<double>(OCN_HHQ_REST), b.f<float>(OCN_LU), (const float *)(scratch + topo_at), bs.nx - 4);
            RC(check_launch());
        }
        RC(launch_gaussian(b.g, b.f<double>(OCN_SSH), b.f<float>(OCN_LU), bs.nx / 2, bs.ny / 2, 1.0, c->stream));
    }
    if (!c->topo.empty()) RC(run_sync(c, {OCN_HHQ_REST}));   // init_data.f90:119
    RC(run_sync(c, {OCN_SSH}));                               // envoke_gaussian_elimination's sync
    for (const LBlock &b : c->blocks) {                       // sshn = ssh, sshp = ssh (whole arrays)
        const size_t bytes = (size_t)b.g.pitch * (b.g.bnd_y2 - b.g.bnd_y1 + 1) * 8;
        HIPCHK(hipMemcpyAsync(b.ptr[field_slot(OCN_SSHN)], b.ptr[field_slot(OCN_SSH)], bytes,
                              hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(b.ptr[field_slot(OCN_SSHP)], b.ptr[field_slot(OCN_SSH)], bytes,
                              hipMemcpyDeviceToDevice, c->stream));
    }
    RC(envoke(c, OCN_STAGE_HH_INIT, 0.0));                    // init_data.f90:60-63
    for (const LBlock &b : c->blocks) {                       // u = v = 0, mu = lvisc_2 then 0 (:67-77)
        const long n = (long)b.g.pitch * (b.g.bnd_y2 - b.g.bnd_y1 + 1);
        for (int id : {OCN_UBRTR, OCN_UBRTRN, OCN_UBRTRP, OCN_VBRTR, OCN_VBRTRN, OCN_VBRTRP, OCN_MU}) {
            hipLaunchKernelGGL(k_fill_r8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                               b.f<double>(id), n, 0.0);
            RC(check_launch());
        }
    }
    if (c->sw.use_tracers > 0) {                              // init_data.f90:80-90
        for (int k = 1; k <= c->sw.tracer_num; ++k) {
            for (const LBlock &b : c->blocks)
                RC(launch_gaussian(b.g, b.f<double>(OCN_FF1(k)), b.f<float>(OCN_LU), bs.nx / 2, bs.ny / 2, 0.5,
                                   c->stream));
            RC(run_sync(c, {OCN_FF1(k)}));
            for (const LBlock &b : c->blocks) {
                const size_t bytes = (size_t)b.g.pitch * (b.g.bnd_y2 - b.g.bnd_y1 + 1) * 8;
                HIPCHK(hipMemcpyAsync(b.ptr[field_slot(OCN_FF1N(k))], b.ptr[field_slot(OCN_FF1(k))], bytes,
                                      hipMemcpyDeviceToDevice, c->stream));
                HIPCHK(hipMemcpyAsync(b.ptr[field_slot(OCN_FF1P(k))], b.ptr[field_slot(OCN_FF1(k))], bytes,
                                      hipMemcpyDeviceToDevice, c->stream));
            }
        }
        for (const LBlock &b : c->blocks) {
            const long n = (long)b.g.pitch * (b.g.bnd_y2 - b.g.bnd_y1 + 1);
            for (int id : {OCN_FLUX_X, OCN_FLUX_Y}) {
                hipLaunchKernelGGL(k_fill_r8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                                   b.f<double>(id), n, 0.0);
                RC(check_launch());
            }
        }
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->initialized = true;
    c->ext_ok = true;   // the real(4) fields are init_state's: the ext rows are the neighbours' metric rows
    c->hrx_ok = false;
    return OCN_OK;
}

void set_mask(ocn_ctx *c, const int32_t *mask)
{
    const ocn_basin *basin = &c->basin;
    const size_t nxy = (size_t)basin->nx * basin->ny;
    c->mask.assign(nxy, 0);
    if (mask) {
        std::memcpy(c->mask.data(), mask, nxy * sizeof(int32_t));
    } else {   // tools/io.f90:49-59: closed box with a 2-cell land frame
        for (int n = 1; n <= basin->ny; ++n)
            for (int m = 1; m <= basin->nx; ++m)
                c->mask[(size_t)(m - 1) + (size_t)(n - 1) * basin->nx] =
                    (m < 3 || m > basin->nx - 2 || n < 3 || n > basin->ny - 2) ? 1 : 0;
    }
}

// host-only context (decomposition only, no device) for the query entry points
int host_ctx(const ocn_basin *basin, const ocn_decomp *dec, const int32_t *mask, ocn_ctx *&c)
{
    if (!basin || !dec) return set_error(OCN_ERR_ARG, "null argument");
    if (basin->nx < 5 || basin->ny < 5) return set_error(OCN_ERR_ARG, "nx, ny must be >= 5");
    if (dec->bnx < 1 || dec->bny < 1 || dec->nranks < 1 || dec->rank < 0 || dec->rank >= dec->nranks)
        return set_error(OCN_ERR_ARG, "bad decomposition request");
    c = new ocn_ctx();
    c->basin = *basin; c->dec = *dec; c->bnx = dec->bnx; c->bny = dec->bny;
    set_mask(c, mask);
    const int rc = decompose(c);
    if (rc) { delete c; c = nullptr; }
    return rc;
}

}  // namespace ocn

extern "C" {

int ocn_decompose(const ocn_basin *basin, const ocn_decomp *dec, const int32_t *mask, ocn_block_info *out,
                  int32_t cap, int32_t *count)
{
    ocn_ctx *c = nullptr;
    RC(host_ctx(basin, dec, mask, c));
    const int n = (int)c->blocks.size();
    if (count) *count = n;
    for (int k = 0; k < n && k < cap && out; ++k) {
        const LBlock &b = c->blocks[k];
        out[k].geom = b.g; out[k].bm = b.bm; out[k].bn = b.bn;
        for (int d = 0; d < 8; ++d) { out[k].nbr_rank[d] = b.nbr_rank[d]; out[k].nbr_k[d] = b.nbr_k[d]; }
    }
    delete c;
    return OCN_OK;
}

}  // extern "C"
