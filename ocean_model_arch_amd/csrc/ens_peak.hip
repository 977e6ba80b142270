// ens_peak.hip -- the peak map of an ensemble's members (ocn_sw.h ocn_ens_peak_*): per point the highest and / or
// lowest value a prognostic field has had after a step since ocn_ens_peak_begin, and that step's number.
//
// k_ens_peak: every tracked member of one block, at the interior points nx_start..nx_end x ny_start..ny_end.
// Layout as k_ens_inflate: one point per lane, lanes along x, a wave's first lane on a 256-B line (lead), a
// workgroup 64 columns x 4 rows; grid.z is the member.  A member's arrays are one EnsPeakMember of a table in
// device memory, written by a copy ordered before the launch and never by a kernel: read through the constant
// address space (uniform scalar loads, as k_ens_forcing's table); a member that is not tracked ends at once.
//   k = 0 (init):     P = x, S = 0
//   k >= 1 (update):  ens_peak_point.h peak_takes: MAX if (x > P || P != P) { P = x; S = k; }, MIN with <
// x is the field's value at the point as the table's src[0] names the array.  A lane reads and writes its own
// point only; P and S are stored only where the rule replaces them (a divergent branch: the others keep their
// bits).  It serves ocn_ens_peak_begin, every step of the chunked route and the last step of an in-launch call
// (sw_kernels.hip k_march_multi_pk does the steps before it).
// k_ens_exceed: per point of the block's array the fraction of the members in use whose Pmax exceeds a threshold,
// the members' pointers by value in the kernel arguments, indexed uniformly (as k_ens_stats has them), counted in
// member order; a NaN compares false and is not counted.
// No atomics, no LDS, no inline assembly.
#include "ens_peak_point.h"
#include "ocn_internal.h"

namespace ocn {

constexpr int kPkRows = 4, kPkCols = 64;   // a workgroup: one wave per row (k_ens_inflate's)

__global__ __launch_bounds__(256) void k_ens_peak(const EnsPeakMember *__restrict__ tab, int k, int i0, int i1, int j0, int j1,
                                                  long pitch, int lead)
{
    typedef const EnsPeakMember __attribute__((address_space(4))) *ConstTab;
    ConstTab e = (ConstTab)tab + blockIdx.z;
    if (!e->tracked) return;
    const int i = (int)(blockIdx.x * kPkCols + threadIdx.x) - lead, j = (int)(blockIdx.y * kPkRows + threadIdx.y);
    if (i < i0 || i > i1 || j < j0 || j > j1) return;
    const long at = (long)j * pitch + i;
    const double x = e->src[0][at];
    double *const pmax = e->pmax, *const pmin = e->pmin;
    int32_t *const smax = e->smax, *const smin = e->smin;
    if (k == 0) {
        if (pmax) { pmax[at] = x; smax[at] = 0; }
        if (pmin) { pmin[at] = x; smin[at] = 0; }
        return;
    }
    if (pmax && peak_takes<false>(x, pmax[at])) { pmax[at] = x; smax[at] = k; }
    if (pmin && peak_takes<true>(x, pmin[at])) { pmin[at] = x; smin[at] = k; }
}

int launch_ens_peak(const ocn_block *b, const EnsPeakMember *d_tab, int members, int k, int lead, hipStream_t s)
{
    if (!b || !d_tab || members < 1 || members > OCN_ENS_MAX_MEMBERS || k < 0 || lead < 0 || lead > 31)
        return set_error(OCN_ERR_ARG, "ens_peak: block, table, member count or step");
    if (b->nx_start < b->bnd_x1 || b->ny_start < b->bnd_y1 || b->nx_end > b->bnd_x2 || b->ny_end > b->bnd_y2 ||
        b->pitch < b->bnd_x2 - b->bnd_x1 + 1)
        return set_error(OCN_ERR_ARG, "ens_peak: an interior outside the array");
    if (b->nx_end < b->nx_start || b->ny_end < b->ny_start) return OCN_OK;
    const int i0 = b->nx_start - b->bnd_x1, i1 = b->nx_end - b->bnd_x1, j0 = b->ny_start - b->bnd_y1, j1 = b->ny_end - b->bnd_y1;
    const dim3 grid((unsigned)((i1 + 1 + lead + kPkCols - 1) / kPkCols), (unsigned)((j1 + 1 + kPkRows - 1) / kPkRows),
                    (unsigned)members);
    hipLaunchKernelGGL(k_ens_peak, grid, dim3((unsigned)kPkCols, (unsigned)kPkRows), 0, s, d_tab, k, i0, i1, j0, j1,
                       (long)b->pitch, lead);
    return check_launch();
}

struct EnsPkPtrs { const double *p[OCN_ENS_MAX_MEMBERS]; };   // the members' Pmax arrays, by value (as k_ens_stats')

__global__ __launch_bounds__(256) void k_ens_exceed(const EnsPkPtrs mem, int n, int w, int h, long pitch, int lead,
                                                    double threshold, double *__restrict__ out)
{
    const int i = (int)(blockIdx.x * kPkCols + threadIdx.x) - lead, j = (int)(blockIdx.y * kPkRows + threadIdx.y);
    if (i < 0 || i >= w || j >= h) return;
    const long at = (long)j * pitch + i;
    int c = 0;
    for (int g = 0; g < n; g += 8) {   // (8 members' loads ahead of the compares; the tail behind uniform branches)
        double x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (g + e < n) x[e] = mem.p[g + e][at];
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (g + e < n) c += x[e] > threshold ? 1 : 0;
    }
    out[(long)j * w + i] = (double)c / (double)n;
}

int launch_ens_exceed(const ocn_block *b, const double *const *pmax, int n, double threshold, double *d_out, hipStream_t s)
{
    if (!b || !pmax || n < 1 || n > OCN_ENS_MAX_MEMBERS || !d_out) return set_error(OCN_ERR_ARG, "ens_exceed: block, members or buffer");
    EnsPkPtrs p;
    for (int i = 0; i < OCN_ENS_MAX_MEMBERS; ++i) p.p[i] = pmax[i < n ? i : 0];
    const int w = b->bnd_x2 - b->bnd_x1 + 1, h = b->bnd_y2 - b->bnd_y1 + 1;
    const int lead = (int)(((uintptr_t)pmax[0] & 255u) / 8u);
    for (int i = 0; i < n; ++i)
        if ((int)(((uintptr_t)pmax[i] & 255u) / 8u) != lead) return set_error(OCN_ERR_STATE, "ens_exceed: members' layouts differ");
    const dim3 grid((unsigned)((w + lead + kPkCols - 1) / kPkCols), (unsigned)((h + kPkRows - 1) / kPkRows));
    hipLaunchKernelGGL(k_ens_exceed, grid, dim3((unsigned)kPkCols, (unsigned)kPkRows), 0, s, p, n, w, h, (long)b->pitch, lead,
                       threshold, d_out);
    return check_launch();
}

}  // namespace ocn
