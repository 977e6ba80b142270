// ens_forcing.hip -- the moving-storm forcing of an ensemble's members (ocn_sw.h ocn_ens_forcing_apply).
//
// k_ens_forcing: OCN_RHSX and OCN_RHSY of every forced member of one block for one time t, at the interior points
// nx_start..nx_end x ny_start..ny_end, by ens_forcing_point.h frc_point -- the header's operations in the header's
// order (-ffp-contract=off, IEEE division and sqrt, Makefile: the bits of ocean_model_arch_amd/ens_forcing_rule.py).
// Layout as k_ens_inflate: one point per lane, lanes along x, a wave's first lane on a 256-B line (lead), a
// workgroup 64 columns x 4 rows; grid.z is the member.  A member's storm and array pointers are one EnsFrcMember
// of a table in device memory, written by a copy ordered before the launch and never by a kernel: read through
// the constant address space (uniform scalar loads, as k_march_multi_b's EnsEntry); a member that is not forced
// ends at once.  A lane reads the real(4) masks and metrics and h_r of its own point and of the points one to
// the east and one to the north (inside the array: the interior has a halo ring), global indices from the
// block's bounds, so the result does not depend on the block grid.  A lane writes its own point only: plain
// stores, no atomics, no inline assembly, no LDS.
#include "ens_forcing_point.h"
#include "ocn_internal.h"

namespace ocn {

constexpr int kFrcRows = 4, kFrcCols = 64;   // a workgroup: one wave per row (k_ens_inflate's)

__global__ __launch_bounds__(256) void k_ens_forcing(const EnsFrcMember *__restrict__ tab, const ocn_ens_forcing_model mo,
                                                     double t, int i0, int i1, int j0, int j1, long pitch, int lead, int gx,
                                                     int gy)
{
    typedef const EnsFrcMember __attribute__((address_space(4))) *ConstTab;
    ConstTab e = (ConstTab)tab + blockIdx.z;
    if (!e->forced) return;
    const int i = (int)(blockIdx.x * kFrcCols + threadIdx.x) - lead, j = (int)(blockIdx.y * kFrcRows + threadIdx.y);
    if (i < i0 || i > i1 || j < j0 || j > j1) return;
    const long at = (long)j * pitch + i;
    const ocn_ens_storm s = *(const ocn_ens_storm *)&e->s;
    const float *const dx = e->dx, *const dy = e->dy;
    const double *const hr = e->hr;
    FrcPoint p;
    p.lcu = e->lcu[at]; p.lcv = e->lcv[at];
    p.dxt = e->dxt[at]; p.dyt = e->dyt[at]; p.dxh = e->dxh[at]; p.dyh = e->dyh[at];
    p.dx0 = dx[at]; p.dy0 = dy[at]; p.dx1 = dx[at + 1]; p.dy1 = dy[at + 1]; p.dx2 = dx[at + pitch]; p.dy2 = dy[at + pitch];
    p.h0 = hr[at]; p.h1 = hr[at + 1]; p.h2 = hr[at + pitch];
    const FrcAt c = frc_at(s, mo, t);
    double rx, ry;
    frc_point(s, mo, c, gx + i, gy + j, p, rx, ry);
    e->rx[at] = rx;
    e->ry[at] = ry;
}

int launch_ens_forcing(const ocn_block *b, const EnsFrcMember *d_tab, int members, const ocn_ens_forcing_model &model,
                       double t, int lead, hipStream_t s)
{
    if (!b || !d_tab || members < 1 || members > OCN_ENS_MAX_MEMBERS || lead < 0 || lead > 31)
        return set_error(OCN_ERR_ARG, "ens_forcing: block, table or member count");
    // (the points one to the east and one to the north of an interior point lie inside the array)
    if (b->nx_start < b->bnd_x1 || b->ny_start < b->bnd_y1 || b->nx_end >= b->bnd_x2 || b->ny_end >= b->bnd_y2 ||
        b->pitch < b->bnd_x2 - b->bnd_x1 + 1)
        return set_error(OCN_ERR_ARG, "ens_forcing: an interior without a halo ring");
    if (b->nx_end < b->nx_start || b->ny_end < b->ny_start) return OCN_OK;
    const int i0 = b->nx_start - b->bnd_x1, i1 = b->nx_end - b->bnd_x1, j0 = b->ny_start - b->bnd_y1, j1 = b->ny_end - b->bnd_y1;
    const dim3 grid((unsigned)((i1 + 1 + lead + kFrcCols - 1) / kFrcCols), (unsigned)((j1 + 1 + kFrcRows - 1) / kFrcRows),
                    (unsigned)members);
    hipLaunchKernelGGL(k_ens_forcing, grid, dim3((unsigned)kFrcCols, (unsigned)kFrcRows), 0, s, d_tab, model, t, i0, i1, j0, j1,
                       (long)b->pitch, lead, (int)b->bnd_x1, (int)b->bnd_y1);
    return check_launch();
}

}  // namespace ocn
