// ens_stats.hip -- statistics over the members of an ensemble (ocn_sw.h ocn_ens_stats, ocn_ens_extrema).
//
// k_ens_stats: per point of one real(8) field of one block, over the members in use in member order:
//   MEAN    s = x0; s = s + x_i (i = 1 .. n-1, in that order); mean = s / (double)n
//   VAR     d_i = x_i - mean; q = d0 d0; q = q + d_i d_i (product rounded, then the sum); var = q / (double)(n-1)
//   SPREAD  sqrt(var)
//   MIN     c = x0; if (x_i < c || c != c) c = x_i       MAX: the same with >
// -ffp-contract=off and IEEE division / sqrt (Makefile) make these the bits of the restatement in
// tests/ens_stats_ref.py.  One point per lane, lanes along x, a wave's first lane on a 256-B line; the
// members' base pointers by value in the kernel arguments (the member index is uniform: scalar loads of
// the pointers); 8 members' loads are issued ahead of the ordered adds.  Up to kEnsStatsReg members the
// values stay in registers and VAR costs no second read; beyond, the second pass reads the members
// again: the same operations in the same order, so the same bits.  No atomics, no LDS.
//
// k_ens_extrema + k_ens_extrema_final: per member, min / max over the finite values, the count of
// non-finite ones and the count of points, over the interior sea points (|lu| >= 0.5) of every local
// block: one wave per 64 x kExtremaRows tile and member writes a partial, one wave per member folds them.
#include "ocn_internal.h"

namespace ocn {

constexpr int kStatsAhead = 8;   // members whose loads are in flight before the ordered adds

struct EnsStatsPtrs { const double *p[OCN_ENS_MAX_MEMBERS]; };

template <bool MIN>
__device__ __forceinline__ double ext_take(double c, double x)
{
    return ((MIN ? x < c : x > c) || c != c) ? x : c;
}

// REG: n <= kEnsStatsReg, the members' values kept in registers for the variance
template <bool REG>
__global__ __launch_bounds__(256) void k_ens_stats(const EnsStatsPtrs src, int n, int w, int h, long pitch, int lead,
                                                   int need_var, double *mean_out, double *var_out,
                                                   double *spread_out, double *min_out, double *max_out)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - lead, j = (int)blockIdx.y;
    if (i < 0 || i >= w || j >= h) return;
    const long at = (long)j * pitch + i;
    constexpr int kKeep = REG ? kEnsStatsReg : kStatsAhead;
    constexpr int kGroups = REG ? kEnsStatsReg / kStatsAhead : 1;   // REG: the groups' loops unrolled, x[] in registers
    double x[kKeep];
    double s = 0.0, lo = 0.0, hi = 0.0;
#pragma unroll kGroups
    for (int g = 0; g < (REG ? kEnsStatsReg : n); g += kStatsAhead) {
        if (g >= n) break;
        double *v = REG ? x + g : x;
#pragma unroll
        for (int e = 0; e < kStatsAhead; ++e)
            if (g + e < n) v[e] = src.p[g + e][at];
#pragma unroll
        for (int e = 0; e < kStatsAhead; ++e) {
            if (g + e >= n) break;
            if (g + e == 0) {
                s = lo = hi = v[e];
            } else {
                s = s + v[e];
                lo = ext_take<true>(lo, v[e]);
                hi = ext_take<false>(hi, v[e]);
            }
        }
    }
    const double mean = s / (double)n;
    if (mean_out) mean_out[at] = mean;
    if (min_out) min_out[at] = lo;
    if (max_out) max_out[at] = hi;
    if (!need_var) return;
    double q = 0.0;
#pragma unroll kGroups
    for (int g = 0; g < (REG ? kEnsStatsReg : n); g += kStatsAhead) {
        if (g >= n) break;
        double *v = REG ? x + g : x;
        if (!REG) {
#pragma unroll
            for (int e = 0; e < kStatsAhead; ++e)
                if (g + e < n) v[e] = src.p[g + e][at];
        }
#pragma unroll
        for (int e = 0; e < kStatsAhead; ++e) {
            if (g + e >= n) break;
            const double d = v[e] - mean;
            const double dd = d * d;
            q = g + e == 0 ? dd : q + dd;
        }
    }
    const double var = q / (double)(n - 1);
    if (var_out) var_out[at] = var;
    if (spread_out) spread_out[at] = sqrt(var);
}

int launch_ens_stats(const ocn_block *b, const double *const *src, int n, bool need_var, double *const out[5],
                     hipStream_t s)
{
    if (n < 1 || n > OCN_ENS_MAX_MEMBERS || (need_var && n < 2)) return set_error(OCN_ERR_ARG, "ens_stats: member count");
    EnsStatsPtrs p;
    for (int i = 0; i < OCN_ENS_MAX_MEMBERS; ++i) p.p[i] = src[i < n ? i : 0];
    const int w = b->bnd_x2 - b->bnd_x1 + 1, h = b->bnd_y2 - b->bnd_y1 + 1;
    // the lane of A(bnd_x1, :) within its 256-B line: a wave's first lane then starts a line
    const int lead = (int)(((uintptr_t)src[0] & 255u) / 8u);
    for (int i = 0; i < n; ++i)
        if ((int)(((uintptr_t)src[i] & 255u) / 8u) != lead) return set_error(OCN_ERR_STATE, "ens_stats: members' layouts differ");
    const dim3 grid((unsigned)((w + lead + 255) / 256), (unsigned)h);
    if (n <= kEnsStatsReg)
        hipLaunchKernelGGL(k_ens_stats<true>, grid, dim3(256), 0, s, p, n, w, h, (long)b->pitch, lead, need_var ? 1 : 0,
                           out[0], out[1], out[2], out[3], out[4]);
    else
        hipLaunchKernelGGL(k_ens_stats<false>, grid, dim3(256), 0, s, p, n, w, h, (long)b->pitch, lead, need_var ? 1 : 0,
                           out[0], out[1], out[2], out[3], out[4]);
    return check_launch();
}

// ------------------------------------------------------------------ per-member extrema
constexpr int kExtremaRows = 16;   // rows of one wave's tile (64 columns wide)

__device__ __forceinline__ void ext_fold(EnsPartial &a, const EnsPartial &b)
{
    a.min = b.min < a.min ? b.min : a.min;
    a.max = b.max > a.max ? b.max : a.max;
    a.nonfinite += b.nonfinite;
    a.count += b.count;
}

__device__ __forceinline__ EnsPartial ext_wave(EnsPartial a)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        EnsPartial b;
        b.min = __shfl_xor(a.min, d, 64);
        b.max = __shfl_xor(a.max, d, 64);
        b.nonfinite = __shfl_xor(a.nonfinite, d, 64);
        b.count = __shfl_xor(a.count, d, 64);
        ext_fold(a, b);
    }
    return a;
}

// grid: (tiles of all blocks, members); tab[member * nblk + block] names the member's field and lu there
__global__ __launch_bounds__(64) void k_ens_extrema(const EnsExtBlock *__restrict__ blk, int nblk,
                                                    const EnsExtSrc *__restrict__ tab, EnsPartial *__restrict__ part)
{
    const int t = (int)blockIdx.x, m = (int)blockIdx.y;
    int k = 0;
    while (k + 1 < nblk && t >= blk[k + 1].first_tile) ++k;
    const EnsExtBlock g = blk[k];
    const EnsExtSrc q = tab[(long)m * nblk + k];
    const int lt = t - g.first_tile, tx = lt % g.tiles_x, ty = lt / g.tiles_x;
    const int i = tx * 64 + (int)threadIdx.x;
    EnsPartial a{__builtin_inf(), -__builtin_inf(), 0, 0};
    if (i < g.w) {
        // every row's loads first (a row past the block's end reads the last row again and is not
        // counted; land is read and not counted): no load waits for a branch on an earlier one
        float l[kExtremaRows];
        double v[kExtremaRows];
#pragma unroll
        for (int r = 0; r < kExtremaRows; ++r) {
            const int j = ty * kExtremaRows + r;
            const long at = g.off + (long)(j < g.h ? j : g.h - 1) * g.pitch + i;
            l[r] = q.lu[at];
            v[r] = q.src[at];
        }
#pragma unroll
        for (int r = 0; r < kExtremaRows; ++r) {
            if (ty * kExtremaRows + r >= g.h || fabsf(l[r]) < 0.5f) continue;
            a.count += 1;
            if (__builtin_isfinite(v[r])) {
                a.min = v[r] < a.min ? v[r] : a.min;
                a.max = v[r] > a.max ? v[r] : a.max;
            } else {
                a.nonfinite += 1;
            }
        }
    }
    a = ext_wave(a);
    if (threadIdx.x == 0) part[(long)m * gridDim.x + t] = a;
}

// one wave per member: its ntiles partials into out[member]
__global__ __launch_bounds__(64) void k_ens_extrema_final(const EnsPartial *__restrict__ part, int ntiles,
                                                          EnsPartial *__restrict__ out)
{
    const int m = (int)blockIdx.x;
    EnsPartial a{__builtin_inf(), -__builtin_inf(), 0, 0};
    for (int t = (int)threadIdx.x; t < ntiles; t += 64) ext_fold(a, part[(long)m * ntiles + t]);
    a = ext_wave(a);
    if (threadIdx.x == 0) out[m] = a;
}

int ens_extrema_tiles(int w, int h, int *tiles_x)
{
    const int tx = (w + 63) / 64, ty = (h + kExtremaRows - 1) / kExtremaRows;
    if (tiles_x) *tiles_x = tx;
    return w > 0 && h > 0 ? tx * ty : 0;
}

int launch_ens_extrema(const EnsExtBlock *d_blk, int nblk, const EnsExtSrc *d_tab, int members, int ntiles,
                       EnsPartial *d_part, EnsPartial *d_out, hipStream_t s)
{
    if (members < 1 || members > OCN_ENS_MAX_MEMBERS || nblk < 1 || ntiles < 1)
        return set_error(OCN_ERR_ARG, "ens_extrema: nothing to reduce");
    hipLaunchKernelGGL(k_ens_extrema, dim3((unsigned)ntiles, (unsigned)members), dim3(64), 0, s, d_blk, nblk, d_tab,
                       d_part);
    if (const int rc = check_launch()) return rc;
    hipLaunchKernelGGL(k_ens_extrema_final, dim3((unsigned)members), dim3(64), 0, s, d_part, ntiles, d_out);
    return check_launch();
}

}  // namespace ocn
