// ens_inflate.hip -- covariance inflation of an ensemble, per point (ocn_sw.h ocn_ens_inflate).
//
// k_ens_inflate: per point of one real(8) field of one block, with x_m the value of the m-th member in use
// (member order, n >= 2):
//   s = x_0;  s = s + x_m (m = 1 .. n-1);  mean = s / (double)n
//   d_m = x_m - mean
//   q = d_0 d_0;  p = d_m d_m, q = q + p;  var = q / (double)(n-1);  sa = sqrt(var)
//   CONST:  f = alpha                                   (applies where sa > 0 and sa is finite)
//   RTPS:   sb = the saved spread at the point          (applies where sa > 0, sa finite and sb finite)
//           t = sb - sa;  r = t / sa;  g = alpha r;  f = 1.0 + g
//   where the rule applies and f != 1.0:  p = f d_m;  x_m = mean + p  for every m
// (-ffp-contract=off, IEEE division and sqrt, Makefile: the bits of ocean_model_arch_amd/ens_inflate_rule.py).
// Everywhere else the point is not written and its factor is 1.0; the factor goes to `factor` at every point
// of the array.  Layout as k_ens_stats: one point per lane, lanes along x, a wave's first lane on a 256-B
// line (lead); the members' base pointers by value in the kernel arguments, indexed uniformly; 8 members'
// loads are issued ahead of the ordered operations.  A workgroup is kInfCols columns x kInfRows rows (64 x 4:
// one wave per row; OCN_ENS_INFLATE_ROWS=1 builds the 256 x 1 one for measurements).  The tails of the member
// loops beyond n are wave-uniform branches, never padded zero terms (s + 0 changes a -0).
//   REG  (n <= kEnsStatsReg): the n values stay in registers from the load to the store.
//   !REG (beyond): the members are read again per pass (sum, variance, update): the same operations in the
//        same order, so the same bits.
// In place is safe: a lane reads and writes its own point only.  The stores of an unwritten lane are under a
// divergent branch, so it keeps its bits.  No atomics, no inline assembly, no LDS.
#include "ocn_internal.h"

#ifndef OCN_ENS_INFLATE_ROWS
#define OCN_ENS_INFLATE_ROWS 4
#endif

namespace ocn {

constexpr int kInfRows = OCN_ENS_INFLATE_ROWS;   // rows of a workgroup
constexpr int kInfCols = 256 / kInfRows;         // its columns
static_assert(kInfRows >= 1 && kInfCols * kInfRows == 256 && kInfCols % 64 == 0, "a workgroup is 4 whole waves");

struct EnsInfPtrs { double *p[OCN_ENS_MAX_MEMBERS]; };

// STMT for the members m = g_ .. g_ + 7 below n (e_ = m - g_): a full group straight through, the last one
// behind uniform branches
#define INF_GROUP_(STMT)                                     \
    if (g_ + 8 <= n) {                                       \
        _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) {   \
            const int m = g_ + e_;                           \
            STMT                                             \
        }                                                    \
    } else {                                                 \
        _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) {   \
            const int m = g_ + e_;                           \
            if (m < n) { STMT }                              \
        }                                                    \
    }
// One pass over the members in groups of 8: the group's loads (REG: in the pass that says LOAD only), then
// BODY in member order.  REG: unrolled over kEnsStatsReg, so that every index into x[] is a constant and the
// values stay in registers (a macro, not a functor: nothing here may be left to the inliner).
#define INF_PASS(LOAD, BODY)                                                \
    if constexpr (REG) {                                                    \
        _Pragma("unroll") for (int g_ = 0; g_ < kEnsStatsReg; g_ += 8) {    \
            if (g_ >= n) break;                                             \
            if (LOAD) { INF_GROUP_(INF_X = mem.p[m][at];) }                 \
            INF_GROUP_(BODY)                                                \
        }                                                                   \
    } else {                                                                \
        for (int g_ = 0; g_ < n; g_ += 8) {                                 \
            INF_GROUP_(INF_X = mem.p[m][at];)                               \
            INF_GROUP_(BODY)                                                \
        }                                                                   \
    }
// member m's value of this lane: REG its own register, !REG the group's
#define INF_X x[REG ? m : e_]

template <bool REG>
__global__ __launch_bounds__(256) void k_ens_inflate(const EnsInfPtrs mem, int n, int w, int h, long pitch, int lead,
                                                     int mode, double alpha, const double *__restrict__ spread,
                                                     double *__restrict__ factor)
{
    const int i = (int)(blockIdx.x * kInfCols + threadIdx.x) - lead, j = (int)(blockIdx.y * kInfRows + threadIdx.y);
    if (i < 0 || i >= w || j >= h) return;
    const long at = (long)j * pitch + i;
    double sb = 0.0;
    if (mode == OCN_ENS_INFLATE_RTPS) sb = spread[at];
    double x[REG ? kEnsStatsReg : 8];
    double s = 0.0;
    INF_PASS(true, s = m == 0 ? INF_X : s + INF_X;)
    const double mean = s / (double)n;
    double q = 0.0;
    INF_PASS(false, const double d = INF_X - mean; const double p = d * d; q = m == 0 ? p : q + p;)
    const double var = q / (double)(n - 1);
    const double sa = sqrt(var);
    bool apply = sa > 0.0 && __builtin_isfinite(sa);
    double f = alpha;
    if (mode == OCN_ENS_INFLATE_RTPS) {
        apply = apply && __builtin_isfinite(sb);
        const double t = sb - sa;
        const double r = t / sa;
        const double g = alpha * r;
        f = 1.0 + g;
    }
    apply = apply && f != 1.0;
    factor[at] = apply ? f : 1.0;
    if (apply) {
        INF_PASS(false, const double d = INF_X - mean; const double p = f * d; mem.p[m][at] = mean + p;)
    }
}

int launch_ens_inflate(const ocn_block *b, double *const *mem, int n, int mode, double alpha, const double *d_spread,
                       double *d_factor, hipStream_t s)
{
    if (n < 2 || n > OCN_ENS_MAX_MEMBERS || !d_factor || (mode != OCN_ENS_INFLATE_CONST && mode != OCN_ENS_INFLATE_RTPS) ||
        (mode == OCN_ENS_INFLATE_RTPS && !d_spread))
        return set_error(OCN_ERR_ARG, "ens_inflate: member count, mode or buffers");
    EnsInfPtrs p;
    for (int i = 0; i < OCN_ENS_MAX_MEMBERS; ++i) p.p[i] = mem[i < n ? i : 0];
    const int w = b->bnd_x2 - b->bnd_x1 + 1, h = b->bnd_y2 - b->bnd_y1 + 1;
    // the lane of A(bnd_x1, :) within its 256-B line (as launch_ens_stats): the buffers are based like the members
    const int lead = (int)(((uintptr_t)mem[0] & 255u) / 8u);
    for (int i = 0; i < n; ++i)
        if ((int)(((uintptr_t)mem[i] & 255u) / 8u) != lead) return set_error(OCN_ERR_STATE, "ens_inflate: members' layouts differ");
    const dim3 grid((unsigned)((w + lead + kInfCols - 1) / kInfCols), (unsigned)((h + kInfRows - 1) / kInfRows));
    const dim3 block((unsigned)kInfCols, (unsigned)kInfRows);
    if (n <= kEnsStatsReg)
        hipLaunchKernelGGL(k_ens_inflate<true>, grid, block, 0, s, p, n, w, h, (long)b->pitch, lead, mode, alpha, d_spread,
                           d_factor);
    else
        hipLaunchKernelGGL(k_ens_inflate<false>, grid, block, 0, s, p, n, w, h, (long)b->pitch, lead, mode, alpha, d_spread,
                           d_factor);
    return check_launch();
}

}  // namespace ocn
