// ens_transform.hip -- recombining the members of an ensemble and sampling them at points (ocn_sw.h
// ocn_ens_transform, ocn_ens_sample).
//
// k_ens_transform: per point of one real(8) field of one block, with x_a the value of the a-th member in
// use and w[a][b] the weight of old member a in new member b:
//   new_b = +0.0 if column b keeps no term; otherwise over a ascending, skipping every a whose w[a][b] is
//   +-0.0:  first kept term s = x_a w[a][b];  later kept terms p = x_a w[a][b], s = s + p
// (-ffp-contract=off, Makefile: the product rounded, then the sum -- the bits of tests/ens_transform_ref.py).
// A skipped term is not formed, so a unit column copies bit for bit and a member with an all-zero row
// reaches no other member, whatever it holds.  The accumulator starts at -0.0, the identity of IEEE
// addition in round-to-nearest (-0.0 + p has p's bits for every p that is not a NaN, -0.0 + -0.0 = -0.0),
// so the first kept term needs no case of its own; a column that keeps none stores +0.0.
// Layout as k_ens_stats: one point per lane, lanes along x, a wave's first lane on a 256-B line (lead);
// the members' base pointers by value in the kernel arguments, indexed uniformly.  The weights lie on the
// device in the order the kernels read them (ocn_internal.h ens_wt_index: REG a column's weights side by
// side, zero-padded to kEnsStatsReg; !REG one input's weights for a pass's 8 columns side by side) and are
// read through the constant address space: scalar loads of 8 weights at a time, and the zero test is an
// integer test of the weight's bit pattern, the same for every lane of a wave: a branch, not a select.  A
// group of 8 weights with no zero among them runs straight through, without a branch per term.
//   REG  (n <= kEnsStatsReg): a lane loads its n values (8 members' loads in flight ahead), keeps them in
//        registers and stores column after column into the members' own arrays.  In place is safe: a lane
//        has all its inputs before its first store and no other lane reads its point.
//   !REG (beyond): 8 columns' accumulators per pass over the n inputs, the results into staging arrays
//        (member b's at stage + b * stage_stride), which k_ens_unstage copies back.  The same operations
//        in the same order as REG, so the same bits.
// No atomics, no LDS.
//
// k_ens_sample: one thread per (point, member), the point's offset (and block) from a device table.
#include "ocn_internal.h"

namespace ocn {

constexpr int kXfAhead = 8;   // members whose loads are in flight before their use
constexpr int kXfCols = 8;    // !REG: output columns per pass over the inputs

struct EnsXfPtrs { double *p[OCN_ENS_MAX_MEMBERS]; };

typedef const __attribute__((address_space(4))) unsigned long long *WeightBits;

// the weight's bits; kept: anything but +0.0 / -0.0
__device__ __forceinline__ bool xf_kept(unsigned long long bits) { return (bits << 1) != 0ull; }
// The skip of a zero weight must stay a branch on a scalar condition, so that the term is not even
// formed; marked as the likely way, the compiler does not turn the two operations behind it into selects.
#define XF_SKIP(bits) __builtin_expect(!xf_kept(bits), 1)
// a group of 8 weights none of which is zero takes a straight path with no branch per term (the same
// operations in the same order); the dense matrices of a filter's analysis are all such groups
__device__ __forceinline__ bool xf_all_kept(const unsigned long long (&b)[8])
{
    bool all = true;
#pragma unroll
    for (int e = 0; e < 8; ++e) all = all && xf_kept(b[e]);
    return all;
}

template <bool REG>
__global__ __launch_bounds__(256) void k_ens_transform(const EnsXfPtrs mem, const double *wt_, int n, int w, int h,
                                                       long pitch, int lead, double *stage, long stage_stride)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - lead, j = (int)blockIdx.y;
    if (i < 0 || i >= w || j >= h) return;
    const long at = (long)j * pitch + i;
    const WeightBits wt = (WeightBits)(uintptr_t)wt_;
    if constexpr (REG) {
        double x[kEnsStatsReg];
#pragma unroll
        for (int g = 0; g < kEnsStatsReg; g += kXfAhead) {
#pragma unroll
            for (int e = 0; e < kXfAhead; ++e) x[g + e] = 0.0;
            if (g < n) {   // (the table's entries beyond n name member 0: read, never used)
#pragma unroll
                for (int e = 0; e < kXfAhead; ++e) x[g + e] = mem.p[g + e][at];
            }
        }
        for (int b = 0; b < n; ++b) {
            const WeightBits col = wt + (long)b * kEnsStatsReg;   // (zero beyond n: skipped)
            double s = -0.0;
            unsigned long long any = 0ull;
#pragma unroll
            for (int g = 0; g < kEnsStatsReg; g += kXfAhead) {
                if (g >= n) break;
                unsigned long long bits[kXfAhead];
#pragma unroll
                for (int e = 0; e < kXfAhead; ++e) bits[e] = col[g + e];
                if (xf_all_kept(bits)) {   // a dense group: straight through
#pragma unroll
                    for (int e = 0; e < kXfAhead; ++e) s = s + x[g + e] * __longlong_as_double((long long)bits[e]);
                    any |= bits[0];
                    continue;
                }
#pragma unroll
                for (int e = 0; e < kXfAhead; ++e) {
                    if (XF_SKIP(bits[e])) continue;
                    s = s + x[g + e] * __longlong_as_double((long long)bits[e]);
                    any |= bits[e];
                }
            }
            mem.p[b][at] = xf_kept(any) ? s : 0.0;
        }
    } else {
        for (int b0 = 0; b0 < n; b0 += kXfCols) {   // (the columns are padded to a multiple of kXfCols)
            double acc[kXfCols];
#pragma unroll
            for (int c = 0; c < kXfCols; ++c) acc[c] = -0.0;
            unsigned long long any[kXfCols] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
            const WeightBits row = wt + (long)b0 * n;   // this pass's weights: input a's kXfCols side by side
            for (int g = 0; g < n; g += kXfAhead) {
                double v[kXfAhead];
#pragma unroll
                for (int e = 0; e < kXfAhead; ++e) v[e] = mem.p[g + e][at];   // (beyond n: member 0, never used)
#pragma unroll
                for (int e = 0; e < kXfAhead; ++e) {
                    if (g + e >= n) break;
                    unsigned long long bits[kXfCols];
#pragma unroll
                    for (int c = 0; c < kXfCols; ++c) bits[c] = row[(long)(g + e) * kXfCols + c];
                    if (xf_all_kept(bits)) {   // a dense group: straight through
#pragma unroll
                        for (int c = 0; c < kXfCols; ++c) {
                            acc[c] = acc[c] + v[e] * __longlong_as_double((long long)bits[c]);
                            any[c] |= bits[c];
                        }
                        continue;
                    }
#pragma unroll
                    for (int c = 0; c < kXfCols; ++c) {
                        if (XF_SKIP(bits[c])) continue;
                        acc[c] = acc[c] + v[e] * __longlong_as_double((long long)bits[c]);
                        any[c] |= bits[c];
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < kXfCols; ++c)
                if (b0 + c < n) stage[(long)(b0 + c) * stage_stride + at] = xf_kept(any[c]) ? acc[c] : 0.0;
        }
    }
}

// grid.z: the member; its staging array back into its own array
__global__ __launch_bounds__(256) void k_ens_unstage(const EnsXfPtrs mem, int w, int h, long pitch, int lead,
                                                     const double *stage, long stage_stride)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - lead, j = (int)blockIdx.y, b = (int)blockIdx.z;
    if (i < 0 || i >= w || j >= h) return;
    const long at = (long)j * pitch + i;
    mem.p[b][at] = stage[(long)b * stage_stride + at];
}

int launch_ens_transform(const ocn_block *b, double *const *mem, int n, const double *d_wt, double *stage,
                         long stage_stride, hipStream_t s)
{
    if (n < 1 || n > OCN_ENS_MAX_MEMBERS || !d_wt || (n > kEnsStatsReg && !stage))
        return set_error(OCN_ERR_ARG, "ens_transform: member count, weights or staging");
    EnsXfPtrs p;
    for (int i = 0; i < OCN_ENS_MAX_MEMBERS; ++i) p.p[i] = mem[i < n ? i : 0];
    const int w = b->bnd_x2 - b->bnd_x1 + 1, h = b->bnd_y2 - b->bnd_y1 + 1;
    // the lane of the first member's A(bnd_x1, :) within its 256-B line (a member based otherwise is
    // still indexed correctly: the shift only aligns the waves)
    const int lead = (int)(((uintptr_t)mem[0] & 255u) / 8u);
    const dim3 grid((unsigned)((w + lead + 255) / 256), (unsigned)h);
    if (n <= kEnsStatsReg) {
        hipLaunchKernelGGL(k_ens_transform<true>, grid, dim3(256), 0, s, p, d_wt, n, w, h, (long)b->pitch, lead,
                           (double *)nullptr, 0L);
        return check_launch();
    }
    hipLaunchKernelGGL(k_ens_transform<false>, grid, dim3(256), 0, s, p, d_wt, n, w, h, (long)b->pitch, lead, stage,
                       stage_stride);
    if (const int rc = check_launch()) return rc;
    hipLaunchKernelGGL(k_ens_unstage, dim3(grid.x, grid.y, (unsigned)n), dim3(256), 0, s, p, w, h, (long)b->pitch,
                       lead, (const double *)stage, stage_stride);
    return check_launch();
}

// ------------------------------------------------------------------ sampling at points
// grid: (points / 256, members); tab (several blocks only): member m's array of block k at tab[k * n + m]
__global__ __launch_bounds__(256) void k_ens_sample(const EnsXfPtrs mem, const double *const *__restrict__ tab, int n,
                                                    const long *__restrict__ off, const int *__restrict__ blk,
                                                    int npts, double *__restrict__ out)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x), m = (int)blockIdx.y;
    if (p >= npts) return;
    const double *a = tab ? tab[(long)blk[p] * n + m] : mem.p[m];
    out[(long)p * n + m] = a[off[p]];
}

int launch_ens_sample(const double *const *mem, const double *const *d_tab, int n, const long *d_off,
                      const int *d_blk, int npts, double *d_out, hipStream_t s)
{
    if (n < 1 || n > OCN_ENS_MAX_MEMBERS || npts < 1) return set_error(OCN_ERR_ARG, "ens_sample: nothing to gather");
    EnsXfPtrs p;
    for (int i = 0; i < OCN_ENS_MAX_MEMBERS; ++i) p.p[i] = (double *)mem[i < n ? i : 0];
    hipLaunchKernelGGL(k_ens_sample, dim3((unsigned)((npts + 255) / 256), (unsigned)n), dim3(256), 0, s, p, d_tab, n,
                       d_off, d_blk, npts, d_out);
    return check_launch();
}

}  // namespace ocn
