// ens_local.hip -- the localized serial observation update of an ensemble (ocn_sw.h ocn_ens_local_update).
//
// k_ens_local: per point (i, j) -- global indices -- of one real(8) field of one block, with x_m the value
// of the m-th member in use, over the block's observation list in ascending order:
//   d2 = (i-io)^2 + (j-jo)^2;  d2 >= ntaper: skip;  rho = taper[d2];  rho +-0.0: skip
//   s = x_0;  s = s + x_m (m = 1 .. n-1);  mean = s / (double)n
//   a = (x_0 - mean) y[k][0];  p = (x_m - mean) y[k][m], a = a + p (m = 1 .. n-1);  g = rho a
//   x_m = x_m + g z[k][m]  for every m
// (-ffp-contract=off, Makefile: every product rounded, then the sum -- the bits of tests/ens_local_ref.py).
// A skipped observation forms nothing; a point no observation reaches is neither loaded for nor stored.
// Layout as k_ens_transform: one point per lane, lanes along x, a wave's first lane on a 256-B line
// (lead); the members' base pointers by value in the kernel arguments, indexed uniformly.  The block's
// list (the observations whose box [io-R, io+R] x [jo-R, jo+R] meets the block's array, R the largest r
// with r^2 < ntaper, in the caller's order, padded to groups of kLuGroup with entries no wave accepts) and
// the y and z rows (kLuRow-padded) are read through the constant address space with uniform indices:
// scalar loads, a group of list entries and 8 row values at a time.  An observation whose box misses the
// wave's row or its span of columns is rejected on scalar compares before any vector work; the per-lane
// skip inside a reached wave is a divergent branch, so an unreached lane keeps its bits.  The first
// observation a wave accepts loads the lanes' n values; only touched lanes store, once, at the end.  In
// place is safe: a lane reads and writes its own point only.  The tails of the member loops beyond n are
// wave-uniform branches, never padded zero terms (s + 0 changes a -0).
//   REG  (n <= kEnsStatsReg): the n values in registers, 256 threads per workgroup.
//   !REG (beyond): the values in LDS as [member][lane] (lane-consecutive doubles: no bank conflict), one
//        wave per workgroup, n x 512 B of dynamic LDS.  The same operations in the same order: the same bits.
//        Up to 128 members that is at most 64 KiB and launches as it stands; 129 .. 256 members need 66 048 B ..
//        128 KiB of gfx950's 160 KiB, which a kernel gets only after hipFuncSetAttribute(...,
//        hipFuncAttributeMaxDynamicSharedMemorySize, bytes) -- the launcher sets it per call beyond 64 KiB, and a
//        refusal is OCN_ERR_HIP, nothing launched.  Observed on the MI355X: the attribute is granted and the kernel
//        launches at 129, 255 and 256 members (tests/test_gpu_ens_large.py, bitwise; one such workgroup fits a CU).
// No atomics, no inline assembly.
#include "ocn_internal.h"

namespace ocn {

struct EnsLuPtrs { double *p[OCN_ENS_MAX_MEMBERS]; };

typedef const __attribute__((address_space(4))) double *LuRow;
typedef const __attribute__((address_space(4))) int *LuList;   // EnsLuObs as its four ints

extern __shared__ double ens_local_lds[];

// BODY for m = 0 .. n-1 in groups of 8: a full group straight through, the last one behind uniform
// branches.  REG: unrolled over kEnsStatsReg, so that every index into the lane's values is a constant and
// they stay in registers (a macro, not a functor: nothing here may be left to the inliner).
#define LU_GROUP_(BODY)                                      \
    if (g_ + 8 <= n) {                                       \
        _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) {   \
            const int m = g_ + e_;                           \
            BODY                                             \
        }                                                    \
    } else {                                                 \
        _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) {   \
            const int m = g_ + e_;                           \
            if (m < n) { BODY }                              \
        }                                                    \
    }
#define LU_MEMBERS(BODY)                                                    \
    if constexpr (REG) {                                                    \
        _Pragma("unroll") for (int g_ = 0; g_ < kEnsStatsReg; g_ += 8) {    \
            if (g_ >= n) break;                                             \
            LU_GROUP_(BODY)                                                 \
        }                                                                   \
    } else {                                                                \
        for (int g_ = 0; g_ < n; g_ += 8) { LU_GROUP_(BODY) }               \
    }
// member m's value of this lane: a register, or its LDS word
#define LU_X(m) (*lu_x<REG>(x, col, (m)))
template <bool REG, int N>
__device__ __forceinline__ double *lu_x(double (&x)[N], double *col, int m)
{
    if constexpr (REG) return &x[m];
    else return &col[m * 64];
}

template <bool REG>
__global__ __launch_bounds__(REG ? 256 : 64) void k_ens_local(const EnsLuPtrs mem, const EnsLuObs *list_, int ngroups,
                                                              const double *y_, const double *z_,
                                                              const double *__restrict__ taper, int ntaper, int reach,
                                                              int n, int w, int h, long pitch, int lead, int gx0, int gy0)
{
    // the wave's row and its span of columns, known to be uniform
    const int wave = REG ? __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) : 0;
    const int lane = (int)threadIdx.x & 63;
    const int i0 = (int)blockIdx.x * (REG ? 256 : 64) + wave * 64 - lead, j = (int)blockIdx.y;
    const int ia = i0 < 0 ? 0 : i0, ib = i0 + 63 < w - 1 ? i0 + 63 : w - 1;
    if (ia > ib || j >= h) return;
    const int i = i0 + lane;
    const bool valid = i >= 0 && i < w;
    const long at = (long)j * pitch + i;
    const int gi = gx0 + i, gj = gy0 + j, ga = gx0 + ia, gb = gx0 + ib;
    const LuList list = (LuList)(uintptr_t)list_;
    const LuRow y = (LuRow)(uintptr_t)y_, z = (LuRow)(uintptr_t)z_;
    const long row = (long)((n + kLuRow - 1) / kLuRow) * kLuRow;
    const double dn = (double)n;

    double x[REG ? kEnsStatsReg : 1];
    double *const col = ens_local_lds + lane;   // !REG: member m's value at col[m * 64]
    if constexpr (REG) {
#pragma unroll
        for (int m = 0; m < kEnsStatsReg; ++m) x[m] = 0.0;
    }
    bool loaded = false, touched = false;

    for (int q = 0; q < ngroups; ++q) {
        EnsLuObs o[kLuGroup];
        unsigned pass = 0u;
#pragma unroll
        for (int e = 0; e < kLuGroup; ++e) {
            const LuList at_e = list + (long)(q * kLuGroup + e) * 4;
            o[e] = EnsLuObs{at_e[0], at_e[1], at_e[2], 0};
            const bool miss = o[e].jo - reach > gj || o[e].jo + reach < gj || o[e].io - reach > gb || o[e].io + reach < ga;
            pass |= miss ? 0u : 1u << e;
        }
        while (pass) {
            const int e = __builtin_ctz(pass);
            pass &= pass - 1u;
            int io = o[0].io, jo = o[0].jo, k = o[0].k;
#pragma unroll
            for (int t = 1; t < kLuGroup; ++t)
                if (e == t) { io = o[t].io; jo = o[t].jo; k = o[t].k; }
            if (!loaded) {   // the first observation that reaches the wave
                loaded = true;
                if (valid) { LU_MEMBERS(LU_X(m) = mem.p[m][at];) }
            }
            // (|di| <= reach + 63 and |dj| <= reach with reach <= 255: no overflow)
            const int di = gi - io, dj = gj - jo, d2 = di * di + dj * dj;
            const bool within = valid && d2 < ntaper;
            double rho = 0.0;
            if (within) rho = taper[d2];
            if (rho != 0.0) {   // (not: out of reach, or +0.0 / -0.0 in the table, whose entries are finite)
                touched = true;
                const LuRow yk = y + (long)k * row, zk = z + (long)k * row;
                double s = 0.0;
                LU_MEMBERS(s = m == 0 ? LU_X(0) : s + LU_X(m);)
                const double mean = s / dn;
                double a = 0.0;
                LU_MEMBERS(const double p = (LU_X(m) - mean) * yk[m]; a = m == 0 ? p : a + p;)
                const double g = rho * a;
                LU_MEMBERS(LU_X(m) = LU_X(m) + g * zk[m];)
            }
        }
    }
    if (touched) { LU_MEMBERS(mem.p[m][at] = LU_X(m);) }
}

int launch_ens_local(const ocn_block *b, double *const *mem, int n, const EnsLuObs *d_list, int ngroups, const double *d_y,
                     const double *d_z, const double *d_taper, int ntaper, int reach, hipStream_t s)
{
    if (n < 2 || n > OCN_ENS_MAX_MEMBERS || !d_list || !d_y || !d_z || !d_taper || ngroups < 1 || ntaper < 1 ||
        reach < 0 || reach > 255)
        return set_error(OCN_ERR_ARG, "ens_local: member count, tables or reach");
    EnsLuPtrs p;
    for (int i = 0; i < OCN_ENS_MAX_MEMBERS; ++i) p.p[i] = mem[i < n ? i : 0];
    const int w = b->bnd_x2 - b->bnd_x1 + 1, h = b->bnd_y2 - b->bnd_y1 + 1;
    const int lead = (int)(((uintptr_t)mem[0] & 255u) / 8u);   // (as launch_ens_transform)
    if (n <= kEnsStatsReg) {
        const dim3 grid((unsigned)((w + lead + 255) / 256), (unsigned)h);
        hipLaunchKernelGGL(k_ens_local<true>, grid, dim3(256), 0, s, p, d_list, ngroups, d_y, d_z, d_taper, ntaper, reach,
                           n, w, h, (long)b->pitch, lead, (int)b->bnd_x1, (int)b->bnd_y1);
        return check_launch();
    }
    const size_t lds = (size_t)n * 64 * sizeof(double);
    // (beyond 64 KiB a kernel has to be allowed its dynamic LDS; gfx950 gives one workgroup up to 160 KiB)
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void *)k_ens_local<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds) != hipSuccess)
        return set_error(OCN_ERR_HIP, "ens_local: the LDS of this many members");
    const dim3 grid((unsigned)((w + lead + 63) / 64), (unsigned)h);
    hipLaunchKernelGGL(k_ens_local<false>, grid, dim3(64), lds, s, p, d_list, ngroups, d_y, d_z, d_taper, ntaper, reach, n,
                       w, h, (long)b->pitch, lead, (int)b->bnd_x1, (int)b->bnd_y1);
    return check_launch();
}

}  // namespace ocn
