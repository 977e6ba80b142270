// ens_perturb.hip -- correlated random perturbations of an ensemble's members (ocn_sw.h ocn_ens_perturb).
//
// k_ens_noise: Z_m = B_y^P B_x^P W_m of one block for the n members in use (blockIdx.z), into the ensemble's
// int64 scratch (member a's array zstride elements after member a-1's, based like the members' arrays).
//   W_m(i, j) = S - 262140, S the sum of the eight 16-bit halves of
//               Philox4x32-10((uint32)i, (uint32)j, u_m, draw; seed & 0xffffffff, seed >> 32)
//   (B_x Z)(i, j) = the sum over d = -R .. R of Z(i + d, j), a box SUM
// Integer arithmetic throughout: tiles, pass order and the order of the sums cannot change a bit.
//   A workgroup (4 waves) owns kNoiseCols = 64 columns -- a wave's first lane on a 256-B line of the scratch
//   (lead), as k_ens_stats -- and th = min(kNoiseRows - 2 A, kNoiseTile) rows, A = R P the apron: 32 rows,
//   which is all the largest apron, 48, leaves of the column buffer; taller tiles at smaller aprons draw less
//   noise twice but leave a basin of the Black Sea's size with too few workgroups (OCN_ENS_NOISE_TILE=128
//   builds them for measurements: DESIGN 7).  Stage 1, a row per wave at a time: the row of W widened by
//   the apron, 64 + 2 A points, Philox in registers, into the wave's LDS row buffer; P times the direct box
//   sum from one row buffer into the other, R points shorter at either end each time; the last result, 64
//   points, into the LDS column buffer.  Stage 2, P times: each of the 64 columns runs down the column
//   buffer in place with a running sum (ascending rows: a row is overwritten only after every sum that reads
//   it), 2 R rows shorter each time; 16 columns per wave, so that the four SIMDs share them.  Stage 3: the th
//   rows that are left go to the scratch, a row per wave at a time.  The stages and the x-passes are
//   separated by workgroup barriers in uniform loops.
//   LDS: the column buffer kNoiseRows x 64 x 8 B = 65536 B and 4 x 2 row buffers of 160 x 8 B = 10240 B,
//   75776 B static: two workgroups per CU, no dynamic LDS.
// k_ens_perturb_apply: per point of one real(8) field of one block, k_ens_inflate's layout and 64 x 4 geometry,
// the members' pointers by value:
//   T = the sum over the members in use of Z (centre);  D_m = n Z_m - T (centre), Z_m (not)       (int64)
//   where the mask applies (none, or member 0's mask > 0.5f):  d = (double)D_m;  p = c * d;  x_m = x_m + p
// (-ffp-contract=off, Makefile: the bits of ocean_model_arch_amd/ens_perturb_rule.py).  Elsewhere the point is
// not stored to.  The members go in groups of 8 whose loads are issued ahead of the stores.
// No atomics, no inline assembly.
#include "ocn_internal.h"

#ifndef OCN_ENS_NOISE_TILE
#define OCN_ENS_NOISE_TILE 32
#endif

namespace ocn {

constexpr int kNoiseCols = 64;                                  // output columns of a workgroup: one wave wide
constexpr int kNoiseRows = 128;                                 // rows of the column buffer: th + 2 A
constexpr int kNoiseTile = OCN_ENS_NOISE_TILE;                  // the most output rows of a workgroup
constexpr int kNoiseApron = OCN_ENS_PERTURB_MAX_REACH * OCN_ENS_PERTURB_MAX_PASSES;
constexpr int kNoiseRowLen = kNoiseCols + 2 * kNoiseApron;      // the widest row of W
static_assert(kNoiseRows > 2 * kNoiseApron && kNoiseTile >= 1, "the largest apron leaves rows to a tile");
static_assert((kNoiseRows * kNoiseCols + 8 * kNoiseRowLen) * 8 <= 160 * 1024 / 2, "two workgroups per CU");

struct EnsPertPtrs { double *p[OCN_ENS_MAX_MEMBERS]; };         // the members' arrays, by value (as k_ens_inflate's)
struct EnsNoiseIdx { uint8_t u[OCN_ENS_MAX_MEMBERS]; };         // the members in use: their indices in the ensemble

__device__ __forceinline__ long long philox_w(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (unsigned)p1; c2 = n2; c3 = (unsigned)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const unsigned s = (c0 & 0xffffu) + (c0 >> 16) + (c1 & 0xffffu) + (c1 >> 16) + (c2 & 0xffffu) + (c2 >> 16) +
                       (c3 & 0xffffu) + (c3 >> 16);
    return (long long)s - 262140ll;
}

__global__ __launch_bounds__(256) void k_ens_noise(const EnsNoiseIdx idx, int w, int h, long pitch, int lead, int gx0, int gy0,
                                                   unsigned draw, unsigned k0, unsigned k1, int R, int P,
                                                   long long *__restrict__ z, long zstride)
{
    __shared__ long long col[kNoiseRows][kNoiseCols];
    __shared__ long long row[4][2][kNoiseRowLen];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int A = R * P, th_max = min(kNoiseRows - 2 * A, kNoiseTile);
    const int x0 = (int)blockIdx.x * kNoiseCols - lead, y0 = (int)blockIdx.y * th_max;   // the tile's first point in the array
    const int th = min(th_max, h - y0), rows = th + 2 * A;
    const unsigned member = idx.u[blockIdx.z];
    // stage 1: row r of the column buffer is array row y0 + r - A, its columns x0 .. x0 + 63
    for (int r0 = 0; r0 < rows; r0 += 4) {
        const int r = r0 + wave;
        const bool live = r < rows;
        int len = kNoiseCols + 2 * A, cur = 0;
        if (live) {
            const unsigned gj = (unsigned)(gy0 + y0 + r - A);
            long long *out = P ? row[wave][0] : col[r];
            for (int t = lane; t < len; t += 64) out[t] = philox_w((unsigned)(gx0 + x0 + t - A), gj, member, draw, k0, k1);
        }
        for (int p = 1; p <= P; ++p) {
            __syncthreads();
            len -= 2 * R;
            if (live) {
                const long long *in = row[wave][cur];
                long long *out = p < P ? row[wave][cur ^ 1] : col[r];
                for (int t = lane; t < len; t += 64) {
                    long long s = in[t];
                    for (int d = 1; d <= 2 * R; ++d) s += in[t + d];
                    out[t] = s;
                }
            }
            cur ^= 1;
        }
        __syncthreads();   // (the row buffers are written again by the next row)
    }
    // stage 2: down the columns, in place
    const int c = wave * 16 + lane;
    for (int p = 1, len = rows; p <= P; ++p) {
        len -= 2 * R;
        if (lane < 16) {
            long long s = 0;
            for (int d = 0; d <= 2 * R; ++d) s += col[d][c];
            for (int r = 0; r < len; ++r) {
                const long long old = col[r][c];
                col[r][c] = s;
                if (r + 1 < len) s += col[r + 1 + 2 * R][c] - old;
            }
        }
        __syncthreads();
    }
    // stage 3: rows 0 .. th - 1 are the tile's
    const int i = x0 + lane;
    if (i < 0 || i >= w) return;
    long long *dst = z + (long)blockIdx.z * zstride;
    for (int r = wave; r < th; r += 4) dst[(long)(y0 + r) * pitch + i] = col[r][lane];
}

constexpr int kPertCols = 64, kPertRows = 4;   // (k_ens_inflate's geometry)

__global__ __launch_bounds__(256) void k_ens_perturb_apply(const EnsPertPtrs mem, int n, int w, int h, long pitch, int lead,
                                                           const long long *__restrict__ z, long zstride, int centre, double c,
                                                           const float *__restrict__ mask)
{
    const int i = (int)(blockIdx.x * kPertCols + threadIdx.x) - lead, j = (int)(blockIdx.y * kPertRows + threadIdx.y);
    if (i < 0 || i >= w || j >= h) return;
    const long at = (long)j * pitch + i;
    if (mask && !(mask[at] > 0.5f)) return;
    long long T = 0;
    if (centre)
        for (int m = 0; m < n; ++m) T += z[(long)m * zstride + at];
    for (int g = 0; g < n; g += 8) {
        double x[8];
        long long D[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (g + e < n) {
                x[e] = mem.p[g + e][at];
                D[e] = z[(long)(g + e) * zstride + at];
            }
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (g + e < n) {
                const double d = (double)(centre ? (long long)n * D[e] - T : D[e]);
                const double p = c * d;
                mem.p[g + e][at] = x[e] + p;
            }
    }
}

int launch_ens_noise(const ocn_block *b, const uint8_t *members, int n, uint64_t seed, uint32_t draw, int reach, int passes,
                     long long *d_z, long zstride, int lead, hipStream_t s)
{
    if (n < 1 || n > OCN_ENS_MAX_MEMBERS || !d_z || reach < 0 || reach > OCN_ENS_PERTURB_MAX_REACH || passes < 0 ||
        passes > OCN_ENS_PERTURB_MAX_PASSES || lead < 0 || lead >= 32)
        return set_error(OCN_ERR_ARG, "ens_noise: member count, reach, passes or buffer");
    EnsNoiseIdx idx;
    for (int i = 0; i < OCN_ENS_MAX_MEMBERS; ++i) idx.u[i] = members[i < n ? i : 0];
    if (reach == 0 || passes == 0) reach = passes = 0;   // Z = W
    const int w = b->bnd_x2 - b->bnd_x1 + 1, h = b->bnd_y2 - b->bnd_y1 + 1;
    const int th = std::min(kNoiseRows - 2 * reach * passes, kNoiseTile);
    const dim3 grid((unsigned)((w + lead + kNoiseCols - 1) / kNoiseCols), (unsigned)((h + th - 1) / th), (unsigned)n);
    hipLaunchKernelGGL(k_ens_noise, grid, dim3(256), 0, s, idx, w, h, (long)b->pitch, lead, (int)b->bnd_x1, (int)b->bnd_y1, draw,
                       (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), reach, passes, d_z, zstride);
    return check_launch();
}

int launch_ens_perturb_apply(const ocn_block *b, double *const *mem, int n, const long long *d_z, long zstride, bool centre,
                             double c, const float *d_mask, hipStream_t s)
{
    if (n < 1 || n > OCN_ENS_MAX_MEMBERS || !d_z) return set_error(OCN_ERR_ARG, "ens_perturb_apply: member count or buffer");
    EnsPertPtrs p;
    for (int i = 0; i < OCN_ENS_MAX_MEMBERS; ++i) p.p[i] = mem[i < n ? i : 0];
    const int w = b->bnd_x2 - b->bnd_x1 + 1, h = b->bnd_y2 - b->bnd_y1 + 1;
    // the lane of A(bnd_x1, :) within its 256-B line (as launch_ens_inflate): the scratch is based like the members
    const int lead = (int)(((uintptr_t)mem[0] & 255u) / 8u);
    for (int i = 0; i < n; ++i)
        if ((int)(((uintptr_t)mem[i] & 255u) / 8u) != lead) return set_error(OCN_ERR_STATE, "ens_perturb: members' layouts differ");
    if ((int)(((uintptr_t)d_z & 255u) / 8u) != lead) return set_error(OCN_ERR_STATE, "ens_perturb: the scratch is not based like the members");
    const dim3 grid((unsigned)((w + lead + kPertCols - 1) / kPertCols), (unsigned)((h + kPertRows - 1) / kPertRows));
    hipLaunchKernelGGL(k_ens_perturb_apply, grid, dim3((unsigned)kPertCols, (unsigned)kPertRows), 0, s, p, n, w, h,
                       (long)b->pitch, lead, d_z, zstride, centre ? 1 : 0, c, d_mask);
    return check_launch();
}

}  // namespace ocn
