// ens_assim.hip -- the observation-space loop of the serial ensemble square-root filter on the device
// (ocn_sw.h ocn_ens_assimilate): from the members' arrays to the rows Y and Z that k_ens_local reads.
//
// k_ens_obs_space: ONE launch of ONE workgroup of kAsThreads threads.  The dependency is serial
// (observation k reads what observations 0 .. k-1 left at its point), so the work of one observation is
// spread over the threads and the observations follow each other behind workgroup barriers.
//   prologue  hx[j][m] = element off[j] of tab[blk[j] * n + m] (member u_m's array of the block that holds
//             observation j), gathered by all threads; the padding of the hx, Y and Z rows is written +0.0
//             (k_ens_local reads it and never uses it); prior[j] = SPREAD(hx[j]).
//   loop      k ascending, x = the CURRENT row hx[k]:
//               s1 = x_0; s1 = s1 + x_m;  ybar = s1 / (double)n;  y'_m = x_m - ybar
//               q = y'_0 y'_0; p = y'_m y'_m, q = q + p;  s = q / (double)(n-1)
//               D = s + r_k;  d = value_k - ybar;  t = r_k / D;  alpha = 1.0 / (1.0 + sqrt(t));  c = (double)(n-1) D
//               Y[k][m] = y'_m;  Z[k][m] = (d - alpha y'_m) / c;  innovation[k] = d
//             thread m copies x_m into LDS; barrier; every lane forms ybar .. c from that copy of row k (the
//             same address in every lane, the operations ordered: the same bits in every lane, no
//             broadcast); thread m forms and stores Y[k][m] and Z[k][m], to the rows' table and to LDS -- the
//             n divisions side by side, not one after another in every lane.  Barrier.  Row j belongs to
//             thread j mod kAsThreads; its thread takes observation k by k_ens_local's rule with
//             rho = taper[(io[j]-io[k])^2 + (jo[j]-jo[k])^2], after integer compares on |io[j]-io[k]| and
//             |jo[j]-jo[k]| against `reach` have rejected what is out of range, reading Y[k] and Z[k] from
//             LDS.  Barrier.
//             THREE barriers per observation: after the copy of row k (2 n dependent additions on loads
//             that each wait for L2 were about half of the kernel's time; from LDS they are not), after Y[k] and
//             Z[k] (which also keeps the owner of row k from updating it while another wave still reads it),
//             and after the rows' update, which publishes them to the next observation.  (One barrier
//             would have every lane form the n quotients of Z[k] for itself.)
//   epilogue  posterior[j] = SPREAD(final hx[j]);  *nonfinite = the observations whose D or d was not finite.
// SPREAD is ens_stats.hip's: ordered sum, / (double)n, d = x - mean, q = d0 d0, q = q + d d, / (double)(n-1),
// sqrt.  -ffp-contract=off and IEEE division / sqrt (Makefile): the bits of
// ens_local_rule.ensrf_obs_space_ordered.  Member loops run to n, never over padded zero terms (s + 0 turns
// a -0.0 sum into +0.0).  The rows live in the ensemble's table in global memory (L2-resident: 8192 rows of
// 256 members are 16 MiB at most, a test's a few KiB), ens_lu_row(n) doubles apart, the layout k_ens_local
// reads Y and Z in; a thread streams its row through registers kAsChunk members at a time behind constant
// indices, so nothing goes to scratch, and there is ONE path for every n and nobs.
// No atomics, no grid barrier, no inline assembly; plain stores.
//
// A sparse linear observation operator (ocn_sw.h ocn_ens_sample_h, ocn_ens_assimilate_h): obs_apply forms
// H_j(member u_m) from a CSR table of terms; k_ens_sample_h brings it down, one thread per (observation,
// member); k_ens_obs_space_h is k_ens_obs_space with hx[j][m] = H_j(member u_m) in the prologue -- the two
// are instances of one body, as_stage, and still ONE launch of ONE workgroup each.
//
// Observations at their own times (ocn_sw.h ocn_ens_record_sample, ocn_ens_assimilate_rec): rec_interp forms hx
// from the station recorder's series, one gather in time; k_ens_record_sample brings it down, one thread per
// (observation, member) with the member fastest; k_ens_obs_space_r is the third instance of as_stage.
//
// Quality control against the background (ocn_sw.h ocn_ens_set_gate): k_ens_obs_space_g, _hg and _rg are the three
// instances with as_stage's kGate -- an observation whose squared innovation exceeds gate2 D, or whose D or d is
// not finite, forms nothing; still ONE launch of ONE workgroup each (see as_stage).
#include "ocn_internal.h"

namespace ocn {

// SPREAD of the n values at x
__device__ __forceinline__ double as_spread(const double *x, int n)
{
    double s = x[0];
    for (int m = 1; m < n; ++m) s = s + x[m];
    const double mean = s / (double)n;
    const double d0 = x[0] - mean;
    double q = d0 * d0;
    for (int m = 1; m < n; ++m) {
        const double d = x[m] - mean;
        q = q + d * d;
    }
    return sqrt(q / (double)(n - 1));
}

// members of a row in flight per thread (32 gained nothing at 64 members and lost half at 8: 256 VGPRs)
constexpr int kAsChunk = 8;
static_assert(kAsChunk == kLuRow, "a chunk's loads may run into the row's padding, never beyond it");
static_assert(OCN_ENS_MAX_MEMBERS % kAsChunk == 0, "... nor beyond the LDS copy of row k");

// ------------------------------------------------------------------ a sparse linear observation operator
// H_j(member u_m): s = x_0 * w_0, then p = x_t * w_t; s = s + p in the caller's term order, every product
// rounded before the sum (-ffp-contract=off).  ONE function for the sample and for the filter's prologue:
// the same bits from both.  A group's loads go out together (a term's value hangs on two dependent loads:
// the table's pointer, then the element), the ordered multiply-adds follow behind constant indices: no
// scratch.  The loop runs to the row's term count, never over padding (s + 0 turns a -0.0 sum into +0.0).
constexpr int kObsGroup = 4;
static_assert(OCN_ENS_OBS_MAX_TERMS % kObsGroup == 0, "whole groups up to the limit");

__device__ __forceinline__ double obs_apply(const EnsObsOp &h, int j, int m)
{
    const int t0 = h.start[j], t1 = h.start[j + 1];
    double s = 0.0;
    for (int t = t0; t < t1; t += kObsGroup) {
        double x[kObsGroup], w[kObsGroup];
#pragma unroll
        for (int e = 0; e < kObsGroup; ++e)
            if (t + e < t1) {
                const EnsObsTerm q = h.term[t + e];
                x[e] = h.tab[q.slot + m][q.off];
                w[e] = q.w;
            }
#pragma unroll
        for (int e = 0; e < kObsGroup; ++e)
            if (t + e < t1) {
                const double p = x[e] * w[e];
                s = t + e == t0 ? p : s + p;
            }
    }
    return s;
}

// ------------------------------------------------------------------ the recorder's series as the source
// hx[j][m] from the station recorder's series (ocn_sw.h ocn_ens_record_sample): a = the row's value in record
// rec, column col[m]; with wt == 0.0 a itself, bit for bit, and the second load is not issued; else b = the same
// element of record rec + 1, p = b - a; q = wt * p; a + q, every operation rounded (-ffp-contract=off).  ONE
// function for the sample and for the filter's prologue: the same bits from both.
__device__ __forceinline__ double rec_interp(const EnsRecSrc &r, int j, int m)
{
    const EnsRecObs o = r.obs[j];
    const double *at = r.series + (o.off + r.col[m]);
    const double a = at[0];
    if (o.wt == 0.0) return a;
    const double b = at[r.next];
    const double p = b - a;
    const double q = o.wt * p;
    return a + q;
}

// ------------------------------------------------------------------ the observation-space stage
// The whole stage, ONE text for k_ens_obs_space (kSrc kAsPoints: hx gathered at points), k_ens_obs_space_h
// (kAsOperator: hx = the operator h applied to the members) and k_ens_obs_space_r (kAsRecords: hx interpolated in
// the recorder's series r): only the prologue's right-hand side differs.
constexpr int kAsPoints = 0, kAsOperator = 1, kAsRecords = 2;

// kGate (ocn_sw.h ocn_ens_set_gate; k_ens_obs_space_g, _hg, _rg): after D and d of observation k, every lane forms
// lim = gate2 * D (one rounded product) and ok = isfinite(D) && isfinite(d) && d * d <= lim from the same LDS copy of
// row k with the same operations -- the same bits in every lane, so what hangs on ok is workgroup-uniform.  Not ok:
// Y[k] as formed, Z[k] = +0.0, innovation[k] = d, accept[k] = 0.0, and no row takes observation k; the two barriers
// behind the stores stand outside the test, so all kAsThreads threads reach them either way and xk is free when it
// is refilled.  The epilogue walks the update's lists (g.list, every block's, nlist entries) and writes
// ens_lu_filler() over each entry of a rejected observation: k_ens_local, unchanged and behind this launch on the
// same stream, rejects a filler on its scalar compares, so no field point takes the observation and a point that
// only rejected observations reach is not stored.  A filler's own k is 0: accept[0] decides whether a filler is
// written over it.  Without kGate g is not read and the text is what it was: the ungated kernels keep their bytes.
template <int kSrc, bool kGate>
__device__ __forceinline__ void as_stage(const EnsAsArgs a, const EnsObsOp h, const EnsRecSrc r, const EnsAsGate g,
                                         double *xk, double *yk, double *zk)
{
    const int tid = (int)threadIdx.x, n = a.n, nobs = a.nobs;
    const long row = a.row;
    const double dn = (double)n, dn1 = (double)(n - 1);

    // prologue: the gather, the padding, the prior spread
    for (long q = tid; q < (long)nobs * row; q += kAsThreads) {
        const int j = (int)(q / row), m = (int)(q % row);
        if (m < n) {
            if constexpr (kSrc == kAsOperator) a.hx[q] = obs_apply(h, j, m);
            else if constexpr (kSrc == kAsRecords) a.hx[q] = rec_interp(r, j, m);
            else a.hx[q] = a.tab[(long)a.blk[j] * n + m][a.off[j]];
        } else {
            a.hx[q] = 0.0; a.y[q] = 0.0; a.z[q] = 0.0;
        }
    }
    __syncthreads();
    for (int j = tid; j < nobs; j += kAsThreads) a.prior[j] = as_spread(a.hx + (long)j * row, n);

    long bad = 0;   // (thread 0's count)
    for (int k = 0; k < nobs; ++k) {
        // row k into LDS, one member per thread: every lane then walks it at LDS latency, not at L2's
        for (int m = tid; m < n; m += kAsThreads) xk[m] = a.hx[(long)k * row + m];
        __syncthreads();
        const double *x = xk;
        double s1 = 0.0, q = 0.0;
        for (int m0 = 0; m0 < n; m0 += kAsChunk) {   // (chunks as in the rows' update below)
            double v[kAsChunk];
#pragma unroll
            for (int e = 0; e < kAsChunk; ++e) v[e] = x[m0 + e];
#pragma unroll
            for (int e = 0; e < kAsChunk; ++e)
                if (m0 + e < n) s1 = m0 + e == 0 ? v[e] : s1 + v[e];
        }
        const double ybar = s1 / dn;
        for (int m0 = 0; m0 < n; m0 += kAsChunk) {
            double v[kAsChunk];
#pragma unroll
            for (int e = 0; e < kAsChunk; ++e) v[e] = x[m0 + e];
#pragma unroll
            for (int e = 0; e < kAsChunk; ++e)
                if (m0 + e < n) {
                    const double ym = v[e] - ybar;
                    const double p = ym * ym;
                    q = m0 + e == 0 ? p : q + p;
                }
        }
        const double s = q / dn1;
        const double r = a.variance[k];
        const double D = s + r;
        const double d = a.value[k] - ybar;
        const double t = r / D;
        const double alpha = 1.0 / (1.0 + sqrt(t));
        const double c = dn1 * D;
        bool ok = true;
        if constexpr (kGate) {
            const double lim = g.gate2 * D;
            ok = isfinite(D) && isfinite(d) && d * d <= lim;
        }
        for (int m = tid; m < n; m += kAsThreads) {
            const double ym = x[m] - ybar;
            const double zm = ok ? (d - alpha * ym) / c : 0.0;
            yk[m] = ym; zk[m] = zm;
            a.y[(long)k * row + m] = ym;
            a.z[(long)k * row + m] = zm;
        }
        if (tid == 0) {
            a.innovation[k] = d;
            if (!(isfinite(D) && isfinite(d))) ++bad;
            if constexpr (kGate) g.accept[k] = ok ? 1.0 : 0.0;
        }
        __syncthreads();   // Y[k], Z[k] in LDS; every lane has read row k
        const int iok = a.io[k], jok = a.jo[k];
        for (int j = tid; ok && j < nobs; j += kAsThreads) {
            const int di = a.io[j] - iok, dj = a.jo[j] - jok;   // (both within the basin: no overflow)
            if (di > a.reach || -di > a.reach || dj > a.reach || -dj > a.reach) continue;
            const int d2 = di * di + dj * dj;                   // (reach <= 255)
            if (d2 >= a.ntaper) continue;
            const double rho = a.taper[d2];
            if (rho != 0.0) {   // (not +0.0 / -0.0; the table's entries are finite)
                // the row through registers kAsChunk members at a time: a chunk's loads go out together, the
                // operations follow in member order (constant indices after unrolling: no scratch)
                double *xj = a.hx + (long)j * row;
                double sj = 0.0, acc = 0.0;
                for (int m0 = 0; m0 < n; m0 += kAsChunk) {
                    double v[kAsChunk];
#pragma unroll
                    for (int e = 0; e < kAsChunk; ++e)
                        v[e] = xj[m0 + e];   // (the row's padding is there to be read)
#pragma unroll
                    for (int e = 0; e < kAsChunk; ++e)
                        if (m0 + e < n) sj = m0 + e == 0 ? v[e] : sj + v[e];
                }
                const double mean = sj / dn;
                for (int m0 = 0; m0 < n; m0 += kAsChunk) {
                    double v[kAsChunk];
#pragma unroll
                    for (int e = 0; e < kAsChunk; ++e)
                        v[e] = xj[m0 + e];   // (the row's padding is there to be read)
#pragma unroll
                    for (int e = 0; e < kAsChunk; ++e)
                        if (m0 + e < n) {
                            const double p = (v[e] - mean) * yk[m0 + e];
                            acc = m0 + e == 0 ? p : acc + p;
                        }
                }
                const double g = rho * acc;
                for (int m0 = 0; m0 < n; m0 += kAsChunk) {
                    double v[kAsChunk];
#pragma unroll
                    for (int e = 0; e < kAsChunk; ++e)
                        v[e] = xj[m0 + e];   // (the row's padding is there to be read)
#pragma unroll
                    for (int e = 0; e < kAsChunk; ++e)
                        if (m0 + e < n) xj[m0 + e] = v[e] + g * zk[m0 + e];
                }
            }
        }
        __syncthreads();   // the rows as observation k leaves them; yk, zk free
    }

    for (int j = tid; j < nobs; j += kAsThreads) a.posterior[j] = as_spread(a.hx + (long)j * row, n);
    if (tid == 0) *a.nonfinite = bad;
    if constexpr (kGate) {
        // (accept[] is thread 0's, published by the loop's last barrier as the rows are; an entry's k < nobs)
        for (int q = tid; q < g.nlist; q += kAsThreads)
            if (g.accept[g.list[q].k] == 0.0) g.list[q] = ens_lu_filler();
    }
}

__global__ __launch_bounds__(kAsThreads) void k_ens_obs_space(const EnsAsArgs a)
{
    __shared__ double xk[OCN_ENS_MAX_MEMBERS], yk[OCN_ENS_MAX_MEMBERS], zk[OCN_ENS_MAX_MEMBERS];
    as_stage<kAsPoints, false>(a, EnsObsOp{}, EnsRecSrc{}, EnsAsGate{}, xk, yk, zk);
}

__global__ __launch_bounds__(kAsThreads) void k_ens_obs_space_g(const EnsAsArgs a, const EnsAsGate g)
{
    __shared__ double xk[OCN_ENS_MAX_MEMBERS], yk[OCN_ENS_MAX_MEMBERS], zk[OCN_ENS_MAX_MEMBERS];
    as_stage<kAsPoints, true>(a, EnsObsOp{}, EnsRecSrc{}, g, xk, yk, zk);
}

// grid: (observations / 256, members)
__global__ __launch_bounds__(256) void k_ens_sample_h(const EnsObsOp h, int n, int nobs, double *__restrict__ out)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x), m = (int)blockIdx.y;
    if (j >= nobs) return;
    out[(long)j * n + m] = obs_apply(h, j, m);
}

// k_ens_obs_space with the operator in its prologue: one thread per (observation, member) in turn
__global__ __launch_bounds__(kAsThreads) void k_ens_obs_space_h(const EnsAsArgs a, const EnsObsOp h)
{
    __shared__ double xk[OCN_ENS_MAX_MEMBERS], yk[OCN_ENS_MAX_MEMBERS], zk[OCN_ENS_MAX_MEMBERS];
    as_stage<kAsOperator, false>(a, h, EnsRecSrc{}, EnsAsGate{}, xk, yk, zk);
}

__global__ __launch_bounds__(kAsThreads) void k_ens_obs_space_hg(const EnsAsArgs a, const EnsObsOp h, const EnsAsGate g)
{
    __shared__ double xk[OCN_ENS_MAX_MEMBERS], yk[OCN_ENS_MAX_MEMBERS], zk[OCN_ENS_MAX_MEMBERS];
    as_stage<kAsOperator, true>(a, h, EnsRecSrc{}, g, xk, yk, zk);
}

// one thread per (observation, member), the member fastest: a wave's series loads and its stores are contiguous
// runs (k_ens_sample_h's mapping, j fastest, would stride the series by the recorder's member count)
__global__ __launch_bounds__(256) void k_ens_record_sample(const EnsRecSrc r, int n, long total, double *__restrict__ out)
{
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    out[q] = rec_interp(r, (int)(q / n), (int)(q % n));
}

// k_ens_obs_space with the recorder's series in its prologue
__global__ __launch_bounds__(kAsThreads) void k_ens_obs_space_r(const EnsAsArgs a, const EnsRecSrc r)
{
    __shared__ double xk[OCN_ENS_MAX_MEMBERS], yk[OCN_ENS_MAX_MEMBERS], zk[OCN_ENS_MAX_MEMBERS];
    as_stage<kAsRecords, false>(a, EnsObsOp{}, r, EnsAsGate{}, xk, yk, zk);
}

__global__ __launch_bounds__(kAsThreads) void k_ens_obs_space_rg(const EnsAsArgs a, const EnsRecSrc r, const EnsAsGate g)
{
    __shared__ double xk[OCN_ENS_MAX_MEMBERS], yk[OCN_ENS_MAX_MEMBERS], zk[OCN_ENS_MAX_MEMBERS];
    as_stage<kAsRecords, true>(a, EnsObsOp{}, r, g, xk, yk, zk);
}

int launch_ens_obs_space(const EnsAsArgs &a, hipStream_t s)
{
    if (a.n < 2 || a.n > OCN_ENS_MAX_MEMBERS || a.nobs < 1 || a.ntaper < 1 || a.reach < 0 || a.reach > 255 ||
        a.row != (long)ens_lu_row(a.n) || !a.tab || !a.off || !a.blk || !a.io || !a.jo || !a.value || !a.variance ||
        !a.taper || !a.hx || !a.y || !a.z || !a.innovation || !a.prior || !a.posterior || !a.nonfinite)
        return set_error(OCN_ERR_ARG, "ens_obs_space: member count, tables or reach");
    hipLaunchKernelGGL(k_ens_obs_space, dim3(1), dim3(kAsThreads), 0, s, a);
    return check_launch();
}

int launch_ens_sample_h(const EnsObsOp &h, int n, int nobs, double *d_out, hipStream_t s)
{
    if (n < 1 || n > OCN_ENS_MAX_MEMBERS || nobs < 1 || !h.tab || !h.start || !h.term || !d_out)
        return set_error(OCN_ERR_ARG, "ens_sample_h: nothing to gather");
    hipLaunchKernelGGL(k_ens_sample_h, dim3((unsigned)((nobs + 255) / 256), (unsigned)n), dim3(256), 0, s, h, n, nobs, d_out);
    return check_launch();
}

int launch_ens_obs_space_h(const EnsAsArgs &a, const EnsObsOp &h, hipStream_t s)
{
    if (a.n < 2 || a.n > OCN_ENS_MAX_MEMBERS || a.nobs < 1 || a.ntaper < 1 || a.reach < 0 || a.reach > 255 ||
        a.row != (long)ens_lu_row(a.n) || !h.tab || !h.start || !h.term || !a.io || !a.jo || !a.value || !a.variance ||
        !a.taper || !a.hx || !a.y || !a.z || !a.innovation || !a.prior || !a.posterior || !a.nonfinite)
        return set_error(OCN_ERR_ARG, "ens_obs_space_h: member count, tables or reach");
    hipLaunchKernelGGL(k_ens_obs_space_h, dim3(1), dim3(kAsThreads), 0, s, a, h);
    return check_launch();
}

int launch_ens_record_sample(const EnsRecSrc &r, int n, int nobs, double *d_out, hipStream_t s)
{
    if (n < 1 || n > OCN_ENS_MAX_MEMBERS || nobs < 1 || nobs > 65536 || !r.series || !r.obs || !r.col || r.next < 1 || !d_out)
        return set_error(OCN_ERR_ARG, "ens_record_sample: nothing to gather");
    const long total = (long)nobs * n;   // (at most 2^24: the grid's x dimension holds it)
    hipLaunchKernelGGL(k_ens_record_sample, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, r, n, total, d_out);
    return check_launch();
}

int launch_ens_obs_space_r(const EnsAsArgs &a, const EnsRecSrc &r, hipStream_t s)
{
    if (a.n < 2 || a.n > OCN_ENS_MAX_MEMBERS || a.nobs < 1 || a.ntaper < 1 || a.reach < 0 || a.reach > 255 ||
        a.row != (long)ens_lu_row(a.n) || !r.series || !r.obs || !r.col || r.next < 1 || !a.io || !a.jo || !a.value ||
        !a.variance || !a.taper || !a.hx || !a.y || !a.z || !a.innovation || !a.prior || !a.posterior || !a.nonfinite)
        return set_error(OCN_ERR_ARG, "ens_obs_space_r: member count, tables or reach");
    hipLaunchKernelGGL(k_ens_obs_space_r, dim3(1), dim3(kAsThreads), 0, s, a, r);
    return check_launch();
}

// what the gated launches check beyond their siblings: a threshold > 0 (not NaN; +inf allowed), the arrays
static bool as_gate_bad(const EnsAsGate &g) { return !(g.gate2 > 0.0) || !g.accept || !g.list || g.nlist < 0; }

int launch_ens_obs_space_g(const EnsAsArgs &a, const EnsAsGate &g, hipStream_t s)
{
    if (a.n < 2 || a.n > OCN_ENS_MAX_MEMBERS || a.nobs < 1 || a.ntaper < 1 || a.reach < 0 || a.reach > 255 ||
        a.row != (long)ens_lu_row(a.n) || !a.tab || !a.off || !a.blk || !a.io || !a.jo || !a.value || !a.variance ||
        !a.taper || !a.hx || !a.y || !a.z || !a.innovation || !a.prior || !a.posterior || !a.nonfinite || as_gate_bad(g))
        return set_error(OCN_ERR_ARG, "ens_obs_space_g: member count, tables, reach or gate");
    hipLaunchKernelGGL(k_ens_obs_space_g, dim3(1), dim3(kAsThreads), 0, s, a, g);
    return check_launch();
}

int launch_ens_obs_space_hg(const EnsAsArgs &a, const EnsObsOp &h, const EnsAsGate &g, hipStream_t s)
{
    if (a.n < 2 || a.n > OCN_ENS_MAX_MEMBERS || a.nobs < 1 || a.ntaper < 1 || a.reach < 0 || a.reach > 255 ||
        a.row != (long)ens_lu_row(a.n) || !h.tab || !h.start || !h.term || !a.io || !a.jo || !a.value || !a.variance ||
        !a.taper || !a.hx || !a.y || !a.z || !a.innovation || !a.prior || !a.posterior || !a.nonfinite || as_gate_bad(g))
        return set_error(OCN_ERR_ARG, "ens_obs_space_hg: member count, tables, reach or gate");
    hipLaunchKernelGGL(k_ens_obs_space_hg, dim3(1), dim3(kAsThreads), 0, s, a, h, g);
    return check_launch();
}

int launch_ens_obs_space_rg(const EnsAsArgs &a, const EnsRecSrc &r, const EnsAsGate &g, hipStream_t s)
{
    if (a.n < 2 || a.n > OCN_ENS_MAX_MEMBERS || a.nobs < 1 || a.ntaper < 1 || a.reach < 0 || a.reach > 255 ||
        a.row != (long)ens_lu_row(a.n) || !r.series || !r.obs || !r.col || r.next < 1 || !a.io || !a.jo || !a.value ||
        !a.variance || !a.taper || !a.hx || !a.y || !a.z || !a.innovation || !a.prior || !a.posterior || !a.nonfinite ||
        as_gate_bad(g))
        return set_error(OCN_ERR_ARG, "ens_obs_space_rg: member count, tables, reach or gate");
    hipLaunchKernelGGL(k_ens_obs_space_rg, dim3(1), dim3(kAsThreads), 0, s, a, r, g);
    return check_launch();
}

}  // namespace ocn
