// ens_peak_point.h -- the running extreme of one point (include/ocn_sw.h ocn_ens_peak_*): whether the value x a
// step has left replaces the peak P held so far.
//
// One text for the device (ens_peak.hip and sw_kernels.hip k_march_multi_pk, hipcc) and for the host
// (tests/test_ens_peak_cpu.py, g++ with __host__ and __device__ defined away); ocean_model_arch_amd/ens_peak_rule.py
// restates it in numpy.  The comparisons are ocn_ens_stats' MIN / MAX (ens_stats.hip ext_take):
//   MAX:  if (x > P || P != P) { P = x; S = k; }        MIN: the same with <
// so a tie -- +0.0 against -0.0 included -- keeps the earlier step and its bits, a NaN in P goes as soon as a
// number arrives, and a NaN x never replaces a number.  (While P is NaN every x replaces it, a NaN x too: S then
// names the last step so far.)
#pragma once
#include <cstdint>

namespace ocn {

template <bool MIN> __host__ __device__ inline bool peak_takes(double x, double P)
{
    return (MIN ? x < P : x > P) || P != P;
}

// the rule on one point's pair: k is the step's number since ocn_ens_peak_begin (1-based)
template <bool MIN> __host__ __device__ inline void peak_point(double x, int32_t k, double &P, int32_t &S)
{
    if (peak_takes<MIN>(x, P)) {
        P = x;
        S = k;
    }
}

}  // namespace ocn
