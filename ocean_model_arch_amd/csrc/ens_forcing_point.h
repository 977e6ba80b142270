// ens_forcing_point.h -- the moving-storm forcing at one point (include/ocn_sw.h ocn_ens_forcing_*): the wind
// stress and the air pressure gradient of a Gaussian vortex as OCN_RHSX / OCN_RHSY take them.
//
// One text for the device (ens_forcing.hip, hipcc) and for the host (tests/test_ens_forcing_cpu.py, g++ with
// __host__ and __device__ defined away): every statement below is ONE IEEE double operation in the order the
// header states, so with -ffp-contract=off both give the same bits; ocean_model_arch_amd/ens_forcing_rule.py
// restates it in numpy.  No division by r, no pow, no log, no sin or cos; exp is ocn_exp.h exp_libm, whose
// domain |x| < 512 the clamp at -500 keeps (the exponents are at most 0.5).
#pragma once
#include <cmath>

#include "../../include/ocn_sw.h"
#include "ocn_exp.h"

namespace ocn {

// what a storm and the model give at one time t: the same for every point
struct FrcAt { double xc, yc, rr, sv, ra; };

__host__ __device__ inline FrcAt frc_at(const ocn_ens_storm &s, const ocn_ens_forcing_model &m, double t)
{
    FrcAt c;
    double p = s.cx * t;
    c.xc = s.x0 + p;
    p = s.cy * t;
    c.yc = s.y0 + p;
    c.rr = s.radius * s.radius;
    c.sv = s.vmax / s.radius;
    c.ra = m.rho_air / m.rho_water;
    return c;
}

// the offsets ex, ey (m) of the index position (xi, yj) from the centre with sx, sy metres per index step, and
// q = r^2 / R^2
__host__ __device__ inline double frc_q(const FrcAt &c, double xi, double yj, double sx, double sy, double &ex, double &ey)
{
    double d = xi - c.xc;
    ex = d * sx;
    d = yj - c.yc;
    ey = d * sy;
    const double a = ex * ex;
    const double b = ey * ey;
    const double s = a + b;
    return s / c.rr;
}

// the kinematic wind stress (taux, tauy) at (xi, yj)
__host__ __device__ inline void frc_stress(const ocn_ens_storm &s, const ocn_ens_forcing_model &m, const FrcAt &c, double xi,
                                           double yj, double sx, double sy, double &taux, double &tauy)
{
    double ex, ey;
    const double q = frc_q(c, xi, yj, sx, sy, ex, ey);
    const double h = 0.5 * q;
    double a = 0.5 - h;
    a = a > -500.0 ? a : -500.0;
    const double e = exp_libm(a);
    const double sp = c.sv * e;
    double te = s.turn * ey;
    double a1 = te * s.cos_in;
    a1 = -a1;
    double b1 = ex * s.sin_in;
    double c1 = a1 - b1;
    c1 = sp * c1;
    const double uw = m.ub + c1;
    te = s.turn * ex;
    a1 = te * s.cos_in;
    b1 = ey * s.sin_in;
    c1 = a1 - b1;
    c1 = sp * c1;
    const double vw = m.vb + c1;
    a1 = uw * uw;
    b1 = vw * vw;
    const double ss = a1 + b1;
    const double w = sqrt(ss);
    double cd = m.cd1 * w;
    cd = m.cd0 + cd;
    cd = cd < m.cd_max ? cd : m.cd_max;
    double k = c.ra * cd;
    k = k * w;
    taux = k * uw;
    tauy = k * vw;
}

// the air pressure anomaly (Pa, <= 0) at (xi, yj)
__host__ __device__ inline double frc_pa(const ocn_ens_storm &s, const FrcAt &c, double xi, double yj, double sx, double sy)
{
    double ex, ey;
    const double q = frc_q(c, xi, yj, sx, sy, ex, ey);
    double h = -0.5 * q;
    h = h > -500.0 ? h : -500.0;
    const double e = exp_libm(h);
    const double pa = s.dp * e;
    return -pa;
}

// what a face takes of its two t-points' pressures: the stress over the face's area less the pressure gradient
// over the rest depth.  tau: the stress component along the face's normal; da, db: the face's two metrics in
// the order the header pairs them (ar = da db); dg: the one the gradient keeps; pa0, pa1, h0, h1: the pressure
// and h_r at this t-point and at the next one along the normal
__host__ __device__ inline double frc_face(const ocn_ens_forcing_model &m, double tau, double da, double db, double dg,
                                           double pa0, double pa1, double h0, double h1)
{
    const double ar = da * db;
    const double a = tau * ar;
    double d = pa1 - pa0;
    d = d / m.rho_water;
    d = d * dg;
    double hf = h0 + h1;
    hf = 0.5 * hf;
    d = d * hf;
    return a - d;
}

// The real(4) metrics and masks and h_r of the points RHSx(m, n) and RHSy(m, n) read
struct FrcPoint {
    float lcu, lcv, dxt, dyt, dxh, dyh;
    float dx0, dy0, dx1, dy1, dx2, dy2;   // dx, dy at (m, n), (m + 1, n), (m, n + 1)
    double h0, h1, h2;                    // h_r there
};

// RHSx(m, n) and RHSy(m, n) at the global 1-based point (m, n)
__host__ __device__ inline void frc_point(const ocn_ens_storm &s, const ocn_ens_forcing_model &mo, const FrcAt &c, int m, int n,
                                          const FrcPoint &p, double &rx, double &ry)
{
    const double xm = (double)m, yn = (double)n;
    const double pa0 = frc_pa(s, c, xm, yn, (double)p.dx0, (double)p.dy0);
    rx = 0.0;
    ry = 0.0;
    if (p.lcu > 0.5f) {
        double taux, tauy;
        frc_stress(s, mo, c, xm + 0.5, yn, (double)p.dxt, (double)p.dyh, taux, tauy);
        const double pa1 = frc_pa(s, c, xm + 1.0, yn, (double)p.dx1, (double)p.dy1);
        rx = frc_face(mo, taux, (double)p.dxt, (double)p.dyh, (double)p.dyh, pa0, pa1, p.h0, p.h1);
    }
    if (p.lcv > 0.5f) {
        double taux, tauy;
        frc_stress(s, mo, c, xm, yn + 0.5, (double)p.dxh, (double)p.dyt, taux, tauy);
        const double pa2 = frc_pa(s, c, xm, yn + 1.0, (double)p.dx2, (double)p.dy2);
        ry = frc_face(mo, tauy, (double)p.dyt, (double)p.dxh, (double)p.dxh, pa0, pa2, p.h0, p.h2);
    }
}

}  // namespace ocn
