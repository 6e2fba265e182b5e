// Optimal-decay CBF-QP: the row build and the exact solve, shared by the single-solve kernel (csrc/od_cbf_qp.hip) and the fused
// closed loop (csrc/tracking_od.hip).
//   OptimalDecayCBFQP.solve_control_problem   position_control/optimal_decay_cbf_qp.py:131-158
// The QP has 4 variables (u0, u1, omega1, omega2), a diagonal Hessian diag(1, 1, p1, p2), ONE general
// row  a0 u0 + a1 u1 + e1 w1 + e2 w2 + b >= 0  and a box on (u0, u1).  Strictly convex => unique
// minimiser; it is found exactly by checking the KKT conditions of the 1 + 9 possible active sets
// (row inactive; row active with each of u0, u1 free / at its lower / at its upper bound).
#pragma once
#include "sc_models.hpp"

namespace sc {

template <typename T>
struct OdSol { T u0, u1, w1, w2, cost; bool ok; };

// the row  a0 u0 + a1 u1 + e1 w1 + e2 w2 + b >= 0  of one obstacle (all zero without one, optimal_decay_cbf_qp.py:133-137)
template <typename T>
struct OdRow { T a0, a1, b, e1, e2, h; bool bad; };

template <int MODEL>
struct od_rel2 {
    static constexpr bool value = (MODEL == SC_MODEL_DYNAMIC_UNICYCLE2D || MODEL == SC_MODEL_KINEMATIC_BICYCLE2D || MODEL == SC_MODEL_QUAD2D);
};

template <typename TC>
__device__ __forceinline__ OdRow<TC> od_row_none() {
    OdRow<TC> r;
    r.a0 = 0; r.a1 = 0; r.b = 0; r.e1 = 0; r.e2 = 0; r.h = 0; r.bad = false;
    return r;
}

// A = dh g, b = dh f (optimal_decay_cbf_qp.py:138-146), e1, e2; `o` is one 7-wide obstacle row
template <typename TC, int MODEL>
__device__ __forceinline__ OdRow<TC> od_build_row(const Agent<TC>& ag, const TC* o, const CbfConsts<TC>& k) {
    TC a0 = 0, a1 = 0, b = 0, e1 = 0, e2 = 0, h = 0;
    bool bad = false;
    if constexpr (MODEL == SC_MODEL_QUAD2D) {
        // optimal_decay_cbf_qp.py:38-45,105-115,141-146 over robots/quad2D.py:166-177 (circle, no flag test) and g of :68-81: both
        // thrusts enter alike, A = dh_dot_dx g = [a, a], a = 2 (-ex sin th + ez cos th) / m; b = dh_dot_dx f = 2 |v|^2 - 2 g ez
        const TC ex = ag.x - o[0], ez = ag.y - o[1];
        const TC dmin = o[2] + k.R;
        h = (ex * ex + ez * ez) - TC(1.01) * dmin * dmin;
        const TC hdot = TC(2) * (ex * ag.f0 + ez * ag.f1);
        a0 = (TC(2) * ex * (-ag.s) + TC(2) * ez * ag.c) * k.inv_mass;
        a1 = a0;
        b = TC(2) * ag.f0 * ag.f0 + TC(2) * ag.f1 * ag.f1 + TC(2) * ez * TC(-9.81);
        e1 = k.g1 * hdot;
        e2 = k.g2 * h;
    } else if constexpr (od_rel2<MODEL>::value) {
        TC hdot, d[4];
        if constexpr (MODEL == SC_MODEL_DYNAMIC_UNICYCLE2D) {
            if (o[6] == TC(0)) hocbf_circle(ag, o, k.R, TC(1.01), h, hdot, d);
            else if (o[6] == TC(1)) hocbf_superellipsoid(ag, o, k.R, h, hdot, d);
            else { bad = true; h = hdot = 0; d[0] = d[1] = d[2] = d[3] = 0; }
            a0 = d[3]; a1 = d[2];
        } else {
            hocbf_circle(ag, o, k.R, TC(1.1), h, hdot, d);
            a0 = d[3];
            a1 = -ag.f1 * d[0] + ag.f0 * d[1] + ag.v * k.inv_Lr * d[2];
        }
        b = d[0] * ag.f0 + d[1] * ag.f1;
        e1 = k.g1 * hdot;                    // (alpha1 + alpha2) h_dot
        e2 = k.g2 * h;                       // alpha1 alpha2 h
    } else {
        TC d[4];
        if constexpr (MODEL == SC_MODEL_KINEMATIC_BICYCLE2D_C3BF) c3bf(ag, o, k.R, h, d);
        else dpcbf(ag, o, k.R, h, d);
        // the reference's max(|p|^2 - ego^2, eps) hands a NaN radius on (kinematic_bicycle2D_c3bf.py:15-75); fmax_ in c3bf() drops it
        // and leaves a finite row.  An infinite radius gives eps there and here alike
        if (o[2] != o[2]) h = num<TC>::nan();
        a0 = d[3];
        a1 = -ag.f1 * d[0] + ag.f0 * d[1] + ag.v * k.inv_Lr * d[2];
        b = d[0] * ag.f0 + d[1] * ag.f1;
        e1 = k.a1 * h;                       // alpha h
        e2 = TC(0);
    }
    OdRow<TC> r;
    r.a0 = a0; r.a1 = a1; r.b = b; r.e1 = e1; r.e2 = e2; r.h = h; r.bad = bad;
    return r;
}

// exact solve by KKT enumeration; returns SC_STATUS_* and (u, omega), NaN unless optimal
template <typename TC, bool REL2>
__device__ __forceinline__ int od_solve(const OdRow<TC>& row, const TC r0, const TC r1, const TC wr1, const TC wr2, const TC p1,
                                        const TC p2, const CbfConsts<TC>& k, TC& u0_out, TC& u1_out, TC& w1_out, TC& w2_out) {
    const TC a0 = row.a0, a1 = row.a1, b = row.b, e1 = row.e1, e2 = row.e2;
    const TC tol = num<TC>::tol_feas();
    const TC c0 = fmin_(fmax_(r0, k.lo0), k.hi0), c1 = fmin_(fmax_(r1, k.lo1), k.hi1);
    OdSol<TC> best;
    best.ok = false; best.cost = num<TC>::inf(); best.u0 = c0; best.u1 = c1; best.w1 = wr1; best.w2 = wr2;
    const TC rowscale = fmax_(TC(1), fabs_(a0 * c0) + fabs_(a1 * c1) + fabs_(e1 * wr1) + fabs_(e2 * wr2) + fabs_(b));
    // (1) row inactive
    {
        const TC s = a0 * c0 + a1 * c1 + e1 * wr1 + e2 * wr2 + b;
        if (s >= -tol * rowscale) {
            best.ok = true;
            best.cost = (c0 - r0) * (c0 - r0) + (c1 - r1) * (c1 - r1);
        }
    }
    // (2) row active, u0 / u1 each free (0), at lo (1) or at hi (2)
    const TC iw1 = e1 * e1 / p1, iw2 = REL2 ? e2 * e2 / p2 : TC(0);
#pragma unroll
    for (int q0 = 0; q0 < 3; ++q0) {
#pragma unroll
        for (int q1 = 0; q1 < 3; ++q1) {
            const TC f0 = q0 == 1 ? k.lo0 : k.hi0, f1 = q1 == 1 ? k.lo1 : k.hi1;
            const TC x0 = q0 == 0 ? r0 : f0, x1 = q1 == 0 ? r1 : f1;            // fixed at bound, else reference
            const TC s = a0 * x0 + a1 * x1 + e1 * wr1 + e2 * wr2 + b;             // row value at that point
            const TC den = (q0 == 0 ? a0 * a0 : TC(0)) + (q1 == 0 ? a1 * a1 : TC(0)) + iw1 + iw2;
            // stationarity: 2 D (x - r) = lam a on the free variables, row = 0  =>  lam = -2 s / den
            const TC lam = TC(-2) * s / den;
            const TC u0 = q0 == 0 ? r0 + TC(0.5) * lam * a0 : f0;
            const TC u1 = q1 == 0 ? r1 + TC(0.5) * lam * a1 : f1;
            const TC w1 = wr1 + TC(0.5) * lam * e1 / p1;
            const TC w2 = REL2 ? wr2 + TC(0.5) * lam * e2 / p2 : wr2;
            bool ok = (den > TC(0)) && (lam >= -tol);
            const TC btol = tol * fmax_(TC(1), fmax_(fabs_(k.hi0), fabs_(k.hi1)));
            // free inputs inside the box, fixed inputs pushed against their bound (multiplier >= 0)
            if (q0 == 0) ok = ok && (u0 >= k.lo0 - btol) && (u0 <= k.hi0 + btol);
            if (q0 == 1) ok = ok && (TC(2) * (k.lo0 - r0) - lam * a0 >= -tol);
            if (q0 == 2) ok = ok && (lam * a0 - TC(2) * (k.hi0 - r0) >= -tol);
            if (q1 == 0) ok = ok && (u1 >= k.lo1 - btol) && (u1 <= k.hi1 + btol);
            if (q1 == 1) ok = ok && (TC(2) * (k.lo1 - r1) - lam * a1 >= -tol);
            if (q1 == 2) ok = ok && (lam * a1 - TC(2) * (k.hi1 - r1) >= -tol);
            const TC cost = (u0 - r0) * (u0 - r0) + (u1 - r1) * (u1 - r1) + p1 * (w1 - wr1) * (w1 - wr1) +
                            (REL2 ? p2 * (w2 - wr2) * (w2 - wr2) : TC(0));
            if (ok && cost < best.cost) {
                best.ok = true; best.cost = cost; best.u0 = u0; best.u1 = u1; best.w1 = w1; best.w2 = w2;
            }
        }
    }
    const bool finite = finite_(a0 + a1 + b + e1 + e2 + r0 + r1);
    int st = (best.ok && finite) ? SC_STATUS_OPTIMAL : SC_STATUS_INFEASIBLE;
    if (row.bad) st = SC_STATUS_BAD_OBSTACLE;
    TC u0 = fmin_(fmax_(best.u0, k.lo0), k.hi0), u1 = fmin_(fmax_(best.u1, k.lo1), k.hi1);
    TC w1 = best.w1, w2 = best.w2;
    if (st != SC_STATUS_OPTIMAL) { u0 = u1 = w1 = w2 = num<TC>::nan(); }
    u0_out = u0; u1_out = u1; w1_out = w1; w2_out = w2;
    return st;
}

}  // namespace sc
