// Cross-lane helpers for kernels that spread one agent over a group of G lanes (one obstacle row per lane):
// broadcast / min / max inside the group and the cooperative incremental QP walk.  Used by the cooperative CBF-QP
// kernel (cbf_qp_kernel.hpp) and the cooperative closed-loop rollout (tracking.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "sc_qp2.hpp"

namespace sc {

// Cross-lane moves inside a group.  For G = 8 (the headline launch) they are DPP moves -- quad permutes and the
// half-row mirror, VALU latency -- instead of ds_bpermute round trips (~100 cycles each for a wave that has
// nothing else to do): broadcast of lane I = quad broadcast + mirror into the other quad; min / max = xor 1, xor 2,
// mirror.  Wider groups keep the shuffles.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
template <typename T, int G, int I>
__device__ __forceinline__ T group_bcast(T v, int sub) {
    if constexpr (G == 8) {
        const T q = dpp_mov<(I & 3) * 0x55>(v);             // quad_perm [I&3, I&3, I&3, I&3]
        const T m = dpp_mov<0x141>(q);                      // row_half_mirror: the other quad's value
        return ((sub >> 2) == (I >> 2)) ? q : m;
    } else {
        return __shfl(v, I, G);
    }
}
template <typename T, int G>
__device__ __forceinline__ T group_max(T v) {
    if constexpr (G == 8) {
        v = fmax_(v, dpp_mov<0xB1>(v)); v = fmax_(v, dpp_mov<0x4E>(v)); v = fmax_(v, dpp_mov<0x141>(v));
    } else {
#pragma unroll
        for (int o = 1; o < G; o <<= 1) v = fmax_(v, __shfl_xor(v, o));
    }
    return v;
}
template <typename T, int G>
__device__ __forceinline__ T group_min(T v) {
    if constexpr (G == 8) {
        v = fmin_(v, dpp_mov<0xB1>(v)); v = fmin_(v, dpp_mov<0x4E>(v)); v = fmin_(v, dpp_mov<0x141>(v));
    } else {
#pragma unroll
        for (int o = 1; o < G; o <<= 1) v = fmin_(v, __shfl_xor(v, o));
    }
    return v;
}

// step I of the cooperative walk (I is a template parameter so that the broadcast lane is a DPP immediate)
template <typename TC, int G, int I>
__device__ __forceinline__ void coop_step(QpState<TC>& S, int K, int sub, TC a0, TC a1, TC cc, const CbfConsts<TC>& k) {
    if (I >= K) return;
    const TC bi0 = group_bcast<TC, G, I>(a0, sub), bi1 = group_bcast<TC, G, I>(a1, sub), bic = group_bcast<TC, G, I>(cc, sub);
    LineQP<TC> L;
    const bool viol = qp_row_violated(S, bi0, bi1, bic, L, k);
    if (__builtin_amdgcn_ballot_w64(viol) == 0) return;
    clip_box(L, k);
    if (sub < I) clip_row(L, a0, a1, cc);                 // rows j < i, one per lane, in parallel
    L.lo = group_max<TC, G>(L.lo);
    L.hi = group_min<TC, G>(L.hi);
    qp_row_commit(S, L, viol);
}
template <typename TC, int G, int... Is>
__device__ __forceinline__ void coop_walk(QpState<TC>& S, int K, int sub, TC a0, TC a1, TC cc, const CbfConsts<TC>& k,
                                          std::integer_sequence<int, Is...>) {
    (coop_step<TC, G, Is>(S, K, sub, a0, a1, cc, k), ...);
}

// The same walk, driven by the violated rows instead of by the row index.  Every lane tests its OWN row at the running
// optimum; the first violated row of a group (lowest index above the last committed one) is broadcast and committed;
// repeat until no group of the wave has a violated row left.  Rows that are satisfied when their turn comes change
// nothing in the index-driven walk either, so both visit the same rows in the same order with the same arithmetic --
// but a wave whose agents have no violated row (the common case) leaves after one test instead of K.
template <typename TC, int G>
__device__ __forceinline__ void coop_walk_violated(QpState<TC>& S, int K, int sub, int lane, TC a0, TC a1, TC cc,
                                                   const CbfConsts<TC>& k) {
    const int gbase = lane & ~(G - 1);
    const unsigned long long grp = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << gbase;
    const bool testable = (sub < K) && !((a0 == TC(0)) && (a1 == TC(0)));     // all-zero rows are never projected on
    int last = -1;
#ifndef SC_EXP_MAXIT
#define SC_EXP_MAXIT G                                     // developer builds cap it to time one pass of the loop
#endif
    for (int it = 0; it < SC_EXP_MAXIT; ++it) {               // at most K commits per agent
        const TC s = a0 * S.u0 + (a1 * S.u1 + cc);
        const bool v = testable && (sub > last) && (s < TC(0));
        const unsigned long long m = __builtin_amdgcn_ballot_w64(v);
        if (m == 0ull) break;                                 // wave-uniform
        const unsigned long long mg = m & grp;
        const bool has = mg != 0ull;
        const int istar = has ? (__builtin_ctzll(mg) - gbase) : 0;
        const TC bi0 = __shfl(a0, istar, G), bi1 = __shfl(a1, istar, G), bic = __shfl(cc, istar, G);
        LineQP<TC> L;
        const bool viol = qp_row_violated(S, bi0, bi1, bic, L, k) && has;
        clip_box(L, k);
        if (sub < istar) clip_row(L, a0, a1, cc);             // rows j < i*, one per lane, in parallel
        L.lo = group_max<TC, G>(L.lo);
        L.hi = group_min<TC, G>(L.hi);
        qp_row_commit(S, L, viol);
        last = has ? istar : K;
    }
}

// ---- all candidates at once (G = 8) ---------------------------------------------------------------------------------
// The walk above commits one violated row per pass: its latency is (number of commits of the slowest agent of the WAVE + 1)
// passes of ~1000 cycles each for a lone wave (measured on the headline launch: 0.5 us for the first pass, 1.9 us for the five
// passes its slowest wave needs -- the launch ends with that wave).  This form has a fixed, shorter critical path: the
// minimiser of ||u - u_ref||^2 over {box, rows} is u_box = clamp(u_ref) when no row is violated there; otherwise it lies on the
// line of a row that IS violated at u_box (moving from the optimum towards u_box lowers the objective, so it must leave the
// feasible set through an active row, which u_box then violates), and on that line it is the point of the feasible interval
// closest to the foot of u_ref.  So every lane whose row is violated at u_box clips ITS line against the box and against the
// seven other rows of the group (seven xor-partners: DPP quad permutes and the half-row mirror, no LDS round trip), takes the
// closest point of the interval, and the group keeps the candidate with the smallest distance.  Same clip_box / clip_row /
// midpoint rule as the walk, so the chosen point is computed by the same arithmetic as the walk's last commit on that row;
// feasibility is again decided once, in slack space, by the caller.
template <typename T, int X>
__device__ __forceinline__ T group_xor8(T v, T mirrored) {          // value of lane (sub ^ X), X = 1..7; mirrored = lane (sub ^ 7)
    if constexpr (X == 1) return dpp_mov<0xB1>(v);
    else if constexpr (X == 2) return dpp_mov<0x4E>(v);
    else if constexpr (X == 3) return dpp_mov<0x1B>(v);
    else if constexpr (X == 4) return dpp_mov<0x1B>(mirrored);
    else if constexpr (X == 5) return dpp_mov<0x4E>(mirrored);
    else if constexpr (X == 6) return dpp_mov<0xB1>(mirrored);
    else return mirrored;
}
// ---- the shorter instruction stream of the two solves below -----------------------------------------------------------
// A lone wave per SIMD issues one instruction every four to five cycles, whatever it is, so the solve's time is its executed
// instruction count.  The helpers here compute the same values as fmin_ / fmax_ / clip_row / group_max with fewer
// instructions; they are for the cooperative solves only (the other kernels keep the forms of sc_qp2.hpp).
//
// v_min / v_max without the canonicalising v_max(x, x) the compiler puts in front of an operand whose history it cannot see (a
// value that came through a DPP move): that instruction only turns a signalling NaN into a quiet one, and no value here can be a
// signalling NaN (inputs are converted from storage or produced by arithmetic, both of which quiet).  With IEEE mode on, a quiet
// NaN operand yields the other operand, as fmin / fmax do.
__device__ __forceinline__ float min_raw(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float max_raw(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double min_raw(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double max_raw(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float max_neg_raw(float a, float b) { float r; asm("v_max_f32 %0, %1, -%2" : "=v"(r) : "v"(a), "v"(b)); return r; }     // max(a, -b)
__device__ __forceinline__ double max_neg_raw(double a, double b) { double r; asm("v_max_f64 %0, %1, -%2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float max_abs_one_raw(float a) { float r; asm("v_max_f32 %0, |%1|, 1.0" : "=v"(r) : "v"(a)); return r; }            // max(|a|, 1)
__device__ __forceinline__ double max_abs_one_raw(double a) { double r; asm("v_max_f64 %0, |%1|, 1.0" : "=v"(r) : "v"(a)); return r; }
// keep ? v : a quiet NaN.  For a double only the high word is selected: the low word of a NaN is free, so it stays v's.
__device__ __forceinline__ float keep_or_nan(bool keep, float v) { return keep ? v : __int_as_float(0x7fc00000); }
__device__ __forceinline__ double keep_or_nan(bool keep, double v) {
    return __hiloint2double(keep ? __double2hiint(v) : 0x7ff80000, __double2loint(v));
}
template <typename T>
__device__ __forceinline__ T min8_raw(T v) {
    v = min_raw(v, dpp_mov<0xB1>(v)); v = min_raw(v, dpp_mov<0x4E>(v)); v = min_raw(v, dpp_mov<0x141>(v));
    return v;
}
template <typename T>
__device__ __forceinline__ T min16_raw(T v) { v = min8_raw(v); return min_raw(v, dpp_mov<0x140>(v)); }
// Bitwise OR over the group, for picking the value of ONE lane (every other lane passes 0): the DPP move folds into the 32-bit OR,
// one instruction per word and step where a max of -inf-masked doubles takes four.
template <int CTRL>
__device__ __forceinline__ int or_dpp(int v) { return v | __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
template <int G>
__device__ __forceinline__ int group_or_bits(int v) {
    v = or_dpp<0xB1>(v); v = or_dpp<0x4E>(v); v = or_dpp<0x141>(v);
    if constexpr (G == 16) v = or_dpp<0x140>(v);
    return v;
}
template <int G>
__device__ __forceinline__ float group_pick(bool mine, float v) { return __int_as_float(group_or_bits<G>(mine ? __float_as_int(v) : 0)); }
template <int G>
__device__ __forceinline__ double group_pick(bool mine, double v) {
    const int lo = group_or_bits<G>(mine ? __double2loint(v) : 0), hi = group_or_bits<G>(mine ? __double2hiint(v) : 0);
    return __hiloint2double(hi, lo);
}

// clip_row for the solves below: the same restriction of [L.lo, L.hi] as clip_row (sc_qp2.hpp), value for value, wherever the
// lane's candidate can still be chosen.
//   * "no restriction" is a quiet NaN operand of the max / min instead of -inf / +inf: the interval ends are never NaN on a lane
//     with a finite foot point (clip_box leaves none for a unit direction), so max(lo, NaN) = lo = max(lo, -inf); a lane whose
//     foot point is not finite ends with a non-finite cost and is masked either way.  One select per end instead of four.
//   * a parallel row violated beyond tolerance sets L.lo = +inf in clip_row, which ends in t = inf or NaN, a non-finite point and
//     a masked candidate; here it sets `dead`, and the caller masks the candidate.
//   * a > eps is "not parallel and a >= 0", !(a >= -eps) is "not parallel and not a >= 0" (a NaN included, as in clip_row).
// The dot products, the reciprocal and the quotient are clip_row's, operation for operation.
template <typename T>
__device__ __forceinline__ void clip_row_coop(LineQP<T>& L, bool& dead, T g0, T g1, T gc) {
    const T a = g0 * L.d0 + g1 * L.d1;
    const T r = g0 * L.p0 + (g1 * L.p1 + gc);
    const bool pos = a > num<T>::eps_par();
    const bool neg = !(a >= -num<T>::eps_par());
    const bool par_viol = r < -num<T>::tol_feas() * max_abs_one_raw(gc);
    const T q = r * rcp_(fabs_(a));
    dead |= !pos && !neg && par_viol;
    L.lo = max_neg_raw(L.lo, keep_or_nan(pos, q));
    L.hi = min_raw(L.hi, keep_or_nan(neg, q));
}

// lowest lane of this lane's group that is set in a wave ballot: the group's byte (8 lanes) or half-word (16) of the mask
template <int G>
__device__ __forceinline__ bool group_first(unsigned long long m, int lane, int sub, bool& has) {
    const unsigned bits = (unsigned)(m >> (lane & ~(G - 1))) & ((1u << G) - 1u);
    has = bits != 0u;
    return sub == __builtin_ctz(bits | (1u << G));               // bit G: an empty mask names no lane
}

template <typename TC, int... Xs>
__device__ __forceinline__ void clip_partners8(LineQP<TC>& L, bool& dead, TC a0, TC a1, TC cc, std::integer_sequence<int, Xs...>) {
    const TC m0 = dpp_mov<0x141>(a0), m1 = dpp_mov<0x141>(a1), mc = dpp_mov<0x141>(cc);
    (clip_row_coop(L, dead, group_xor8<TC, Xs + 1>(a0, m0), group_xor8<TC, Xs + 1>(a1, m1), group_xor8<TC, Xs + 1>(cc, mc)), ...);
}
// what both solves do once the interval is known: the closest point of it, its cost, the group's cheapest candidate (lowest lane
// on ties) and that lane's point
template <typename TC, int G>
__device__ __forceinline__ void coop_pick_winner(QpState<TC>& S, const LineQP<TC>& L, bool ok, int sub, int lane) {
    const TC inf = num<TC>::inf();
    TC t = fmin_(fmax_(TC(0), L.lo), L.hi);
    const bool inverted = L.lo > L.hi;
    t = inverted ? TC(0.5) * (L.lo + L.hi) : t;                               // by a hair (rounding): split the difference, as the walk
    const bool empty = L.lo > L.hi + num<TC>::tol_feas() * fmax_(TC(1), fmax_(fabs_(L.lo), fabs_(L.hi)));
    const TC v0 = L.p0 + t * L.d0, v1 = L.p1 + t * L.d1;
    const TC e0 = v0 - S.ur0, e1 = v1 - S.ur1;
    TC cost = e0 * e0 + e1 * e1;
    cost = (ok && !empty && (cost == cost)) ? cost : inf;
    TC best;
    if constexpr (G == 8) best = min8_raw(cost); else best = min16_raw(cost);
    bool has;
    const bool mine = group_first<G>(__builtin_amdgcn_ballot_w64((cost == best) && (best < inf)), lane, sub, has);
    const TC s0 = group_pick<G>(mine, v0), s1 = group_pick<G>(mine, v1);       // a finite cost means a finite point: its bits as they are
    S.u0 = has ? s0 : S.u0;                                                   // no candidate: u_box stays and fails the slack check
    S.u1 = has ? s1 : S.u1;
}
template <typename TC>
__device__ __forceinline__ void coop_solve_all8(QpState<TC>& S, int K, int sub, int lane, TC a0, TC a1, TC cc,
                                                const CbfConsts<TC>& k) {
    const bool testable = (sub < K) && !((a0 == TC(0)) && (a1 == TC(0)));     // all-zero rows are never projected on
    LineQP<TC> L;
    const bool viol = qp_row_violated(S, a0, a1, cc, L, k) && testable;       // S holds u_box; L: the line of this lane's row
    if (__builtin_amdgcn_ballot_w64(viol) == 0ull) return;                   // wave-uniform: nothing violated anywhere
    clip_box(L, k);
    bool dead = false;
    clip_partners8(L, dead, a0, a1, cc, std::make_integer_sequence<int, 7>{});
    coop_pick_winner<TC, 8>(S, L, viol && !dead, sub, lane);
}

// ---- the solve of the specialised K = 8 kernel (cbfqp_coop8_du_kernel) ---------------------------------------------------
// What follows serves cbfqp_coop8_du_kernel only.  A lone wave pays for every instruction it executes, so the fast path of that
// kernel treats every lane as ordinary: no flat direction in the box clip, no partner row parallel to the lane's line, no
// canonicalising v_max(x, x) in front of a min / max.  It does not repair the rare cases either: each lane reports whether it met
// one (coop_solve_all8_fast returns the flag), and a wave in which any lane did discards the fast path's result and runs the
// generic K = 8 sequence (coop_solve_all8 and its neighbours above) from the loaded inputs.  So the forms below only have to be
// right -- bit for bit what the generic forms give -- for lanes of waves that report nothing.
// How many of the 512 waves of the benchmark batch report something is counted in DESIGN.md 1b (none does).

// min / max forms whose operands the compiler would canonicalise first (asm outputs, kernel arguments): the argument above
// min_raw holds for each of them -- see the call sites.  `b` of the *_s forms is wave-uniform (a kernel argument, an SGPR pair).
__device__ __forceinline__ double max_raw_s(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "s"(b)); return r; }
__device__ __forceinline__ double min_raw_s(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "s"(b)); return r; }
__device__ __forceinline__ double max_zero_raw(double a) { double r; asm("v_max_f64 %0, %1, 0" : "=v"(r) : "v"(a)); return r; }             // max(a, 0)
__device__ __forceinline__ double max_one_raw(double a) { double r; asm("v_max_f64 %0, %1, 1.0" : "=v"(r) : "v"(a)); return r; }            // max(a, 1)
__device__ __forceinline__ double max_abs_abs_raw(double a, double b) { double r; asm("v_max_f64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b)); return r; }

// qp_begin / qp_finish_box (sc_qp2.hpp) without the four v_max(x, x) on the box bounds and the two on the point.  The bounds are
// kernel arguments, which the compiler must assume could be signalling NaNs: launch_coop8_du hands them over quieted, u_ref is
// converted from storage, and the point is the output of a min / max or of arithmetic.  Operand order as the compiler emits it
// for fmin_(fmax_(u, lo), hi).
__device__ __forceinline__ void qp_begin_raw(QpState<double>& S, double ur0, double ur1, const CbfConsts<double>& k) {
    S.ur0 = ur0; S.ur1 = ur1;
    S.u0 = min_raw_s(max_raw_s(ur0, k.lo0), k.hi0);
    S.u1 = min_raw_s(max_raw_s(ur1, k.lo1), k.hi1);
}
__device__ __forceinline__ void qp_finish_box_raw(QpState<double>& S, const CbfConsts<double>& k) {
    S.u0 = min_raw_s(max_raw_s(S.u0, k.lo0), k.hi0);
    S.u1 = min_raw_s(max_raw_s(S.u1, k.lo1), k.hi1);
}
// The literals of the specialised solve as wave-uniform values from the argument block (Coop8Consts::k1, filled by launch_coop8_du
// with the bit patterns of num<double>): as a literal each is two s_mov_b32 in front of every instruction that names it, rebuilt
// per use; as an SGPR pair that the wave has fetched anyway it is the instruction's scalar operand.  Same operations, same values.
template <typename T>
struct SolveLit { T tol_feas, eps_par, inf, th_max, neg_beta; };   // th_max: 1e5 of sincos_; neg_beta: -1.01 of the circle barrier

// qp_row_margin (sc_qp2.hpp) of one row against worst = +inf, with max(1, |ci|) as one instruction: ci is the product of
// arithmetic (normalise_row), never a signalling NaN.
__device__ __forceinline__ double qp_row_margin_raw(double a0, double a1, double ci, double u0, double u1, double& poison,
                                                    const SolveLit<double>& lit) {
    const double s = a0 * u0 + (a1 * u1 + ci);
    const double m = s + lit.tol_feas * max_abs_one_raw(ci);
    poison += 0.0 * s;
    return fmin_(lit.inf, m);
}
// qp_status (sc_qp2.hpp) with the infinity of its finiteness test from the argument block: !(|x| < inf) is "inf or NaN"
__device__ __forceinline__ int qp_status_lit(const QpState<double>& S, double worst, double poison, const CbfConsts<double>& k,
                                             const SolveLit<double>& lit) {
    const bool finite = (poison == poison) && (fabs_(S.ur0 + S.ur1) < lit.inf);
    const bool box_ok = (k.lo0 <= k.hi0) && (k.lo1 <= k.hi1);
    return (!(worst >= 0.0) || !finite || !box_ok) ? SC_STATUS_INFEASIBLE : SC_STATUS_OPTIMAL;
}

// clip_box for a line without a flat direction: the two reciprocal chains and the min / max, which is what clip_box gives a lane
// with d0 != 0 and d1 != 0.  A lane with a flat direction gets something else here; the caller reports it.
template <typename T>
__device__ __forceinline__ void clip_box_fast(LineQP<T>& L, const CbfConsts<T>& k) {
    const T r0 = rcp_(L.d0), r1 = rcp_(L.d1);
    const T t1 = (k.lo0 - L.p0) * r0, t2 = (k.hi0 - L.p0) * r0;
    const T t3 = (k.lo1 - L.p1) * r1, t4 = (k.hi1 - L.p1) * r1;
    L.lo = fmax_(fmin_(t1, t2), fmin_(t3, t4));
    L.hi = fmin_(fmax_(t1, t2), fmax_(t3, t4));
}

// clip_row_coop without its parallel-row test: `dead` needs par_viol only where the partner is parallel to the line (!pos && !neg,
// i.e. |a| <= eps_par), so the clip hands back its `a`, the loop keeps the smallest |a| of the seven partners -- one vector
// instruction per partner, the |.| a source modifier -- and the caller reports min |a| <= eps_par.  min |a| <= eps exactly when
// some |a| <= eps; a NaN `a` is not parallel in clip_row_coop (`neg` holds) and the raw minimum passes it over, and seven NaNs
// leave a NaN, which fails the compare.  The restriction of the interval is clip_row_coop's, operation for operation; eps_par is
// an SGPR operand.
__device__ __forceinline__ double min_abs_abs_raw(double a, double b) { double r; asm("v_min_f64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double min_abs_raw(double a, double b) { double r; asm("v_min_f64 %0, %1, |%2|" : "=v"(r) : "v"(a), "v"(b)); return r; }     // min(a, |b|)
__device__ __forceinline__ double clip_row_coop_lazy(LineQP<double>& L, double eps, double g0, double g1, double gc) {
    const double a = g0 * L.d0 + g1 * L.d1;
    const double r = g0 * L.p0 + (g1 * L.p1 + gc);
    const bool pos = a > eps;
    const bool neg = !(a >= -eps);
    const double q = r * rcp_(fabs_(a));
    L.lo = max_neg_raw(L.lo, keep_or_nan(pos, q));
    L.hi = min_raw(L.hi, keep_or_nan(neg, q));
    return a;
}
template <int X>
__device__ __forceinline__ double clip_partner8_lazy(LineQP<double>& L, double eps, double a0, double a1, double cc, double m0, double m1,
                                                     double mc) {
    return clip_row_coop_lazy(L, eps, group_xor8<double, X>(a0, m0), group_xor8<double, X>(a1, m1), group_xor8<double, X>(cc, mc));
}
// the seven partners in the order of clip_partners8; returns the smallest |a|
__device__ __forceinline__ double clip_partners8_lazy(LineQP<double>& L, double eps, double a0, double a1, double cc) {
    const double m0 = dpp_mov<0x141>(a0), m1 = dpp_mov<0x141>(a1), mc = dpp_mov<0x141>(cc);
    const double x1 = clip_partner8_lazy<1>(L, eps, a0, a1, cc, m0, m1, mc);
    const double x2 = clip_partner8_lazy<2>(L, eps, a0, a1, cc, m0, m1, mc);
    double amin = min_abs_abs_raw(x1, x2);
    amin = min_abs_raw(amin, clip_partner8_lazy<3>(L, eps, a0, a1, cc, m0, m1, mc));
    amin = min_abs_raw(amin, clip_partner8_lazy<4>(L, eps, a0, a1, cc, m0, m1, mc));
    amin = min_abs_raw(amin, clip_partner8_lazy<5>(L, eps, a0, a1, cc, m0, m1, mc));
    amin = min_abs_raw(amin, clip_partner8_lazy<6>(L, eps, a0, a1, cc, m0, m1, mc));
    amin = min_abs_raw(amin, clip_partner8_lazy<7>(L, eps, a0, a1, cc, m0, m1, mc));
    return amin;
}
// coop_pick_winner for 8 lanes per agent without the v_max(x, x) in front of lo, hi, |lo| and |hi|: the interval ends come out of
// the raw min / max of the clips (inline assembly, so the compiler cannot see that they are canonical); those return one of their
// operands or a quieted NaN, and their operands are products of arithmetic.  Operand order as the compiler emits it for the
// expressions of coop_pick_winner: max(lo, 0), then min(., hi); max(|lo|, |hi|), then max(., 1).
__device__ __forceinline__ void coop_pick_winner8_raw(QpState<double>& S, const LineQP<double>& L, bool ok, int sub, int lane,
                                                      const SolveLit<double>& lit) {
    using TC = double;
    const TC inf = num<TC>::inf();                                              // of the select, whose high word needs a VGPR anyway
    TC t = min_raw(max_zero_raw(L.lo), L.hi);
    const bool inverted = L.lo > L.hi;
    t = inverted ? TC(0.5) * (L.lo + L.hi) : t;
    const bool empty = L.lo > L.hi + lit.tol_feas * max_one_raw(max_abs_abs_raw(L.lo, L.hi));
    const TC v0 = L.p0 + t * L.d0, v1 = L.p1 + t * L.d1;
    const TC e0 = v0 - S.ur0, e1 = v1 - S.ur1;
    TC cost = e0 * e0 + e1 * e1;
    cost = (ok && !empty && (cost == cost)) ? cost : inf;
    const TC best = min8_raw(cost);
    bool has;
    const bool mine = group_first<8>(__builtin_amdgcn_ballot_w64((cost == best) && (best < lit.inf)), lane, sub, has);
    const TC s0 = group_pick<8>(mine, v0), s1 = group_pick<8>(mine, v1);
    S.u0 = has ? s0 : S.u0;
    S.u1 = has ? s1 : S.u1;
}

// coop_solve_all8 with every lane holding a row (K = 8: no `sub < K`) and every lane taken as ordinary.  Returns the lanes that
// met what this form does not handle -- a flat direction of the box clip or a partner row parallel to the line -- as a wave mask
// (a scalar: carried across the early-out as a lane flag it would be rebuilt through a VGPR).  A wave that does not enter the
// solve reports nothing, as it runs neither clip in coop_solve_all8.
template <typename TC>
__device__ __forceinline__ unsigned long long coop_solve_all8_fast(QpState<TC>& S, int sub, int lane, TC a0, TC a1, TC cc,
                                                     const CbfConsts<TC>& k, const SolveLit<TC>& lit) {
    const bool testable = !((a0 == TC(0)) && (a1 == TC(0)));
    LineQP<TC> L;
    const bool viol = qp_row_violated(S, a0, a1, cc, L, k) && testable;
    if (__builtin_amdgcn_ballot_w64(viol) == 0ull) return 0ull;
    clip_box_fast(L, k);
    const TC amin = clip_partners8_lazy(L, lit.eps_par, a0, a1, cc);
    coop_pick_winner8_raw(S, L, viol, sub, lane, lit);
    return __builtin_amdgcn_ballot_w64((L.d0 == TC(0)) || (L.d1 == TC(0)) || (amin <= lit.eps_par));
}

// The same for 16 lanes per agent (K <= 16; one DPP row per agent): fifteen partners by row_ror, reductions by quad permutes and
// the two mirrors.
template <typename TC, int... Rs>
__device__ __forceinline__ void clip_partners16(LineQP<TC>& L, bool& dead, TC a0, TC a1, TC cc, std::integer_sequence<int, Rs...>) {
    (clip_row_coop(L, dead, dpp_mov<0x121 + Rs>(a0), dpp_mov<0x121 + Rs>(a1), dpp_mov<0x121 + Rs>(cc)), ...);     // row_ror:1 .. row_ror:15
}
template <typename TC>
__device__ __forceinline__ void coop_solve_all16(QpState<TC>& S, int K, int sub, int lane, TC a0, TC a1, TC cc,
                                                 const CbfConsts<TC>& k) {
    const bool testable = (sub < K) && !((a0 == TC(0)) && (a1 == TC(0)));
    LineQP<TC> L;
    const bool viol = qp_row_violated(S, a0, a1, cc, L, k) && testable;
    if (__builtin_amdgcn_ballot_w64(viol) == 0ull) return;
    clip_box(L, k);
    bool dead = false;
    clip_partners16(L, dead, a0, a1, cc, std::make_integer_sequence<int, 15>{});
    coop_pick_winner<TC, 16>(S, L, viol && !dead, sub, lane);
}

}  // namespace sc
