// Fused batched CBF-QP for gfx950: one launch = row assembly + exact QP solve
// + status + h(x) for B agents.  Replaces the per-robot Python path
//   CBFQP.solve_control_problem   position_control/cbf_qp.py:108-199
//   robot.agent_barrier / f / g    robots/robot.py:389-436
//   cvxpy -> GUROBI                position_control/cbf_qp.py:190
//
// Mapping: one QP per lane, one 64-agent wave per workgroup.  The wave's
// obstacle rows (64 x K x 7 contiguous values in the reference's [B,K,7]
// layout) are streamed HBM -> LDS with 16-byte LDS-DMA (global_load_lds, 1 KiB
// per wave instruction, no VGPR round trip) and read back per lane; X / u_ref
// / outputs are plain coalesced vector accesses.  All rows live in registers;
// the solve is sc_qp2.hpp.  HBM traffic is exactly the algorithmic bytes
// (every input read once, every output written once).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include <cstdlib>

#include "sc_qp2.hpp"
#include "sc_group.hpp"
#include "sc_agent_params.hpp"

namespace sc {

// batches up to this many agents use the cooperative (8 lanes per agent) kernel: below it the
// lane-per-QP kernel cannot fill the chip (65536 agents = 1024 waves = one per SIMD)
#ifndef SC_COOP_MAX_AGENTS
#define SC_COOP_MAX_AGENTS 32768
#endif

// test / profiling hook: SC_FORCE_LDS_KERNEL=1 routes K > 8 to the LDS-staged kernel instead of the
// row-per-lane kernel
static inline long long sc_coop_max_agents() {             // SC_COOP_MAX_AGENTS=<n> overrides the compiled default
    static const long long v = [] { const char* e = getenv("SC_COOP_MAX_AGENTS"); return e ? atoll(e) : (long long)SC_COOP_MAX_AGENTS; }();
    return v;
}
static inline bool sc_two_pass() {                         // SC_CBFQP_TWO_PASS=0: the single-launch register kernel for every model
    static const bool v = [] { const char* e = getenv("SC_CBFQP_TWO_PASS"); return !(e && e[0] == '0'); }();
    return v;
}
static inline bool sc_force_lds_kernel() {
    static const bool v = [] { const char* e = getenv("SC_FORCE_LDS_KERNEL"); return e && e[0] == '1'; }();
    return v;
}

using as1_void = const __attribute__((address_space(1))) void;
using as3_void = __attribute__((address_space(3))) void;

// State row -> (x0..x4) in the compute type.  4-state models: two 8/16-byte loads; Quad2D: six values per row, five of them used.
// The loads (load_state) and the conversion with its sincos (to_agent) are separate so that a kernel can issue every input load
// before it waits for any of them.
template <typename TIO, int MODEL>
struct StateRow { TIO v[MODEL == SC_MODEL_QUAD2D ? 5 : 4]; };

template <typename TIO, int MODEL>
__device__ __forceinline__ StateRow<TIO, MODEL> load_state(const TIO* __restrict__ X, long long agent) {
    StateRow<TIO, MODEL> s;
    if constexpr (MODEL == SC_MODEL_QUAD2D) {
        const TIO* r = X + agent * 6;
#pragma unroll
        for (int i = 0; i < 5; ++i) s.v[i] = r[i];
    } else {
        const TIO* r = X + agent * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) s.v[i] = r[i];
    }
    return s;
}

template <typename TIO, typename TC, int MODEL>
__device__ __forceinline__ Agent<TC> to_agent(const StateRow<TIO, MODEL>& s) {
    if constexpr (MODEL == SC_MODEL_QUAD2D) return make_agent_m<TC, MODEL>(TC(s.v[0]), TC(s.v[1]), TC(s.v[2]), TC(s.v[3]), TC(s.v[4]));
    else return make_agent_m<TC, MODEL>(TC(s.v[0]), TC(s.v[1]), TC(s.v[2]), TC(s.v[3]));
}

template <typename TIO, typename TC, int MODEL>
__device__ __forceinline__ Agent<TC> load_agent(const TIO* __restrict__ X, long long agent) {
    return to_agent<TIO, TC, MODEL>(load_state<TIO, MODEL>(X, agent));
}

// By-value kernel arguments past the preloaded ones are read with scalar loads, which the compiler sinks to each argument's first
// use: one cold round trip to the argument block after another, each behind the input loads' wait.  Naming a value here makes its
// load issue at this point instead, i.e. while the input loads are in flight.
template <typename T>
__device__ __forceinline__ void fetch_arg_now(const T& v) { asm volatile("" ::"s"(v)); }

template <typename TIO> struct vec2;
template <> struct vec2<float> { using type = float2; };
template <> struct vec2<double> { using type = double2; };

// Stage `bytes` contiguous bytes (multiple of 16, 16-byte aligned) from global
// to LDS with the wave's 64 lanes, 1 KiB per instruction.
__device__ __forceinline__ void wave_dma16(const unsigned char* __restrict__ src, unsigned char* lds,
                                           unsigned bytes, int lane) {
    const unsigned n16 = bytes >> 4;
    for (unsigned base = 0; base < n16; base += 64) {
        const unsigned idx = base + lane;
        if (idx < n16) {
            __builtin_amdgcn_global_load_lds((as1_void*)(src + (size_t)idx * 16),
                                             (as3_void*)(lds + (size_t)base * 16), 16, 0, 0);
        }
    }
}

// ======================================================================================
// K <= 8: register kernel.  No LDS at all: each lane pulls its own agent's K x 7 obstacle
// values straight into VGPRs with 16-byte loads (the block is contiguous and 16-byte aligned
// in the reference's [B,K,7] layout; every byte of every cache line is consumed by the lanes
// that touch it, the 8 partial touches of a line merge in the vector L1), builds the rows in
// registers with the row loop unrolled, and runs the unrolled walk.  With no LDS footprint the
// occupancy is set by VGPRs only, which is what hides the HBM latency of a pure streaming pass.
template <typename TIO> struct vec4io;
template <> struct vec4io<float> { using type = float4; static constexpr int N = 4; };
template <> struct vec4io<double> { using type = double2; static constexpr int N = 2; };

// PASS (DynamicUnicycle2D with f64 arithmetic only; 0 everywhere else = the plain one-launch kernel):
//   1  circles-only fast pass: a wave that finds any obstacle flag != 0 among its agents' rows writes SC_STATUS_PENDING for
//      them and leaves; every other wave runs a body WITHOUT the out-of-line superellipsoid call -- 166 instead of 195 VGPRs
//      (three waves per SIMD instead of two), no spilled SGPRs: 1.55 -> 1.35 ms at 2^24 agents;
//   2  the generic body for exactly the waves pass 1 deferred (it reads status_out first; the others leave at once).
#define SC_STATUS_PENDING (-1)
template <typename TIO, typename TC, int KMAX, int MODEL, int PASS = 0>
__global__ __launch_bounds__(256) void cbfqp_reg_kernel(const TIO* __restrict__ obs, const TIO* __restrict__ X,
                                                        const TIO* __restrict__ u_ref, const int* __restrict__ n_obs,
                                                        const long long B, const int K, const int obs_shared,
                                                        TIO* __restrict__ u_out, int* __restrict__ status_out,
                                                        TIO* __restrict__ h_out, const CbfConsts<TC> k) {
    const long long agent = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = agent < B;
    const long long ag_i = active ? agent : 0;           // inactive lanes compute on agent 0, store nothing
    using V2 = typename vec2<TIO>::type;
    using V4 = typename vec4io<TIO>::type;
    constexpr int VN = vec4io<TIO>::N;
    if constexpr (PASS == 2) {
        const bool pending = active && status_out[ag_i] == SC_STATUS_PENDING;
        if (__builtin_amdgcn_ballot_w64(pending) == 0ull) return;          // wave-uniform: pass 1 finished this wave
    }

    // ---- loads: obstacles first (longest latency), then state ---------------------------
    TIO flat[KMAX * 7];
    const TIO* src = obs + (obs_shared ? 0 : (size_t)ag_i * K * 7);
    if (K == KMAX && ((KMAX * 7) % VN == 0) && ((reinterpret_cast<uintptr_t>(obs) & 15u) == 0) &&
        ((KMAX * 7 * sizeof(TIO)) % 16 == 0)) {
        const V4* s4 = reinterpret_cast<const V4*>(src);
#pragma unroll
        for (int e = 0; e < KMAX * 7 / VN; ++e) {
            const V4 q = s4[e];
            if constexpr (VN == 4) {
                flat[e * 4 + 0] = q.x; flat[e * 4 + 1] = q.y; flat[e * 4 + 2] = q.z; flat[e * 4 + 3] = q.w;
            } else {
                flat[e * 2 + 0] = q.x; flat[e * 2 + 1] = q.y;
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < KMAX; ++r) {
#pragma unroll
            for (int f = 0; f < 7; ++f) flat[r * 7 + f] = (r < K) ? src[r * 7 + f] : TIO(0);
        }
    }
    const V2 ur = reinterpret_cast<const V2*>(u_ref)[ag_i];
    const StateRow<TIO, MODEL> xs = load_state<TIO, MODEL>(X, ag_i);
    int nk = K;
    if (n_obs) nk = n_obs[ag_i];                           // issued with the other loads; clamped once they are all in flight
    nk = nk < 0 ? 0 : (nk > K ? K : nk);
    if constexpr (PASS == 1) {
        bool other = false;
#pragma unroll
        for (int r = 0; r < KMAX; ++r) other |= (r < nk) && (flat[r * 7 + 6] != TIO(0));
        if (__builtin_amdgcn_ballot_w64(other && active) != 0ull) {        // wave-uniform: leave this wave to pass 2
            if (active) status_out[agent] = SC_STATUS_PENDING;
            return;
        }
    }
    const TC ur0 = TC(ur.x), ur1 = TC(ur.y);
    const Agent<TC> ag = to_agent<TIO, TC, MODEL>(xs);

    // ---- rows: agent_barrier + cbf_qp.py:155-183, unrolled, in registers ------------------
    TC n0[KMAX], n1[KMAX], c[KMAX];
    TIO hv[KMAX];
    bool bad_obs = false;
    TC poison = TC(0);
#pragma unroll
    for (int r = 0; r < KMAX; ++r) {
        TC o[7];
#pragma unroll
        for (int f = 0; f < 7; ++f) o[f] = TC(flat[r * 7 + f]);
        TC h, a0, a1, cc;
        const bool ok = cbf_row<TC, MODEL, true, PASS == 1>(ag, o, k, a0, a1, cc, h);
        const bool used = r < nk;                   // nk <= K <= KMAX
        bad_obs |= used && !ok;
        a0 = used ? a0 : TC(0); a1 = used ? a1 : TC(0); cc = used ? cc : TC(0);
        normalise_row(a0, a1, cc, poison);
        n0[r] = a0; n1[r] = a1; c[r] = cc;
        hv[r] = used ? TIO(h) : TIO(0);
    }

    // ---- solve + outputs --------------------------------------------------------------------
    TC u0, u1;
    int st = qp2_solve<TC, KMAX>(n0, n1, c, K, ur0, ur1, poison, k, u0, u1);
    if (bad_obs) st = SC_STATUS_BAD_OBSTACLE;
    if (st != SC_STATUS_OPTIMAL) { u0 = num<TC>::nan(); u1 = num<TC>::nan(); }
    if (active) {
        V2 uo; uo.x = TIO(u0); uo.y = TIO(u1);
        reinterpret_cast<V2*>(u_out)[agent] = uo;
        status_out[agent] = st;
        if (h_out) {
            TIO* hp = h_out + agent * K;
            if (K == KMAX && (KMAX % VN == 0) && ((reinterpret_cast<uintptr_t>(h_out) & 15u) == 0)) {
                V4* h4 = reinterpret_cast<V4*>(hp);
#pragma unroll
                for (int e = 0; e < KMAX / VN; ++e) {
                    V4 q;
                    if constexpr (VN == 4) { q.x = hv[e * 4]; q.y = hv[e * 4 + 1]; q.z = hv[e * 4 + 2]; q.w = hv[e * 4 + 3]; }
                    else { q.x = hv[e * 2]; q.y = hv[e * 2 + 1]; }
                    h4[e] = q;
                }
            } else {
#pragma unroll
                for (int r = 0; r < KMAX; ++r) if (r < K) hp[r] = hv[r];
            }
        }
    }
}

// ======================================================================================
// K <= 8, small batches: cooperative kernel, 8 lanes per agent (one obstacle row per lane).
//
// At BASELINE's 4096-agent batch the lane-per-QP kernel runs 64 waves on a chip with 1024 SIMDs and
// its time is one wave's instruction stream (~1700 VALU).  Here an agent is spread over 8 lanes:
// each lane builds ONE row, the incremental walk broadcasts row i inside the 8-lane group, every
// lane clips the line against its own row in parallel, and the interval ends are combined with
// three xor-shuffle steps.  512 waves instead of 64, each ~4x shorter; with only 8 agents per wave
// the wave-uniform "nobody violates row i" skip fires most of the time.  Arithmetic per row is the
// same code as the lane-per-QP kernel (min/max reductions are exact), so both give the same answer.
// G lanes per agent (G = 8, 16 or 32 >= K), 64 / G agents per wave.
// Parameters are in order of first use: the first 14 dwords (obs .. u_out) arrive in SGPRs at wave start (kernel-argument
// preloading, FLAGS_cbf_qp_* in the Makefile), so the input loads go out without a scalar-load round trip in front of them; the
// rest is fetched while those loads are in flight.  The other two kernels of this file keep the same order.
template <typename TIO, typename TC, int G, int MODEL>
#ifndef SC_COOP_WAVES
#define SC_COOP_WAVES 1                                   // waves per workgroup of the cooperative kernel (developer builds time 2 and 4)
#endif
__global__ __launch_bounds__(64 * SC_COOP_WAVES) void cbfqp_coop_kernel(const TIO* __restrict__ obs, const TIO* __restrict__ X,
                                                        const TIO* __restrict__ u_ref, const int* __restrict__ n_obs,
                                                        const long long B, const int K, const int obs_shared,
                                                        TIO* __restrict__ u_out, int* __restrict__ status_out,
                                                        TIO* __restrict__ h_out, const CbfConsts<TC> k) {
    // Developer builds only (tools/README.md): the attribution ladder of DESIGN.md 1b.  SC_EXP_EMPTY: the same grid with no body;
    // SC_EXP_ARGS: the kernel arguments and one store that depends on them; SC_EXP_LOADS: the input loads and the product's stores.
#ifdef SC_EXP_EMPTY
    return;
#endif
    constexpr int APW = 64 / G;                            // agents per wave
    const int lane = threadIdx.x & 63;
    const int sub = lane & (G - 1);                        // obstacle row handled by this lane
    const long long agent = ((long long)blockIdx.x * SC_COOP_WAVES + (threadIdx.x >> 6)) * APW + lane / G;
    const bool active = agent < B;
    const long long ag_i = active ? agent : 0;
    using V2 = typename vec2<TIO>::type;
#ifdef SC_EXP_ARGS
    if (active && sub == 0)
        status_out[agent] = (int)((reinterpret_cast<uintptr_t>(obs) ^ reinterpret_cast<uintptr_t>(X) ^ reinterpret_cast<uintptr_t>(u_ref) ^
                                   reinterpret_cast<uintptr_t>(n_obs) ^ reinterpret_cast<uintptr_t>(u_out) ^ reinterpret_cast<uintptr_t>(h_out)) >> 4) + K + obs_shared;
    return;
#endif

    TIO orow[7];
    const bool has_row = sub < K;
    const TIO* src = obs + (obs_shared ? 0 : (size_t)ag_i * K * 7) + (has_row ? sub * 7 : 0);
#pragma unroll
    for (int f = 0; f < 7; ++f) orow[f] = src[f];
    const V2 ur = reinterpret_cast<const V2*>(u_ref)[ag_i];
    const StateRow<TIO, MODEL> xs = load_state<TIO, MODEL>(X, ag_i);
    int nk = K;
    if (n_obs) nk = n_obs[ag_i];                           // issued with the other loads; clamped once they are all in flight
    nk = nk < 0 ? 0 : (nk > K ? K : nk);
    fetch_arg_now(status_out); fetch_arg_now(h_out);
    fetch_arg_now(k.R); fetch_arg_now(k.g1); fetch_arg_now(k.g2);
    fetch_arg_now(k.lo0); fetch_arg_now(k.hi0); fetch_arg_now(k.lo1); fetch_arg_now(k.hi1); fetch_arg_now(k.hard);
#ifdef SC_EXP_LOADS
    if (active) {
        if (sub == 0) {
            V2 uo; uo.x = ur.x + xs.v[0] + xs.v[1]; uo.y = ur.y + xs.v[2] + xs.v[3];
            reinterpret_cast<V2*>(u_out)[agent] = uo;
            status_out[agent] = nk;
        }
        if (h_out && has_row) h_out[agent * K + sub] = orow[0] + orow[1] + orow[2] + orow[3] + orow[4] + orow[5] + orow[6];
    }
    return;
#endif
    // From here to the stores this body has a second copy: coop8_generic_body below restates it, function by function, for the
    // waves that leave the specialised kernel's fast path, and must return the same bits (tests/test_cbfqp_exits_gpu.py).  A
    // change to the sequence here is mirrored there.
    const TC ur0 = TC(ur.x), ur1 = TC(ur.y);
    const Agent<TC> ag = to_agent<TIO, TC, MODEL>(xs);

    // ---- this lane's row -------------------------------------------------------------------
    TC o[7];
#pragma unroll
    for (int f = 0; f < 7; ++f) o[f] = TC(orow[f]);
    TC h, a0, a1, cc;
#ifndef SC_EXP_NOROW
    const bool ok = cbf_row<TC, MODEL, false>(ag, o, k, a0, a1, cc, h);
#else
    const bool ok = true; a0 = o[0] - ag.x; a1 = o[1] - ag.y; cc = o[2]; h = o[3];
#endif
    const bool used = sub < nk;
    const bool bad_mine = used && !ok;
    a0 = used ? a0 : TC(0); a1 = used ? a1 : TC(0); cc = used ? cc : TC(0);
    // h(x) is final here: its store (two thirds of the launch's output bytes) leaves before the solve, not after it
    if (active && h_out && has_row) h_out[agent * K + sub] = used ? TIO(h) : TIO(0);
    TC poison = TC(0);
    normalise_row(a0, a1, cc, poison);

    // ---- cooperative walk ----------------------------------------------------------------------
    QpState<TC> S;
    qp_begin(S, ur0, ur1, k);
#ifndef SC_EXP_NOWALK                                     // developer builds only (tools/README.md): what the solve costs in the launch
#ifndef SC_COOP_OLD_WALK
    if constexpr (G == 8) coop_solve_all8<TC>(S, K, sub, lane, a0, a1, cc, k);          // fixed critical path (sc_group.hpp)
    else if constexpr (G == 16) coop_solve_all16<TC>(S, K, sub, lane, a0, a1, cc, k);
    else
#endif
    coop_walk_violated<TC, G>(S, K, sub, lane, a0, a1, cc, k);
#endif
    qp_finish_box(S, k);
    TC worst = qp_row_margin(num<TC>::inf(), a0, a1, cc, S.u0, S.u1, poison);
    // NaN anywhere in the group must make the status infeasible, and min() drops NaN: a poisoned lane enters the minimum as -inf,
    // which fails the slack check as the NaN did.  The group's bad-obstacle flags are its byte (G bits) of the wave's ballot.
    const bool nan_mine = !(poison == poison);
    worst = nan_mine ? -num<TC>::inf() : worst;
    if constexpr (G == 8) worst = min8_raw(worst);
    else if constexpr (G == 16) worst = min16_raw(worst);
    else worst = group_min<TC, G>(worst);
    const unsigned long long bad_mask = __builtin_amdgcn_ballot_w64(bad_mine);
    const bool bad_any = ((bad_mask >> (lane & ~(G - 1))) & (G == 64 ? ~0ull : ((1ull << G) - 1ull))) != 0ull;
    int st = qp_status(S, worst, TC(0), k);
    if (bad_any) st = SC_STATUS_BAD_OBSTACLE;
    TC u0 = S.u0, u1 = S.u1;
    if (st != SC_STATUS_OPTIMAL) { u0 = num<TC>::nan(); u1 = num<TC>::nan(); }
    if (active) {
        if (sub == 0) {
            V2 uo; uo.x = TIO(u0); uo.y = TIO(u1);
            reinterpret_cast<V2*>(u_out)[agent] = uo;
            status_out[agent] = st;
        }
    }
}

// ======================================================================================
// The cooperative kernel above specialised for the headline launch: DynamicUnicycle2D, f64 arithmetic, exactly 8 rows per
// agent, per-agent obstacles, no n_obs.  The generic kernel decides all of that at run time inside every wave; a lone wave per
// SIMD pays for each executed instruction, so what the host knows before the launch is a template parameter or is
// absent here:
//   * K = 8 = lanes per agent: every lane has a row, every row is used (no has_row, no nk clamp, no selects of a0 / a1 / cc / h);
//   * offsets are 32-bit: lane `slot` = blockIdx * 64 + lane owns row `slot` of obs[B, 8, 7] and entry `slot` of h_out[B, 8]
//     (launch_coop checks that the byte offsets fit);
//   * FULL: B is a multiple of the 8 agents of a wave, so there is no `active` guard at all; !FULL keeps it (c.B);
//   * HAS_H: h_out is non-null;
//   * the obstacle row arrives with two loads (16 + 12 bytes, f32 storage) instead of seven;
//   * the f64 sincos reads its sixteen constants, and the solve its literals (SolveLit), from the argument block;
//   * every lane is taken as ordinary: a circle (flag 0), |theta| < 1e5 (the table sincos), a row with nn > 0, no flat direction of
//     the box clip, no partner row parallel to its line -- and the min / max of values that cannot be signalling NaNs skip the
//     canonicalising v_max(x, x) (sc_group.hpp, "the solve of the specialised K = 8 kernel").
// A wave that holds a lane which is not ordinary leaves the fast path through one of two wave-uniform exits, and both lead to the
// same place: the generic K = 8 sequence for the whole wave (coop8_generic_body: the functions cbfqp_coop_kernel calls, in its order,
// on the inputs this kernel has loaded), which stores h itself and hands u and status to the kernel's store.
//   * early exit, as soon as the inputs have landed: some lane's flag is not 0, or not |theta| < 1e5 (a NaN included: the arm
//     sincos_ takes for it).  Both are visible in the inputs, so such a wave -- a fleet among superellipsoids -- pays for no fast path;
//   * late exit, one scalar test in front of the u / status stores: some lane met a row without nn > 0, a flat direction or a
//     parallel partner.  The flag is an OR of wave masks that only grows, so a predicate computed from state an earlier oddity has spoiled cannot clear
//     it; the row test sits in front of the solve's own early-out, which therefore cannot bypass it.  The fast path may have stored
//     an h by then: the generic sequence stores it again, and the later store to the same address wins.  A flag that is neither 0
//     nor 1 (the bad obstacle) is a flag that is not 0: it leaves through the early exit.
// On an ordinary wave both branches fall through and no cold code lies between the entry and s_endpgm (tools/coop8_path_count.py).
// Arithmetic and its order on the fast path are those of the generic kernel, so both return the same bits
// (tests/test_cbfqp_special_gpu.py, tests/test_cbfqp_exits_gpu.py).
// Six pointers in order of first use are preloaded (12 dwords); n_obs, B, K and obs_shared are not arguments.
// The constants travel as four 64-byte vectors so that a wave fetches them with four scalar loads (field by field the compiler
// emits one load per double: two dozen executed instructions).  Filled by launch_coop8_du, taken apart at the top of the kernel.
typedef double sc_d8 __attribute__((ext_vector_type(8)));
struct Coop8Consts {
    sc_d8 t0;                                              // SinCosTab: two_over_pi, pio2_1, pio2_2, pio2_3, s[0..3]
    sc_d8 t1;                                              //            s[4], s[5], c[0..5]
    sc_d8 k0;                                              // R, g1, g2, inv_dt, inv_dt2, lo0, hi0, lo1
    sc_d8 k1;                                              // hi1; SolveLit: th_max, neg_beta; two spares; tol_feas, eps_par, +inf
    unsigned B;                                            // read by the !FULL instantiations only
};

// The circle row of cbf_row<double, DynamicUnicycle2D> (hocbf_circle and the tail of cbf_row) with every sum of products written
// as the fused form the generic kernel compiles to.  `x * y + z * w` leaves it to the compiler which product stays a rounded
// multiply and which goes into the FMA, and the choice depends on the surrounding code: outside cbf_row's flag branches it picks
// the other product for Lf, and the two differ in the last bit of some rows.  The forms below are read, sum by sum, from the
// gfx950 listing of cbfqp_coop_kernel<float, double, 8, 0> (x * y + z * w in source order; "rounded" is the plain multiply):
//   ex ex + ey ey       fma(ex, ex, ey * ey)          first product fused, second rounded
//   (..) - beta dmin^2  fma(dmin, dmin * -1.01, ..)   dmin * -1.01 rounded ( = -(1.01 dmin) exactly), then fused with dmin
//   hdot                2 fma(ex, f0, ey * f1)        first fused, second rounded
//   n1 = dhd[2]         2 fma(ey, f0, -(ex * f1))     the SECOND product fused; the first, ex * (-f1), rounded, its sign folded
//   n0 = dhd[3]         2 fma(ex, c, ey * s)          first fused, second rounded
//   Lf                  fma(dhd0, f0, dhd1 * f1)      first fused, second rounded
//   c, soft             fma(g2, h, fma(g1, hdot, Lf)) ; c, hard: fma(h, inv_dt2, (2 hdot) inv_dt) + Lf, the last a plain add
// 2 x is x + x exactly, so where the factor 2 is applied does not matter.
template <bool HARD>
__device__ __forceinline__ void circle_row_du_as_generic(const Agent<double>& a, const double* o, const CbfConsts<double>& k,
                                                         double neg_beta, double& n0, double& n1, double& c, double& h) {
    const double ex = a.x - o[0], ey = a.y - o[1];
    const double dmin = o[2] + k.R;
    h = __builtin_fma(dmin, dmin * neg_beta, __builtin_fma(ex, ex, ey * ey));
    const double hdot = 2.0 * __builtin_fma(ex, a.f0, ey * a.f1);
    const double dhd0 = 2.0 * a.f0, dhd1 = 2.0 * a.f1;
    n1 = 2.0 * __builtin_fma(ey, a.f0, -(ex * a.f1));      // dhd[2] = 2 (ex (-f1) + ey f0)
    n0 = 2.0 * __builtin_fma(ex, a.c, ey * a.s);           // dhd[3]
    const double Lf = __builtin_fma(dhd0, a.f0, dhd1 * a.f1);
    if constexpr (HARD) c = __builtin_fma(h, k.inv_dt2, (2.0 * hdot) * k.inv_dt) + Lf;
    else c = __builtin_fma(k.g2, h, __builtin_fma(k.g1, hdot, Lf));
}

// normalise_row with the sum of squares written as the fused form the generic kernel compiles to (behind its `used` selects the
// compiler picks fma(n1, n1, n0 * n0), without them the other one) and without the guard `nn > 0 ? rsqrt_(nn) : 1`: a row without
// nn > 0 (all-zero, underflowed, NaN) is reported, and its wave runs normalise_row itself (coop8_generic_body).
__device__ __forceinline__ bool normalise_row_fast(double& n0, double& n1, double& c, double& poison) {
    const double nn = __builtin_fma(n1, n1, n0 * n0);
    poison += 0.0 * (nn + c);
    const double inv = rsqrt_(nn);
    n0 *= inv; n1 *= inv; c *= inv;
    return !(nn > 0.0);
}

// base + off bytes, off a 32-bit lane value: the scalar-base form of the global loads and stores (no 64-bit address arithmetic)
template <typename T>
__device__ __forceinline__ T* at_byte(T* base, unsigned off) {
    using C = typename std::conditional<std::is_const<T>::value, const char, char>::type;
    return reinterpret_cast<T*>(reinterpret_cast<C*>(base) + off);
}

// Where both exits of cbfqp_coop8_du_kernel lead: the body of cbfqp_coop_kernel<TIO, double, 8, DynamicUnicycle2D> from the loaded
// inputs to its stores, restated from the same device functions in the same order.  K and nk are 8 here, but they are handed
// over as run-time values (an empty asm), as they are in that kernel: its `used` and `sub < K` selects then stay in place, and with
// them the way the compiler fuses the sums of products behind them (see normalise_row_fast), which is what keeps the bits.
template <typename TIO, bool HAS_H>
__device__ __forceinline__ void coop8_generic_body(const TIO* orow, typename vec2<TIO>::type ur,
                                                   const StateRow<TIO, SC_MODEL_DYNAMIC_UNICYCLE2D>& xs, bool active,
                                                   unsigned slot, int sub, int lane, const CbfConsts<double>& k,
                                                   TIO* __restrict__ h_out, typename vec2<TIO>::type& uo, int& st) {
    using TC = double;
    constexpr int MODEL = SC_MODEL_DYNAMIC_UNICYCLE2D;
    int K = 8, nk = 8;
    asm volatile("" : "+s"(K), "+s"(nk));
    const TC ur0 = TC(ur.x), ur1 = TC(ur.y);
    const Agent<TC> ag = to_agent<TIO, TC, MODEL>(xs);
    TC o[7];
#pragma unroll
    for (int f = 0; f < 7; ++f) o[f] = TC(orow[f]);
    TC h, a0, a1, cc;
    const bool ok = cbf_row<TC, MODEL, false>(ag, o, k, a0, a1, cc, h);
    const bool used = sub < nk;
    const bool bad_mine = used && !ok;
    a0 = used ? a0 : TC(0); a1 = used ? a1 : TC(0); cc = used ? cc : TC(0);
    if constexpr (HAS_H) {
        if (active && sub < K) *at_byte(h_out, slot * (unsigned)sizeof(TIO)) = used ? TIO(h) : TIO(0);
    }
    TC poison = TC(0);
    normalise_row(a0, a1, cc, poison);
    QpState<TC> S;
    qp_begin(S, ur0, ur1, k);
    coop_solve_all8<TC>(S, K, sub, lane, a0, a1, cc, k);
    qp_finish_box(S, k);
    TC worst = qp_row_margin(num<TC>::inf(), a0, a1, cc, S.u0, S.u1, poison);
    const bool nan_mine = !(poison == poison);
    worst = nan_mine ? -num<TC>::inf() : worst;
    worst = min8_raw(worst);
    const unsigned long long bad_mask = __builtin_amdgcn_ballot_w64(bad_mine);
    const bool bad_any = ((bad_mask >> (lane & ~7)) & 0xffull) != 0ull;
    st = qp_status(S, worst, TC(0), k);
    if (bad_any) st = SC_STATUS_BAD_OBSTACLE;
    TC u0 = S.u0, u1 = S.u1;
    if (st != SC_STATUS_OPTIMAL) { u0 = num<TC>::nan(); u1 = num<TC>::nan(); }
    uo.x = TIO(u0); uo.y = TIO(u1);
}

template <typename TIO, bool FULL, bool HAS_H, bool HARD>
__global__ __launch_bounds__(64) void cbfqp_coop8_du_kernel(const TIO* __restrict__ obs, const TIO* __restrict__ X,
                                                            const TIO* __restrict__ u_ref, TIO* __restrict__ u_out,
                                                            TIO* __restrict__ h_out, int* __restrict__ status_out,
                                                            const Coop8Consts c) {
#ifdef SC_EXP_EMPTY
    return;
#endif
    using TC = double;
    using V2 = typename vec2<TIO>::type;
    const unsigned lane = threadIdx.x;
    const unsigned sub = lane & 7u;
    const unsigned slot = blockIdx.x * 64u + lane;         // agent * 8 + sub
    const unsigned agent = slot >> 3;
    bool active = true;
    if constexpr (!FULL) active = agent < c.B;
    const unsigned row_i = active ? slot : sub;            // inactive lanes compute on agent 0, store nothing
    const unsigned ag8 = row_i & ~7u;                      // agent * 8

    // byte offsets as 32-bit lane values on the scalar bases; launch_coop admits only batches whose slot fits 24 bits
    struct { TIO v[7]; } orow;
    __builtin_memcpy(&orow, at_byte(obs, __umul24(row_i, 7u * (unsigned)sizeof(TIO))), sizeof(orow));
    const V2 ur = *reinterpret_cast<const V2*>(at_byte(u_ref, ag8 * (unsigned)(sizeof(V2) / 8)));
    StateRow<TIO, SC_MODEL_DYNAMIC_UNICYCLE2D> xs;
    __builtin_memcpy(&xs, at_byte(X, ag8 * (unsigned)(sizeof(xs) / 8)), sizeof(xs));
    fetch_arg_now(c.t0); fetch_arg_now(c.t1); fetch_arg_now(c.k0); fetch_arg_now(c.k1);

    CbfConsts<TC> k;                                       // the fields cbf_row<DynamicUnicycle2D> and the solve read; the rest is never looked at
    k.R = c.k0[0]; k.a1 = TC(0); k.a2 = TC(0); k.g1 = c.k0[1]; k.g2 = c.k0[2]; k.inv_dt = c.k0[3]; k.inv_dt2 = c.k0[4];
    k.lo0 = c.k0[5]; k.hi0 = c.k0[6]; k.lo1 = c.k0[7]; k.hi1 = c.k1[0]; k.inv_Lr = TC(0); k.inv_mass = TC(1); k.hard = HARD;
    SolveLit<TC> lit;
    lit.th_max = c.k1[1]; lit.neg_beta = c.k1[2]; lit.tol_feas = c.k1[5]; lit.eps_par = c.k1[6]; lit.inf = c.k1[7];

    // ---- early exit: a flag other than 0, or the library arm of sincos_ (its own test, so a NaN theta goes where it sends it) ----
    const TC th = TC(xs.v[2]);
    const bool early = (orow.v[6] != TIO(0)) || !(fabs(th) < lit.th_max);
    const auto store_u_status = [&](V2 uo, int st) {
        if (active && sub == 0) {
            reinterpret_cast<V2*>(u_out)[agent] = uo;
            status_out[agent] = st;
        }
    };
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(early) != 0ull, 0)) {
        V2 uo; int st;
        coop8_generic_body<TIO, HAS_H>(orow.v, ur, xs, active, slot, (int)sub, (int)lane, k, h_out, uo, st);
        store_u_status(uo, st);
        return;
    }
    SinCosTab sc;
    sc.two_over_pi = c.t0[0]; sc.pio2_1 = c.t0[1]; sc.pio2_2 = c.t0[2]; sc.pio2_3 = c.t0[3];
    sc.s[0] = c.t0[4]; sc.s[1] = c.t0[5]; sc.s[2] = c.t0[6]; sc.s[3] = c.t0[7]; sc.s[4] = c.t1[0]; sc.s[5] = c.t1[1];
#pragma unroll
    for (int i = 0; i < 6; ++i) sc.c[i] = c.t1[2 + i];
    const TC ur0 = TC(ur.x), ur1 = TC(ur.y);
    Agent<TC> ag;                                      // make_agent with the constants of its sincos from the argument block
    ag.x = TC(xs.v[0]); ag.y = TC(xs.v[1]); ag.th = th; ag.v = TC(xs.v[3]);
    sincos_tab_sfma(ag.th, sc, &ag.s, &ag.c);
    ag.f0 = ag.v * ag.c;
    ag.f1 = ag.v * ag.s;

    // ---- this lane's row: a circle --------------------------------------------------------
    TC o[3];
#pragma unroll
    for (int f = 0; f < 3; ++f) o[f] = TC(orow.v[f]);
    TC h, a0, a1, cc;
    circle_row_du_as_generic<HARD>(ag, o, k, lit.neg_beta, a0, a1, cc, h);
    if constexpr (HAS_H) {
        if (active) *at_byte(h_out, slot * (unsigned)sizeof(TIO)) = TIO(h);
    }
    TC poison = TC(0);
    const unsigned long long odd_row = __builtin_amdgcn_ballot_w64(normalise_row_fast(a0, a1, cc, poison));

    // ---- the solve, the slack check and the outputs: as in cbfqp_coop_kernel ----------------
    // The *_raw forms (sc_group.hpp) are qp_begin / qp_finish_box / qp_row_margin without the canonicalising v_max(x, x): the
    // box bounds arrive quieted (launch_coop8_du), everything else here is converted from storage or the result of arithmetic.
    QpState<TC> S;
    qp_begin_raw(S, ur0, ur1, k);
    const unsigned long long odd_solve = coop_solve_all8_fast<TC>(S, (int)sub, (int)lane, a0, a1, cc, k, lit);
    qp_finish_box_raw(S, k);
    TC worst = qp_row_margin_raw(a0, a1, cc, S.u0, S.u1, poison, lit);
    const bool nan_mine = !(poison == poison);
    worst = nan_mine ? -num<TC>::inf() : worst;
    worst = min8_raw(worst);
    int st = qp_status_lit(S, worst, TC(0), k, lit);
    TC u0 = S.u0, u1 = S.u1;
    if (st != SC_STATUS_OPTIMAL) { u0 = num<TC>::nan(); u1 = num<TC>::nan(); }
    V2 uo; uo.x = TIO(u0); uo.y = TIO(u1);
    // ---- late exit: the lanes' flags as wave masks, so that the test is one scalar OR and one branch; the generic sequence
    // replaces u and status, which nothing has stored yet, and stores its own h over the fast path's ----------------------
    if (__builtin_expect((odd_row | odd_solve) != 0ull, 0))
        coop8_generic_body<TIO, HAS_H>(orow.v, ur, xs, active, slot, (int)sub, (int)lane, k, h_out, uo, st);
    store_u_status(uo, st);
}


// Developer builds only (tools/README.md): -DSC_EXP_GRID=n launches n workgroups whatever the batch, to time the wave-launch ramp
// of an empty node.  Only a kernel without a body may run on a grid that is not the batch's.
#if defined(SC_EXP_GRID) && !defined(SC_EXP_EMPTY)
#error "SC_EXP_GRID needs SC_EXP_EMPTY: a kernel with a body would run past the batch"
#endif
static inline unsigned coop_grid(unsigned nblk) {
#ifdef SC_EXP_GRID
    return SC_EXP_GRID;
#else
    return nblk;
#endif
}

// SC_CBFQP_GENERIC=1: every launch takes the generic kernels (the reference of tests/test_cbfqp_special_gpu.py; the kill switch)
static inline bool sc_cbfqp_generic() {
    static const bool v = [] { const char* e = getenv("SC_CBFQP_GENERIC"); return e && e[0] == '1'; }();
    return v;
}

// x with a signalling NaN made quiet, every other value as it is (the sign of a zero included): what v_max(x, x) does to a kernel
// argument, done once on the host so that the kernel's raw min / max may take the box bounds as they come
static inline double sc_quieted(double x) {
    if (x != x) {
        unsigned long long b;
        __builtin_memcpy(&b, &x, sizeof(b));
        b |= 0x0008000000000000ull;
        __builtin_memcpy(&x, &b, sizeof(b));
    }
    return x;
}

template <typename TIO>
static hipError_t launch_coop8_du(const sc_cbfqp_params& p, long long B, const void* X, const void* u_ref, const void* obs,
                                  void* u_out, int* status, void* h_out, hipStream_t stream) {
    const CbfConsts<double> k = make_consts<double>(p);   // once per launch, on the host
    const SinCosTab t = make_sincos_tab();
    Coop8Consts c;
    c.t0 = sc_d8{t.two_over_pi, t.pio2_1, t.pio2_2, t.pio2_3, t.s[0], t.s[1], t.s[2], t.s[3]};
    c.t1 = sc_d8{t.s[4], t.s[5], t.c[0], t.c[1], t.c[2], t.c[3], t.c[4], t.c[5]};
    c.k0 = sc_d8{k.R, k.g1, k.g2, k.inv_dt, k.inv_dt2, sc_quieted(k.lo0), sc_quieted(k.hi0), sc_quieted(k.lo1)};
    // the threshold of sincos_ and -beta of hocbf_circle; tol_feas, eps_par and +inf of the solve: the bit patterns of
    // num<double> (sc_math.hpp), which is device-only
    c.k1 = sc_d8{sc_quieted(k.hi1), 1.0e5, -1.01, 0.0, 0.0, 1e-9, 1e-12, __builtin_huge_val()};
    c.B = (unsigned)B;
    const dim3 grid(coop_grid((unsigned)((B + 7) / 8))), block(64);
#define SC_GO(FULL, HAS_H, HARD)                                                                                             \
    hipLaunchKernelGGL((cbfqp_coop8_du_kernel<TIO, FULL, HAS_H, HARD>), grid, block, 0, stream, (const TIO*)obs, (const TIO*)X, \
                       (const TIO*)u_ref, (TIO*)u_out, (TIO*)h_out, status, c)
#define SC_GO_H(FULL, HAS_H) do { if (k.hard) SC_GO(FULL, HAS_H, true); else SC_GO(FULL, HAS_H, false); } while (0)
    if (B % 8 == 0) { if (h_out) SC_GO_H(true, true); else SC_GO_H(true, false); }
    else { if (h_out) SC_GO_H(false, true); else SC_GO_H(false, false); }
#undef SC_GO_H
#undef SC_GO
    return hipGetLastError();
}

template <typename TIO, typename TC, int G, int MODEL>
static hipError_t launch_coop(const sc_cbfqp_params& p, long long B, int K, const void* X, const void* u_ref,
                              const void* obs, const int* n_obs, void* u_out, int* status, void* h_out,
                              hipStream_t stream) {
    // The specialised kernel serves the launches it was written for and nothing else: 8 rows of per-agent obstacles, no n_obs, a
    // batch in the cooperative regime, every byte offset below 2^31 (the obstacle block is the largest array of a launch), and
    // every row index B * 8 within 24 bits (the kernel forms the row's byte offset with the 24-bit multiply).
    if constexpr (G == 8 && MODEL == SC_MODEL_DYNAMIC_UNICYCLE2D && sizeof(TC) == 8 && SC_COOP_WAVES == 1) {
        if (K == 8 && n_obs == nullptr && p.obs_shared == 0 && B >= 1 && B <= sc_coop_max_agents() &&
            B * 8 * 7 * (long long)sizeof(TIO) <= 0x7fffffffLL && B * 8 <= 0xffffffLL && !sc_cbfqp_generic())
            return launch_coop8_du<TIO>(p, B, X, u_ref, obs, u_out, status, h_out, stream);
    }
    constexpr int APW = 64 / G;
    const unsigned nblk = coop_grid((unsigned)((B + APW * SC_COOP_WAVES - 1) / (APW * SC_COOP_WAVES)));
    const CbfConsts<TC> k = make_consts<TC>(p);           // once per launch, on the host: the kernel gets the finished constants
    hipLaunchKernelGGL((cbfqp_coop_kernel<TIO, TC, G, MODEL>), dim3(nblk), dim3(64 * SC_COOP_WAVES), 0, stream,
                       (const TIO*)obs, (const TIO*)X, (const TIO*)u_ref, n_obs, B, K, (int)p.obs_shared,
                       (TIO*)u_out, status, (TIO*)h_out, k);
    return hipGetLastError();
}

// ======================================================================================
// K > 8: LDS kernel.
// The kernel has three phases per 64-agent wave:
//   1. stage   obstacle rows HBM -> LDS (16-byte LDS-DMA), state / u_ref -> registers
//   2. assemble one CBF row per obstacle (rolled loop, one copy of the row builder) -> LDS
//              rows[(obstacle*3 + comp)*64 + lane]  (lane-contiguous: bank-conflict free)
//   3. solve   KMAX > 0: rows are pulled into registers and the walk is fully unrolled (K <= KMAX <= 8)
//              KMAX == 0: rows stay in LDS, run-time loops (any K up to SC_CBFQP_MAX_OBS)
//
// Phase 2 reads the staged obstacle rows with a per-lane rotation: lane l handles obstacle
// (r + l / P) mod K at step r, P = 32 / gcd(K, 32).  Lanes whose staged rows start on the same
// LDS bank (stride K*7 dwords) then read different rows, which removes the 8- (K = 8) to 16-way
// (K = 16) bank conflict of the straightforward order; the QP does not care about row order.
//
// AGENTS (sc_cbfqp_solve_batch_agents; instantiated in cbf_qp_agents.hip): the last argument is the launch-uniform parameter struct
// and the [SC_AGENT_PARAM_COLS][B] table instead of finished constants, and every lane builds its agent's constants from its
// columns (sc_agent_params.hpp), issued with the state loads.  With AGENTS = false `k` is the argument itself, as before.
template <typename TIO, typename TC, int KMAX, int MODEL, bool AGENTS = false>
__global__ __launch_bounds__(64) void cbfqp_kernel(const TIO* __restrict__ obs, const TIO* __restrict__ X,
                                                   const TIO* __restrict__ u_ref, const int* __restrict__ n_obs,
                                                   const long long B, const int K, const int obs_shared,
                                                   TIO* __restrict__ u_out, int* __restrict__ status_out,
                                                   TIO* __restrict__ h_out, const CbfQpArgs<AGENTS, TC> kargs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    TIO* lobs = reinterpret_cast<TIO*>(smem);

    const int lane = threadIdx.x;
    const long long first = (long long)blockIdx.x * 64;
    const long long agent = first + lane;
    const int nag = (int)((B - first) < 64 ? (B - first) : 64);
    const bool active = lane < nag;
    const int row_elems = K * 7;

    // ---- 1. obstacles: HBM -> LDS ------------------------------------------------
    if (obs_shared) {
        for (int e = lane; e < row_elems; e += 64) lobs[e] = obs[e];
    } else {
        const TIO* src = obs + (size_t)first * row_elems;
        const unsigned bytes = (unsigned)nag * row_elems * sizeof(TIO);
        if ((bytes & 15u) == 0 && ((reinterpret_cast<uintptr_t>(src) & 15u) == 0)) {
            wave_dma16(reinterpret_cast<const unsigned char*>(src), smem, bytes, lane);
        } else {
            const int total = nag * row_elems;
            for (int e = lane; e < total; e += 64) lobs[e] = src[e];
        }
    }

    // state / reference (coalesced, overlaps the DMA)
    using V2 = typename vec2<TIO>::type;
    const long long ag_i = active ? agent : 0;            // inactive lanes read agent 0 (B >= 1), store nothing
    const V2 ur = reinterpret_cast<const V2*>(u_ref)[ag_i];
    const StateRow<TIO, MODEL> xs = load_state<TIO, MODEL>(X, ag_i);
    int nk = K;
    if (n_obs) nk = n_obs[ag_i];                           // issued with the other loads; clamped once they are all in flight
    nk = !active ? K : (nk < 0 ? 0 : (nk > K ? K : nk));
    const TC ur0 = active ? TC(ur.x) : TC(0), ur1 = active ? TC(ur.y) : TC(0);
    const Agent<TC> ag = to_agent<TIO, TC, MODEL>(xs);
    const auto& k = solve_consts<TC>(kargs, B, ag_i);

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // LDS-DMA landed (it is tracked by vmcnt)
    __syncthreads();

    // ---- 2. row assembly: agent_barrier + cbf_qp.py:155-183 ------------------------
    const size_t stage_bytes = ((obs_shared ? (size_t)row_elems : (size_t)64 * row_elems) * sizeof(TIO) + 15) & ~(size_t)15;
    TC* rows = reinterpret_cast<TC*>(smem + stage_bytes);          // [K][3][64]
    TIO* hl = reinterpret_cast<TIO*>(rows + (size_t)K * 3 * 64);   // [K][64], natural obstacle order
    const TIO* mine = lobs + (obs_shared ? 0 : lane * row_elems);
    int period = 32;                                               // P = 32 / gcd(K, 32)
    while (((K * (32 / period)) & 31) != 0 && period > 1) period >>= 1;
    // (period ends as the smallest power of two with K*32/period = 0 mod 32, i.e. 32/gcd(K,32))
    const int rot = obs_shared ? 0 : (lane / period) % K;
    bool bad_obs = false;
    TC poison = TC(0);                                             // NaN once any row entry is non-finite
#pragma nounroll
    for (int r = 0; r < K; ++r) {
        int ro = r + rot;
        ro = ro >= K ? ro - K : ro;
        TC o[7];
#pragma unroll
        for (int f = 0; f < 7; ++f) o[f] = TC(mine[ro * 7 + f]);
        TC h, a0, a1, cc;
        const bool ok = cbf_row<TC, MODEL>(ag, o, k, a0, a1, cc, h);
        const bool used = ro < nk;
        bad_obs |= used && !ok;
        a0 = used ? a0 : TC(0); a1 = used ? a1 : TC(0); cc = used ? cc : TC(0);
        normalise_row(a0, a1, cc, poison);
        // stored at the obstacle's own index: the walk order (hence the rounding) is the same for every lane
        rows[(ro * 3 + 0) * 64 + lane] = a0;
        rows[(ro * 3 + 1) * 64 + lane] = a1;
        rows[(ro * 3 + 2) * 64 + lane] = cc;
        if constexpr (KMAX > 0) {
            hl[ro * 64 + lane] = used ? TIO(h) : TIO(0);
        } else {
            // large K: no LDS left for an h stage (f64, K = 32 uses all 160 KiB) -- store directly
            if (active && h_out) h_out[agent * K + ro] = used ? TIO(h) : TIO(0);
        }
    }

    // ---- 3. solve ---------------------------------------------------------------------
    TC u0, u1;
    int st;
    if constexpr (KMAX > 0) {
        TC n0[KMAX], n1[KMAX], c[KMAX];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            const bool in = j < K;
            n0[j] = in ? rows[(j * 3 + 0) * 64 + lane] : TC(0);
            n1[j] = in ? rows[(j * 3 + 1) * 64 + lane] : TC(0);
            c[j] = in ? rows[(j * 3 + 2) * 64 + lane] : TC(0);
        }
        st = qp2_solve<TC, KMAX>(n0, n1, c, K, ur0, ur1, poison, k, u0, u1);
    } else {
        st = qp2_solve_lds<TC>(rows, lane, K, ur0, ur1, poison, k, u0, u1);
    }

    if (bad_obs) st = SC_STATUS_BAD_OBSTACLE;
    if (st != SC_STATUS_OPTIMAL) { u0 = num<TC>::nan(); u1 = num<TC>::nan(); }

    // ---- outputs ----------------------------------------------------------------------
    if (active) {
        V2 uo; uo.x = TIO(u0); uo.y = TIO(u1);
        reinterpret_cast<V2*>(u_out)[agent] = uo;
        status_out[agent] = st;
        if constexpr (KMAX > 0) {
            if (h_out) {
                TIO* hp = h_out + agent * K;
                if (K == KMAX) {                 // static indices: vector stores
                    TIO hv[KMAX];
#pragma unroll
                    for (int r = 0; r < KMAX; ++r) hv[r] = hl[r * 64 + lane];
#pragma unroll
                    for (int r = 0; r < KMAX; ++r) hp[r] = hv[r];
                } else {
                    for (int r = 0; r < K; ++r) hp[r] = hl[r * 64 + lane];
                }
            }
        }
    }
}

// ---- host-side dispatch ----------------------------------------------------------
template <typename TIO, typename TC, int KMAX, int MODEL>
static hipError_t launch_one(const sc_cbfqp_params& p, long long B, int K, const void* X, const void* u_ref,
                             const void* obs, const int* n_obs, void* u_out, int* status, void* h_out,
                             hipStream_t stream) {
    if constexpr (KMAX > 0) {
        if (B <= sc_coop_max_agents())                    // latency-bound regime: 8 lanes per agent
            return launch_coop<TIO, TC, 8, MODEL>(p, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
        const unsigned threads = 256;
        const unsigned nblk = (unsigned)((B + threads - 1) / threads);
        const CbfConsts<TC> k = make_consts<TC>(p);
        if constexpr (MODEL == SC_MODEL_DYNAMIC_UNICYCLE2D && sizeof(TC) == 8) {
            if (sc_two_pass() && B >= (1 << 18)) {            // below, the second launch costs more than the fast pass gains (2^16: 12.2 -> 13.4 us)
                hipLaunchKernelGGL((cbfqp_reg_kernel<TIO, TC, KMAX, MODEL, 1>), dim3(nblk), dim3(threads), 0, stream,
                                   (const TIO*)obs, (const TIO*)X, (const TIO*)u_ref, n_obs, B, K, (int)p.obs_shared,
                                   (TIO*)u_out, status, (TIO*)h_out, k);
                hipError_t e = hipGetLastError();
                if (e != hipSuccess) return e;
                hipLaunchKernelGGL((cbfqp_reg_kernel<TIO, TC, KMAX, MODEL, 2>), dim3(nblk), dim3(threads), 0, stream,
                                   (const TIO*)obs, (const TIO*)X, (const TIO*)u_ref, n_obs, B, K, (int)p.obs_shared,
                                   (TIO*)u_out, status, (TIO*)h_out, k);
                return hipGetLastError();
            }
        }
        hipLaunchKernelGGL((cbfqp_reg_kernel<TIO, TC, KMAX, MODEL>), dim3(nblk), dim3(threads), 0, stream,
                           (const TIO*)obs, (const TIO*)X, (const TIO*)u_ref, n_obs, B, K, (int)p.obs_shared,
                           (TIO*)u_out, status, (TIO*)h_out, k);
        return hipGetLastError();
    } else {
    if (!sc_force_lds_kernel()) {                          // K > 8: one row per lane, 16 or 32 lanes per agent
        if (K <= 16) return launch_coop<TIO, TC, 16, MODEL>(p, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
        return launch_coop<TIO, TC, 32, MODEL>(p, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
    }
    const unsigned blocks = (unsigned)((B + 63) / 64);
    const CbfConsts<TC> k = make_consts<TC>(p);
    size_t lds = (p.obs_shared ? (size_t)K * 7 : (size_t)64 * K * 7) * sizeof(TIO);
    lds = ((lds + 15) & ~(size_t)15) + (size_t)K * 3 * 64 * sizeof(TC) + (KMAX > 0 ? (size_t)K * 64 * sizeof(TIO) : 0);
    auto kern = cbfqp_kernel<TIO, TC, KMAX, MODEL>;
    if (lds > 64 * 1024) {
        static bool raised = false;        // dynamic LDS above 64 KiB needs the attribute once
        if (!raised) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
            raised = true;
        }
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, stream,
                       (const TIO*)obs, (const TIO*)X, (const TIO*)u_ref, n_obs, B, K, (int)p.obs_shared,
                       (TIO*)u_out, status, (TIO*)h_out, k);
    return hipGetLastError();
    }
}

template <typename TIO, typename TC, int MODEL>
static hipError_t launch_k(const sc_cbfqp_params& p, long long B, int K, const void* X, const void* u_ref,
                           const void* obs, const int* n_obs, void* u_out, int* status, void* h_out,
                           hipStream_t stream) {
#define SC_K(KM) return launch_one<TIO, TC, KM, MODEL>(p, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream)
    if (K <= 4) SC_K(4);
    if (K <= 8) SC_K(8);
    SC_K(0);
#undef SC_K
}

template <typename TIO, typename TC>
static hipError_t launch_model(const sc_cbfqp_params& p, long long B, int K, const void* X, const void* u_ref,
                               const void* obs, const int* n_obs, void* u_out, int* status, void* h_out,
                               hipStream_t stream) {
    switch (p.model_id) {
        case SC_MODEL_DYNAMIC_UNICYCLE2D:
            return launch_k<TIO, TC, SC_MODEL_DYNAMIC_UNICYCLE2D>(p, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
        case SC_MODEL_KINEMATIC_BICYCLE2D:
            return launch_k<TIO, TC, SC_MODEL_KINEMATIC_BICYCLE2D>(p, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
        case SC_MODEL_KINEMATIC_BICYCLE2D_C3BF:
            return launch_k<TIO, TC, SC_MODEL_KINEMATIC_BICYCLE2D_C3BF>(p, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
        case SC_MODEL_SINGLE_INTEGRATOR2D:
            return launch_k<TIO, TC, SC_MODEL_SINGLE_INTEGRATOR2D>(p, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
        case SC_MODEL_DOUBLE_INTEGRATOR2D:
            return launch_k<TIO, TC, SC_MODEL_DOUBLE_INTEGRATOR2D>(p, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
        case SC_MODEL_QUAD2D:
            return launch_k<TIO, TC, SC_MODEL_QUAD2D>(p, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
        case SC_MODEL_UNICYCLE2D:
            return launch_k<TIO, TC, SC_MODEL_UNICYCLE2D>(p, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
        default:
            return launch_k<TIO, TC, SC_MODEL_KINEMATIC_BICYCLE2D_DPCBF>(p, B, K, X, u_ref, obs, n_obs, u_out, status, h_out, stream);
    }
}

}  // namespace sc
