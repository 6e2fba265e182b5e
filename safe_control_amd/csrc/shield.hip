// Batched Gatekeeper and MPS shields for gfx950 on the evade scenario: event test, candidate search over switching times,
// commit / reschedule and the committed input, per agent, with the shield's state kept on the device between calls.
//
// Replaces, for B agents per launch, the per-robot path
//   Gatekeeper.solve_control_problem   shielding/gatekeeper.py:553-672 (candidates :309-367, validity :380-471,499-527,
//                                      commit :529-551, is_using_backup :741-744)
//   MPS.solve_control_problem          shielding/mps.py:59-166
// in external-trajectory mode on the composition examples/evade/test_evade.py builds (:335-408): DoubleIntegrator2D,
// EvadeBackupController, EvadeEnv (walls, pocket, the bullet now) and the bullet predicted at constant speed.
// tests/_shield_oracle.py is the float64 statement of the same computation (pinned on the reference's own run,
// tests/golden/shield.npz).
//
// Gatekeeper mapping: one agent per 32-lane half-wave (two per workgroup).  The nominal trajectory (the caller's, or the
// example's nominal controller rolled out on the device by the half's first lane) is staged in LDS.  An event first tests
// every nominal state across the lanes; the first failing index c gives "prefix valid" = s < c for every candidate, since
// candidate state k <= s IS nominal state k at the same time k dt.  Lane j then rolls out candidate j's backup trajectory
// (only if its prefix is valid; it stops at its first collision), and a ballot picks the smallest valid j -- the candidate
// the reference's sequential search commits.  More than 32 candidates are taken in chunks of 32, in order.
// MPS mapping: one agent per lane (a single candidate, s = 1).
//
// The committed backup inputs are not stored: the backup cursor starts at the switching state and steps once per index
// in [s, s + n_backup), the same operations as the reference's stored rollout, so the input is the same to the bit.
#include <hip/hip_runtime.h>

#include "../../include/safe_control_amd.h"

#pragma clang fp contract(off)

#include "evade.hpp"

namespace sc {
namespace {

using evade::Env;

struct StateView {                // the caller's state buffer (layout: include/safe_control_amd.h)
    double* cu;                   // [B, C, 2] committed nominal inputs
    double* cur;                  // [B, 4] backup cursor
    double* net;                  // [B] next_event_time
    int* s;                       // [B] committed nominal steps
    int* idx;                     // [B] current_time_idx
    int* clen;                    // [B] len(committed_u_traj)
    int* init;                    // [B] 0: fresh shield
};

__device__ __forceinline__ StateView state_view(void* base, long long B, int C) {
    char* b = static_cast<char*>(base);
    StateView v;
    v.cu = reinterpret_cast<double*>(b); b += (size_t)B * C * 2 * sizeof(double);
    v.cur = reinterpret_cast<double*>(b); b += (size_t)B * 4 * sizeof(double);
    v.net = reinterpret_cast<double*>(b); b += (size_t)B * sizeof(double);
    v.s = reinterpret_cast<int*>(b);
    v.idx = v.s + B; v.clen = v.idx + B; v.init = v.clen + B;
    return v;
}

struct Agent {                    // one agent's shield state, in registers during a launch
    int s, idx, clen, init;
    double net, cur[4];
};

__device__ __forceinline__ void load_agent(const StateView& S, long long a, Agent& A) {
    A.s = S.s[a]; A.idx = S.idx[a]; A.clen = S.clen[a]; A.init = S.init[a]; A.net = S.net[a];
#pragma unroll
    for (int j = 0; j < 4; ++j) A.cur[j] = S.cur[a * 4 + j];
}
__device__ __forceinline__ void save_agent(const StateView& S, long long a, const Agent& A) {
    S.s[a] = A.s; S.idx[a] = A.idx; S.clen[a] = A.clen; S.init[a] = A.init; S.net[a] = A.net;
#pragma unroll
    for (int j = 0; j < 4; ++j) S.cur[a * 4 + j] = A.cur[j];
}

// first call (gatekeeper.py:568-580, mps.py:77-89): pure backup commitment from the real state, event at once
__device__ __forceinline__ void first_call(Agent& A, const double* xs, int nb) {
    A.init = 1; A.s = 0; A.idx = 0; A.net = 0.0; A.clen = nb;
#pragma unroll
    for (int j = 0; j < 4; ++j) A.cur[j] = xs[j];
}

// output rule (gatekeeper.py:655-667): the committed input at the index, the backup input at the real state past its end;
// then the index goes up
__device__ __forceinline__ void committed_input(Agent& A, const double* xs, const double* cu_row, const Env& E, double& u0, double& u1) {
    if (A.idx < A.clen) {
        if (A.idx < A.s) { u0 = cu_row[2 * A.idx]; u1 = cu_row[2 * A.idx + 1]; }
        else evade::backup_step(A.cur, E, u0, u1);
    } else {
        evade::backup(xs, E, u0, u1);
    }
    A.idx += 1;
}

// the committed trajectory for get_committed_trajectory(): states x0..x_s (nominal, or the real state on the first call),
// then the backup rollout from x_s; inputs u_0..u_{s-1}, then the backup inputs
template <class ST>
__device__ void write_committed(ST st, void* cx, void* cu, long long a, int C, int nb, int s, const double* xs0, const double* nx,
                                const double* nu, const Env& E) {
    const size_t rx = (size_t)a * (C + 1 + nb) * 4, ru = (size_t)a * (C + nb) * 2;
    double x[4];
    for (int k = 0; k <= s; ++k) {
        const double* xk = k == 0 ? xs0 : nx + 4 * k;
#pragma unroll
        for (int j = 0; j < 4; ++j) { if (cx) st(cx, rx + 4 * k + j, xk[j]); x[j] = xk[j]; }
    }
    for (int k = 0; k < s; ++k) if (cu) { st(cu, ru + 2 * k, nu[2 * k]); st(cu, ru + 2 * k + 1, nu[2 * k + 1]); }
    for (int k = 0; k < nb; ++k) {
        double u0, u1;
        evade::backup_step(x, E, u0, u1);
        if (cx) {
#pragma unroll
            for (int j = 0; j < 4; ++j) st(cx, rx + 4 * (s + 1 + k) + j, x[j]);
        }
        if (cu) { st(cu, ru + 2 * (s + k), u0); st(cu, ru + 2 * (s + k) + 1, u1); }
    }
}

// the example's loop after the shield (test_evade.py:456-497): step, speed clamp, step_bullet, collision with the PRE-step
// position against the stepped bullet, goal
__device__ __forceinline__ void close_loop(double* xs, double& bx, double u0, double u1, const Env& E, int& rcode, int& rstep, int step) {
    const double pos0 = xs[0], pos1 = xs[1];
    double xn[4];
    evade::step(xs, u0, u1, E, xn);
    const double vm = sqrt(xn[2] * xn[2] + xn[3] * xn[3]);
    if (vm > E.vmax) { xn[2] = xn[2] * E.vmax / vm; xn[3] = xn[3] * E.vmax / vm; }
#pragma unroll
    for (int j = 0; j < 4; ++j) xs[j] = xn[j];
    bx += E.bspeed * E.dt;                                                 // EvadeEnv.step_bullet (evade_env.py:360-384)
    if (bx > E.L + E.blen) bx = E.bstart;
    if (evade::bullet_hit_now(pos0, pos1, bx, E)) { rcode = -2; rstep = step; }
    else if (E.gxmin <= pos0 && pos0 <= E.gxmax && -E.hw <= pos1 && pos1 <= E.hw) { rcode = 1; rstep = step; }
}

// lanes of my half-wave for which pred holds (bit j = lane j of the half)
__device__ __forceinline__ unsigned half_ballot(bool pred, int half) {
    return (unsigned)(__builtin_amdgcn_ballot_w64(pred) >> (32 * half));
}

struct Io {
    bool f32;
    __device__ double ld(const void* a, size_t i) const { return f32 ? (double)((const float*)a)[i] : ((const double*)a)[i]; }
    __device__ void operator()(void* a, size_t i, double v) const { if (f32) ((float*)a)[i] = (float)v; else ((double*)a)[i] = v; }
};

// ---- Gatekeeper: one agent per half-wave ----------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void shield_gk_kernel(const sc_shield_params p, const long long B, const int n_ctrl, const int advance,
                                                       void* __restrict__ X, void* __restrict__ bullet_x, const void* __restrict__ nom_x,
                                                       const void* __restrict__ nom_u, void* __restrict__ state, void* __restrict__ u_out,
                                                       int* __restrict__ using_out, int* __restrict__ s_out, void* __restrict__ cx_out,
                                                       void* __restrict__ cu_out, int* __restrict__ ret, int* __restrict__ ret_step,
                                                       int* __restrict__ backup_steps, const int step0) {
    extern __shared__ __attribute__((aligned(16))) double sm_nom[];       // [2 agents][(M+1) x 4 states, M x 2 inputs]
    const Io io{p.base.io_dtype == SC_DTYPE_F32};
    const int lane = threadIdx.x, h = lane >> 5, lh = lane & 31;
    const long long agent = (long long)blockIdx.x * 2 + h;
    const bool active = agent < B;
    const long long ag = active ? agent : 0;
    const Env E = evade::make_env(p.base);
    const int M = p.n_nominal, C = p.max_nominal, nb = p.n_backup, d = p.discount_steps;
    const bool predict = p.predict_bullet != 0;
    double* nx = sm_nom + (size_t)h * (6 * M + 4);
    double* nu = nx + 4 * (M + 1);
    const StateView S = state_view(state, B, C);
    double* cu_row = S.cu + (size_t)ag * C * 2;

    double xs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xs[j] = io.ld(X, ag * 4 + j);
    double bx = io.ld(bullet_x, p.base.bullet_shared ? 0 : ag);
    int rcode = ret ? ret[ag] : 0, rstep = ret_step ? ret_step[ag] : -1, nback = backup_steps ? backup_steps[ag] : 0;
    Agent A;
    load_agent(S, ag, A);
    double uo0 = 0.0, uo1 = 0.0;
    int using_b = 0;

    for (int cs = 0; cs < n_ctrl; ++cs) {
        const bool live = active && (!advance || rcode == 0);           // uniform over the half-wave
        // ---- the nominal trajectory in LDS ----------------------------------------------------------------------------------
        if (live) {
            if (nom_x) {
                for (int i = lh; i < 4 * (M + 1); i += 32) nx[i] = io.ld(nom_x, (size_t)ag * 4 * (M + 1) + i);
                for (int i = lh; i < 2 * M; i += 32) nu[i] = io.ld(nom_u, (size_t)ag * 2 * M + i);
            } else if (lh == 0) {                                          // rollout_nominal (test_evade.py:387-408)
                double x[4] = {xs[0], xs[1], xs[2], xs[3]};
#pragma unroll
                for (int j = 0; j < 4; ++j) nx[j] = x[j];
                for (int k = 0; k < M; ++k) {
                    double a0, a1, xn[4];
                    evade::nominal(x, E, a0, a1);
                    evade::step(x, a0, a1, E, xn);
                    nu[2 * k] = a0; nu[2 * k + 1] = a1;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { x[j] = xn[j]; nx[4 * (k + 1) + j] = xn[j]; }
                }
            }
        }
        __syncthreads();

        if (live) {
            bool fresh = false, committed = false;
            if (!A.init) { first_call(A, xs, nb); fresh = true; }
            if ((double)A.idx >= A.net / E.dt) {                          // event (gatekeeper.py:589)
                // first failing nominal state: prefix of candidate s is valid iff s < c
                int c = M + 1;
                for (int b0 = 0; b0 <= M; b0 += 32) {
                    const int k = b0 + lh;
                    const bool hit = k <= M && evade::state_hits(nx[4 * k], nx[4 * k + 1], (double)k * E.dt, bx, predict, E);
                    const unsigned m = half_ballot(hit, h);
                    if (m) { c = b0 + __builtin_ctz(m); break; }
                }
                // candidates i = 0 .. M / d + 1, s_i = max(M - i d, 0); lane j of a chunk takes candidate b0 + j
                const int n_cand = M / d + 2;
                int win = -1;
                for (int b0 = 0; b0 < n_cand; b0 += 32) {
                    const int i = b0 + lh;
                    bool ok = false;
                    if (i < n_cand) {
                        const int s = max(M - i * d, 0);
                        ok = s < c;
                        if (ok) {
                            double x[4] = {nx[4 * s], nx[4 * s + 1], nx[4 * s + 2], nx[4 * s + 3]};
                            for (int k = 1; k <= nb; ++k) {
                                double a0, a1;
                                evade::backup_step(x, E, a0, a1);
                                if (evade::state_hits(x[0], x[1], (double)(s + k) * E.dt, bx, predict, E)) { ok = false; break; }
                            }
                        }
                    }
                    const unsigned m = half_ballot(ok, h);
                    if (m) { win = b0 + __builtin_ctz(m); break; }
                }
                if (win >= 0) {                                            // _update_committed_trajectory (:529-551)
                    const int s = max(M - win * d, 0);
                    A.s = s; A.idx = 0; A.net = p.event_offset; A.clen = s + nb;
#pragma unroll
                    for (int j = 0; j < 4; ++j) A.cur[j] = nx[4 * s + j];
                    committed = true;
                } else {
                    A.net = (double)A.idx * E.dt + p.event_offset;
                }
            }
            if (lh == 0) {
                if (committed) for (int k = 0; k < A.s; ++k) { cu_row[2 * k] = nu[2 * k]; cu_row[2 * k + 1] = nu[2 * k + 1]; }
                if ((cx_out || cu_out) && (fresh || committed)) {
                    if (committed) write_committed(io, cx_out, cu_out, ag, C, nb, A.s, nx, nx, nu, E);
                    else write_committed(io, cx_out, cu_out, ag, C, nb, 0, xs, nx, nu, E);
                }
            }
            // every lane of the half computes the same input: a commitment of this step is read from LDS (lane 0's global
            // copy is not visible to the other lanes yet), an older one from the state buffer (written before a barrier)
            committed_input(A, xs, committed ? nu : cu_row, E, uo0, uo1);
            using_b = A.idx >= (int)(((double)A.s * E.dt) / E.dt);         // is_using_backup (:741-744)
            if (advance) {
                nback += using_b;
                close_loop(xs, bx, uo0, uo1, E, rcode, rstep, step0 + cs);
            }
        }
        __syncthreads();                                                   // the LDS rows are free for the next step
    }

    if (active && lh == 0) {
        save_agent(S, agent, A);
        io(u_out, agent * 2, uo0); io(u_out, agent * 2 + 1, uo1);
        if (using_out) using_out[agent] = using_b;
        if (s_out) s_out[agent] = A.s;
        if (advance) {
#pragma unroll
            for (int j = 0; j < 4; ++j) io(X, agent * 4 + j, xs[j]);
            io(bullet_x, agent, bx);
            ret[agent] = rcode; ret_step[agent] = rstep;
            if (backup_steps) backup_steps[agent] = nback;
        }
    }
}

// ---- MPS: one agent per lane, one candidate (s = 1) ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void shield_mps_kernel(const sc_shield_params p, const long long B, const int n_ctrl, const int advance,
                                                        void* __restrict__ X, void* __restrict__ bullet_x, const void* __restrict__ nom_x,
                                                        const void* __restrict__ nom_u, void* __restrict__ state, void* __restrict__ u_out,
                                                        int* __restrict__ using_out, int* __restrict__ s_out, void* __restrict__ cx_out,
                                                        void* __restrict__ cu_out, int* __restrict__ ret, int* __restrict__ ret_step,
                                                        int* __restrict__ backup_steps, const int step0) {
    const Io io{p.base.io_dtype == SC_DTYPE_F32};
    const long long agent = (long long)blockIdx.x * 64 + threadIdx.x;
    if (agent >= B) return;
    const Env E = evade::make_env(p.base);
    const int M = p.n_nominal, C = p.max_nominal, nb = p.n_backup;
    const bool predict = p.predict_bullet != 0;
    const StateView S = state_view(state, B, C);
    double* cu_row = S.cu + (size_t)agent * C * 2;

    double xs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xs[j] = io.ld(X, agent * 4 + j);
    double bx = io.ld(bullet_x, p.base.bullet_shared ? 0 : agent);
    int rcode = ret ? ret[agent] : 0, rstep = ret_step ? ret_step[agent] : -1, nback = backup_steps ? backup_steps[agent] : 0;
    Agent A;
    load_agent(S, agent, A);
    double uo0 = 0.0, uo1 = 0.0;
    int using_b = 0;

    for (int cs = 0; cs < n_ctrl; ++cs) {
        if (advance && rcode != 0) break;
        bool fresh = false, committed = false;
        if (!A.init) { first_call(A, xs, nb); fresh = true; }
        // nominal_x_traj[0:2], nominal_u_traj[0]
        double n0[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};                     // x_0 (4), x_1 (4), u_0 (2)
        if (M >= 1) {
            if (nom_x) {
                for (int j = 0; j < 8; ++j) n0[j] = io.ld(nom_x, (size_t)agent * 4 * (M + 1) + j);
                n0[8] = io.ld(nom_u, (size_t)agent * 2 * M); n0[9] = io.ld(nom_u, (size_t)agent * 2 * M + 1);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) n0[j] = xs[j];
                evade::nominal(xs, E, n0[8], n0[9]);
                evade::step(xs, n0[8], n0[9], E, n0 + 4);
            }
            bool ok = !evade::state_hits(n0[0], n0[1], 0.0 * E.dt, bx, predict, E) &&
                      !evade::state_hits(n0[4], n0[5], 1.0 * E.dt, bx, predict, E);
            if (ok) {
                double x[4] = {n0[4], n0[5], n0[6], n0[7]};
                for (int k = 1; k <= nb; ++k) {
                    double a0, a1;
                    evade::backup_step(x, E, a0, a1);
                    if (evade::state_hits(x[0], x[1], (double)(1 + k) * E.dt, bx, predict, E)) { ok = false; break; }
                }
            }
            if (ok) {
                A.s = 1; A.idx = 0; A.net = p.event_offset; A.clen = 1 + nb;
#pragma unroll
                for (int j = 0; j < 4; ++j) A.cur[j] = n0[4 + j];
                cu_row[0] = n0[8]; cu_row[1] = n0[9];
                committed = true;
            } else {
                A.net = (double)A.idx * E.dt + p.event_offset;
            }
        }
        if ((cx_out || cu_out) && (fresh || committed)) {
            double nx1[8] = {0, 0, 0, 0, n0[4], n0[5], n0[6], n0[7]};
            if (committed) write_committed(io, cx_out, cu_out, agent, C, nb, 1, n0, nx1, n0 + 8, E);
            else write_committed(io, cx_out, cu_out, agent, C, nb, 0, xs, nx1, n0 + 8, E);
        }
        committed_input(A, xs, cu_row, E, uo0, uo1);
        if (M >= 1) {                                                       // mps.py:145-157
            const double d0 = uo0 - n0[8], d1 = uo1 - n0[9];
            using_b = !(sqrt(d0 * d0 + d1 * d1) < 1e-2);
        } else {
            using_b = 1;
        }
        if (advance) {
            nback += using_b;
            close_loop(xs, bx, uo0, uo1, E, rcode, rstep, step0 + cs);
        }
    }

    save_agent(S, agent, A);
    io(u_out, agent * 2, uo0); io(u_out, agent * 2 + 1, uo1);
    if (using_out) using_out[agent] = using_b;
    if (s_out) s_out[agent] = A.s;
    if (advance) {
#pragma unroll
        for (int j = 0; j < 4; ++j) io(X, agent * 4 + j, xs[j]);
        io(bullet_x, agent, bx);
        ret[agent] = rcode; ret_step[agent] = rstep;
        if (backup_steps) backup_steps[agent] = nback;
    }
}

}  // namespace

size_t shield_state_bytes(long long B, int C) { return (size_t)B * ((size_t)C * 2 * 8 + 4 * 8 + 8 + 4 * 4); }

hipError_t shield_launch(const sc_shield_params& p, long long B, int n_ctrl, int advance, void* X, void* bullet_x, const void* nom_x,
                         const void* nom_u, void* state, void* u_out, int* using_out, int* s_out, void* cx_out, void* cu_out, int* ret,
                         int* ret_step, int* backup_steps, int step0, hipStream_t stream) {
    if (p.algo == SC_SHIELD_MPS) {
        const unsigned blocks = (unsigned)((B + 63) / 64);
        hipLaunchKernelGGL(shield_mps_kernel, dim3(blocks), dim3(64), 0, stream, p, B, n_ctrl, advance, X, bullet_x, nom_x, nom_u, state,
                           u_out, using_out, s_out, cx_out, cu_out, ret, ret_step, backup_steps, step0);
    } else {
        const size_t lds = (size_t)2 * (6 * p.n_nominal + 4) * sizeof(double);
        const unsigned blocks = (unsigned)((B + 1) / 2);
        hipLaunchKernelGGL(shield_gk_kernel, dim3(blocks), dim3(64), lds, stream, p, B, n_ctrl, advance, X, bullet_x, nom_x, nom_u, state,
                           u_out, using_out, s_out, cx_out, cu_out, ret, ret_step, backup_steps, step0);
    }
    return hipGetLastError();
}

}  // namespace sc
