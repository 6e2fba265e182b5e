// Batched Gatekeeper and MPS shields for gfx950 on the drift-car scenario: the structure of shield.hip around the
// 8-state drifting car of drift.hpp.
//
// Replaces, for B cars per launch, Gatekeeper.solve_control_problem (shielding/gatekeeper.py:553-672) and
// MPS.solve_control_problem (shielding/mps.py:59-166) in external-trajectory mode on the composition
// examples/drift_car/test_drift.py builds (:209-373): DriftingCar, LaneChangeController or StoppingController as the backup, a
// straight DriftingEnv with static and moving obstacle cars, and the friction the caller passes with every call.
// tests/_drift_shield_oracle.py is the float64 statement of the same computation (pinned on the reference's own run,
// tests/golden/drift_shield.npz).
//
// Gatekeeper: one car per 32-lane half-wave.  The nominal trajectory (the caller's, or a lane keeper rolled out by the half's
// first lane) and the car's obstacle tables are staged in LDS.  An event tests every nominal state across the lanes (state k at
// time k dt is the same in every candidate), lane j rolls out candidate j's backup trajectory of n_backup dependent tyre-model
// steps, and a ballot picks the first valid candidate.  MPS: one car per lane, one candidate (s = 1).
//
// The committed backup inputs are not stored: a cursor starts at the switching state and replays them, one step per index, under
// the friction of the commitment (kept in the state: the car's friction may have changed since, test_drift.py:437-446).
#include <hip/hip_runtime.h>

#include "../../include/safe_control_amd.h"

#pragma clang fp contract(off)

#include "drift.hpp"

namespace sc {
namespace {

using drift::Env;

struct StateView {                // the caller's state buffer (layout: include/safe_control_amd.h)
    double* cu;                   // [B, C, 2] committed nominal inputs
    double* cur;                  // [B, 8] backup cursor
    double* cmu;                  // [B] friction of the commitment
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
    v.cur = reinterpret_cast<double*>(b); b += (size_t)B * 8 * sizeof(double);
    v.cmu = reinterpret_cast<double*>(b); b += (size_t)B * sizeof(double);
    v.net = reinterpret_cast<double*>(b); b += (size_t)B * sizeof(double);
    v.s = reinterpret_cast<int*>(b);
    v.idx = v.s + B; v.clen = v.idx + B; v.init = v.clen + B;
    return v;
}

struct Agent {                    // one car's shield state during a launch
    int s, idx, clen, init;
    double net, cmu, cur[8];
};

__device__ __forceinline__ void load_agent(const StateView& S, long long a, Agent& A) {
    A.s = S.s[a]; A.idx = S.idx[a]; A.clen = S.clen[a]; A.init = S.init[a]; A.net = S.net[a]; A.cmu = S.cmu[a];
    for (int j = 0; j < 8; ++j) A.cur[j] = S.cur[a * 8 + j];
}
__device__ __forceinline__ void save_agent(const StateView& S, long long a, const Agent& A) {
    S.s[a] = A.s; S.idx[a] = A.idx; S.clen[a] = A.clen; S.init[a] = A.init; S.net[a] = A.net; S.cmu[a] = A.cmu;
    for (int j = 0; j < 8; ++j) S.cur[a * 8 + j] = A.cur[j];
}

struct Io {
    bool f32;
    __device__ double ld(const void* a, size_t i) const { return f32 ? (double)((const float*)a)[i] : ((const double*)a)[i]; }
    __device__ void operator()(void* a, size_t i, double v) const { if (f32) ((float*)a)[i] = (float)v; else ((double*)a)[i] = v; }
};

struct Args {                     // the pointers of one launch
    void* X; void* fric; const void* sob; void* mob; const void* nom_x; const void* nom_u; void* state; void* u_out;
    int* using_out; int* s_out; void* cx_out; void* cu_out; int* ret; int* ret_step; int* backup_steps;
    int n_ctrl, advance, step0;
};

// first call (gatekeeper.py:568-580, mps.py:77-89): pure backup commitment from the real state under the friction of the call
__device__ __forceinline__ void first_call(Agent& A, const double* xs, double mu, int nb) {
    A.init = 1; A.s = 0; A.idx = 0; A.net = 0.0; A.clen = nb; A.cmu = mu;
    for (int j = 0; j < 8; ++j) A.cur[j] = xs[j];
}

__device__ __forceinline__ void commit(Agent& A, int s, const double* xsw, double mu, int nb, double event_offset) {
    A.s = s; A.idx = 0; A.net = event_offset; A.clen = s + nb; A.cmu = mu;
    for (int j = 0; j < 8; ++j) A.cur[j] = xsw[j];
}

// output rule (gatekeeper.py:655-667): the committed input at the index (the cursor replays the backup part), the backup input at
// the real state past its end; then the index goes up
__device__ __forceinline__ void committed_input(Agent& A, const double* xs, const double* cu_row, const sc_drift_controller& bk, const Env& E,
                                                double& u0, double& u1) {
    if (A.idx < A.clen) {
        if (A.idx < A.s) { u0 = cu_row[2 * A.idx]; u1 = cu_row[2 * A.idx + 1]; }
        else drift::ctrl_step(A.cur, bk, A.cmu, E, u0, u1);
    } else {
        drift::control(xs, bk, u0, u1);
    }
    A.idx += 1;
}

// the backup part of candidate s from its switching state: valid iff none of the n_backup states collides (state s + k at time
// (s + k) dt); stops at the first collision
__device__ __forceinline__ bool backup_valid(const double* xsw, int s, int nb, double mu, const sc_drift_controller& bk, const double* sob, int ns,
                                             const double* mob, int nm, const Env& E) {
    double x[8];
    for (int j = 0; j < 8; ++j) x[j] = xsw[j];
    for (int k = 1; k <= nb; ++k) {
        double a0, a1;
        drift::ctrl_step(x, bk, mu, E, a0, a1);
        if (drift::state_hits(x[0], x[1], (double)(s + k) * E.dt, sob, ns, mob, nm, E)) return false;
    }
    return true;
}

// get_committed_trajectory(): states x0..x_s then the backup rollout from x_s; inputs u_0..u_{s-1} then the backup inputs
__device__ void write_committed(Io st, void* cx, void* cu, long long a, int C, int nb, int s, const double* xs0, const double* nx, const double* nu,
                                double mu, const sc_drift_controller& bk, const Env& E) {
    const size_t rx = (size_t)a * (C + 1 + nb) * 8, ru = (size_t)a * (C + nb) * 2;
    double x[8];
    for (int k = 0; k <= s; ++k) {
        const double* xk = k == 0 ? xs0 : nx + 8 * k;
        for (int j = 0; j < 8; ++j) { if (cx) st(cx, rx + 8 * k + j, xk[j]); x[j] = xk[j]; }
    }
    for (int k = 0; k < s; ++k) if (cu) { st(cu, ru + 2 * k, nu[2 * k]); st(cu, ru + 2 * k + 1, nu[2 * k + 1]); }
    for (int k = 0; k < nb; ++k) {
        double u0, u1;
        drift::ctrl_step(x, bk, mu, E, u0, u1);
        if (cx) for (int j = 0; j < 8; ++j) st(cx, rx + 8 * (s + 1 + k) + j, x[j]);
        if (cu) { st(cu, ru + 2 * (s + k), u0); st(cu, ru + 2 * (s + k) + 1, u1); }
    }
}

// lanes of my half-wave for which pred holds (bit j = lane j of the half)
__device__ __forceinline__ unsigned half_ballot(bool pred, int half) {
    return (unsigned)(__builtin_amdgcn_ballot_w64(pred) >> (32 * half));
}

// ---- Gatekeeper: one car per half-wave ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void drift_gk_kernel(const sc_drift_shield_params p, const long long B, const Args g) {
    extern __shared__ __attribute__((aligned(16))) double sm_all[];       // [2 cars][(M+1) x 8 states, M x 2 inputs, obstacle tables]
    const Io io{p.io_dtype == SC_DTYPE_F32};
    const int lane = threadIdx.x, h = lane >> 5, lh = lane & 31;
    const long long agent = (long long)blockIdx.x * 2 + h;
    const bool active = agent < B;
    const long long ag = active ? agent : 0;
    const Env E = drift::make_env(p);
    const int M = p.n_nominal, C = p.max_nominal, nb = p.n_backup, d = p.discount_steps, ns = p.n_static, nm = p.n_moving;
    const size_t per = (size_t)10 * M + 8 + 3 * SC_DRIFT_MAX_OBS + 7 * SC_DRIFT_MAX_OBS;
    double* nx = sm_all + (size_t)h * per;
    double* nu = nx + 8 * (M + 1);
    double* sob = nu + 2 * M;
    double* mob = sob + 3 * SC_DRIFT_MAX_OBS;
    const StateView S = state_view(g.state, B, C);
    double* cu_row = S.cu + (size_t)ag * C * 2;

    double xs[8];
    for (int j = 0; j < 8; ++j) xs[j] = io.ld(g.X, ag * 8 + j);
    double mu = io.ld(g.fric, ag);
    const size_t orow = p.obs_shared ? 0 : (size_t)ag;
    for (int i = lh; i < 3 * ns; i += 32) sob[i] = io.ld(g.sob, orow * 3 * ns + i);
    for (int i = lh; i < 7 * nm; i += 32) mob[i] = io.ld(g.mob, orow * 7 * nm + i);
    int rcode = g.ret ? g.ret[ag] : 0, rstep = g.ret_step ? g.ret_step[ag] : -1, nback = g.backup_steps ? g.backup_steps[ag] : 0;
    Agent A;
    load_agent(S, ag, A);
    double uo0 = 0.0, uo1 = 0.0;
    int using_b = 0;

    for (int cs = 0; cs < g.n_ctrl; ++cs) {
        const bool live = active && (!g.advance || rcode == 0);           // uniform over the half-wave
        const double pos0 = xs[0];
        if (live) {
            if (g.advance) {                                                // the puddle check (test_drift.py:437-440)
                const double cur = drift::friction_at(xs[0], xs[1], p);
                if (fabs(cur - mu) > 0.01) mu = cur;
            }
            if (g.nom_x) {
                for (int i = lh; i < 8 * (M + 1); i += 32) nx[i] = io.ld(g.nom_x, (size_t)ag * 8 * (M + 1) + i);
                for (int i = lh; i < 2 * M; i += 32) nu[i] = io.ld(g.nom_u, (size_t)ag * 2 * M + i);
            } else if (lh == 0) {                                          // the lane keeper, rolled out with car.step
                double x[8];
                for (int j = 0; j < 8; ++j) { x[j] = xs[j]; nx[j] = xs[j]; }
                for (int k = 0; k < M; ++k) {
                    double a0, a1;
                    drift::ctrl_step(x, p.keeper, mu, E, a0, a1);
                    nu[2 * k] = a0; nu[2 * k + 1] = a1;
                    for (int j = 0; j < 8; ++j) nx[8 * (k + 1) + j] = x[j];
                }
            }
        }
        __syncthreads();

        if (live) {
            bool fresh = false, committed = false;
            if (!A.init) { first_call(A, xs, mu, nb); fresh = true; }
            if ((double)A.idx >= A.net / E.dt) {                          // event (gatekeeper.py:589)
                int c = M + 1;                                             // first failing nominal state: prefix of s valid iff s < c
                for (int b0 = 0; b0 <= M; b0 += 32) {
                    const int k = b0 + lh;
                    const bool hit = k <= M && drift::state_hits(nx[8 * k], nx[8 * k + 1], (double)k * E.dt, sob, ns, mob, nm, E);
                    const unsigned m = half_ballot(hit, h);
                    if (m) { c = b0 + __builtin_ctz(m); break; }
                }
                const int n_cand = M / d + 2;                               // s_i = max(M - i d, 0); lane j of a chunk takes candidate b0 + j
                int win = -1;
                for (int b0 = 0; b0 < n_cand; b0 += 32) {
                    const int i = b0 + lh;
                    bool ok = false;
                    if (i < n_cand) {
                        const int s = max(M - i * d, 0);
                        ok = s < c && backup_valid(nx + 8 * s, s, nb, mu, p.backup, sob, ns, mob, nm, E);
                    }
                    const unsigned m = half_ballot(ok, h);
                    if (m) { win = b0 + __builtin_ctz(m); break; }
                }
                if (win >= 0) {                                            // _update_committed_trajectory (:529-551)
                    const int s = max(M - win * d, 0);
                    commit(A, s, nx + 8 * s, mu, nb, p.event_offset);
                    committed = true;
                } else {
                    A.net = (double)A.idx * E.dt + p.event_offset;
                }
            }
            if (lh == 0) {
                if (committed) for (int k = 0; k < A.s; ++k) { cu_row[2 * k] = nu[2 * k]; cu_row[2 * k + 1] = nu[2 * k + 1]; }
                if ((g.cx_out || g.cu_out) && (fresh || committed))
                    write_committed(io, g.cx_out, g.cu_out, ag, C, nb, committed ? A.s : 0, committed ? nx : xs, nx, nu, mu, p.backup, E);
            }
            // every lane of the half computes the same input: a commitment of this step is read from LDS, an older one from
            // the state buffer (written before a barrier)
            committed_input(A, xs, committed ? nu : cu_row, p.backup, E, uo0, uo1);
            using_b = A.idx >= (int)(((double)A.s * E.dt) / E.dt);         // is_using_backup (:741-744)
            if (g.advance) {                                                // the example's loop after the shield (:469-510)
                nback += using_b;
                drift::car_step(xs, uo0, uo1, mu, E);
                double mnew[2 * SC_DRIFT_MAX_OBS];
                bool hit = xs[1] > E.hw - E.R || xs[1] < -(E.hw - E.R);
                for (int j = 0; j < ns; ++j) {
                    const double dx = xs[0] - sob[3 * j], dy = xs[1] - sob[3 * j + 1];
                    hit = hit || sqrt(dx * dx + dy * dy) < sob[3 * j + 2] + E.R;
                }
                for (int j = 0; j < SC_DRIFT_MAX_OBS; ++j) {
                    if (j < nm) {                                          // step_dynamic_obstacles (drifting_env.py:652-658)
                        mnew[2 * j] = mob[7 * j] + mob[7 * j + 2] * E.dt; mnew[2 * j + 1] = mob[7 * j + 1] + mob[7 * j + 3] * E.dt;
                        const double dx = xs[0] - mnew[2 * j], dy = xs[1] - mnew[2 * j + 1];
                        hit = hit || sqrt(dx * dx + dy * dy) < mob[7 * j + 6] + E.R;
                    }
                }
                __builtin_amdgcn_wave_barrier();                            // every lane has read the old positions
                if (lh == 0) for (int j = 0; j < SC_DRIFT_MAX_OBS; ++j) if (j < nm) { mob[7 * j] = mnew[2 * j]; mob[7 * j + 1] = mnew[2 * j + 1]; }
                if (hit) { rcode = -2; rstep = g.step0 + cs; }
                else if (pos0 > E.L - 10) { rcode = 1; rstep = g.step0 + cs; }
            }
        }
        __syncthreads();                                                   // the LDS rows are free for the next step
    }

    if (active && lh == 0) {
        save_agent(S, agent, A);
        io(g.u_out, agent * 2, uo0); io(g.u_out, agent * 2 + 1, uo1);
        if (g.using_out) g.using_out[agent] = using_b;
        if (g.s_out) g.s_out[agent] = A.s;
        if (g.advance) {
            for (int j = 0; j < 8; ++j) io(g.X, agent * 8 + j, xs[j]);
            io(g.fric, agent, mu);
            for (int j = 0; j < nm; ++j) { io(g.mob, (size_t)agent * 7 * nm + 7 * j, mob[7 * j]); io(g.mob, (size_t)agent * 7 * nm + 7 * j + 1, mob[7 * j + 1]); }
            g.ret[agent] = rcode; g.ret_step[agent] = rstep;
            if (g.backup_steps) g.backup_steps[agent] = nback;
        }
    }
}

// ---- MPS: one car per lane, one candidate (s = 1) -----------------------------------------------------------------------------
__global__ __launch_bounds__(64) void drift_mps_kernel(const sc_drift_shield_params p, const long long B, const Args g) {
    const Io io{p.io_dtype == SC_DTYPE_F32};
    const long long agent = (long long)blockIdx.x * 64 + threadIdx.x;
    if (agent >= B) return;
    const Env E = drift::make_env(p);
    const int M = p.n_nominal, C = p.max_nominal, nb = p.n_backup, ns = p.n_static, nm = p.n_moving;
    const StateView S = state_view(g.state, B, C);
    double* cu_row = S.cu + (size_t)agent * C * 2;
    double sob[3 * SC_DRIFT_MAX_OBS], mob[7 * SC_DRIFT_MAX_OBS];          // the car's obstacle tables (private memory: indexed by row)
    const size_t orow = p.obs_shared ? 0 : (size_t)agent;
    for (int i = 0; i < 3 * ns; ++i) sob[i] = io.ld(g.sob, orow * 3 * ns + i);
    for (int i = 0; i < 7 * nm; ++i) mob[i] = io.ld(g.mob, orow * 7 * nm + i);

    double xs[8];
    for (int j = 0; j < 8; ++j) xs[j] = io.ld(g.X, agent * 8 + j);
    double mu = io.ld(g.fric, agent);
    int rcode = g.ret ? g.ret[agent] : 0, rstep = g.ret_step ? g.ret_step[agent] : -1, nback = g.backup_steps ? g.backup_steps[agent] : 0;
    Agent A;
    load_agent(S, agent, A);
    double uo0 = 0.0, uo1 = 0.0;
    int using_b = 0;

    for (int cs = 0; cs < g.n_ctrl; ++cs) {
        if (g.advance && rcode != 0) break;
        const double pos0 = xs[0];
        if (g.advance) {
            const double cur = drift::friction_at(xs[0], xs[1], p);
            if (fabs(cur - mu) > 0.01) mu = cur;
        }
        bool fresh = false, committed = false;
        if (!A.init) { first_call(A, xs, mu, nb); fresh = true; }
        double n0[18];                                                     // nominal x_0 (8), x_1 (8), u_0 (2)
        for (int j = 0; j < 18; ++j) n0[j] = 0.0;
        if (M >= 1) {
            if (g.nom_x) {
                for (int j = 0; j < 16; ++j) n0[j] = io.ld(g.nom_x, (size_t)agent * 8 * (M + 1) + j);
                n0[16] = io.ld(g.nom_u, (size_t)agent * 2 * M); n0[17] = io.ld(g.nom_u, (size_t)agent * 2 * M + 1);
            } else {
                for (int j = 0; j < 8; ++j) { n0[j] = xs[j]; n0[8 + j] = xs[j]; }
                drift::ctrl_step(n0 + 8, p.keeper, mu, E, n0[16], n0[17]);
            }
            const bool ok = !drift::state_hits(n0[0], n0[1], 0.0 * E.dt, sob, ns, mob, nm, E) &&
                            !drift::state_hits(n0[8], n0[9], 1.0 * E.dt, sob, ns, mob, nm, E) &&
                            backup_valid(n0 + 8, 1, nb, mu, p.backup, sob, ns, mob, nm, E);
            if (ok) {
                commit(A, 1, n0 + 8, mu, nb, p.event_offset);
                cu_row[0] = n0[16]; cu_row[1] = n0[17];
                committed = true;
            } else {
                A.net = (double)A.idx * E.dt + p.event_offset;
            }
        }
        if ((g.cx_out || g.cu_out) && (fresh || committed))
            write_committed(io, g.cx_out, g.cu_out, agent, C, nb, committed ? 1 : 0, committed ? n0 : xs, n0, n0 + 16, mu, p.backup, E);
        committed_input(A, xs, cu_row, p.backup, E, uo0, uo1);
        if (M >= 1) {                                                       // mps.py:146-158
            const double d0 = uo0 - n0[16], d1 = uo1 - n0[17];
            using_b = !(sqrt(d0 * d0 + d1 * d1) < 1e-2);
        } else {
            using_b = 1;
        }
        if (g.advance) {
            nback += using_b;
            drift::car_step(xs, uo0, uo1, mu, E);
            for (int j = 0; j < nm; ++j) { mob[7 * j] = mob[7 * j] + mob[7 * j + 2] * E.dt; mob[7 * j + 1] = mob[7 * j + 1] + mob[7 * j + 3] * E.dt; }
            if (drift::sim_hit(xs[0], xs[1], sob, ns, mob, nm, E)) { rcode = -2; rstep = g.step0 + cs; }
            else if (pos0 > E.L - 10) { rcode = 1; rstep = g.step0 + cs; }
        }
    }

    save_agent(S, agent, A);
    io(g.u_out, agent * 2, uo0); io(g.u_out, agent * 2 + 1, uo1);
    if (g.using_out) g.using_out[agent] = using_b;
    if (g.s_out) g.s_out[agent] = A.s;
    if (g.advance) {
        for (int j = 0; j < 8; ++j) io(g.X, agent * 8 + j, xs[j]);
        io(g.fric, agent, mu);
        for (int j = 0; j < nm; ++j) { io(g.mob, (size_t)agent * 7 * nm + 7 * j, mob[7 * j]); io(g.mob, (size_t)agent * 7 * nm + 7 * j + 1, mob[7 * j + 1]); }
        g.ret[agent] = rcode; g.ret_step[agent] = rstep;
        if (g.backup_steps) g.backup_steps[agent] = nback;
    }
}

}  // namespace

size_t drift_shield_state_bytes(long long B, int C) { return (size_t)B * ((size_t)C * 2 * 8 + 8 * 8 + 8 + 8 + 4 * 4); }

hipError_t drift_shield_launch(const sc_drift_shield_params& p, long long B, int n_ctrl, int advance, void* X, void* friction, const void* sob,
                               void* mob, const void* nom_x, const void* nom_u, void* state, void* u_out, int* using_out, int* s_out,
                               void* cx_out, void* cu_out, int* ret, int* ret_step, int* backup_steps, int step0, hipStream_t stream) {
    const Args g{X, friction, sob, mob, nom_x, nom_u, state, u_out, using_out, s_out, cx_out, cu_out, ret, ret_step, backup_steps, n_ctrl, advance, step0};
    if (p.algo == SC_SHIELD_MPS) {
        const unsigned blocks = (unsigned)((B + 63) / 64);
        hipLaunchKernelGGL(drift_mps_kernel, dim3(blocks), dim3(64), 0, stream, p, B, g);
        return hipGetLastError();
    }
    const size_t lds = (size_t)2 * ((size_t)10 * p.n_nominal + 8 + 10 * SC_DRIFT_MAX_OBS) * sizeof(double);
    const unsigned blocks = (unsigned)((B + 1) / 2);
    hipLaunchKernelGGL(drift_gk_kernel, dim3(blocks), dim3(64), lds, stream, p, B, g);
    return hipGetLastError();
}

}  // namespace sc
