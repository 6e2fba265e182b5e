// Fused closed loop for Quad2D under the two QP position controllers: one launch = n_steps iterations of
//   LocalTrackingController.control_step        tracking.py:559-668
//   LocalTrackingControllerDyn.control_step     dynamic_env/main.py:126-236 (moving obstacles)
// with robot_spec['model'] = 'Quad2D' and controller_type {'pos': 'cbf_qp'} or {'pos': 'optimal_decay_cbf_qp'}
// (examples/test_tracking.py --model quad --algo cbf_qp; dynamic_env/main.py:314).  Built as tracking_rollout_kernel (csrc/tracking.hip)
// and tracking_od_rollout_kernel (csrc/tracking_od.hip) are -- one agent per lane, its six states, goal, state machine and waypoint index
// in registers for the whole rollout, the shared obstacle table in LDS -- with the controller as a template parameter.  What Quad2D
// changes in the loop:
//   state machine  update_goal leaves 'rotate' at once (tracking.py:512-513); has_stopped is hypot(vx, vz) < 0.05 (quad2D.py:156-158)
//   selection      angle_unpassed = 2 pi: every row counts, ordered by centre distance, the lower index first on a tie
//   reference      Quad2D.nominal_input at its default gains under both controllers: robots/robot.py:410-413 drops the k_omega / k_a / k_v
//                  that tracking.py:602 passes; without a goal stop() = nominal_input towards the own position (quad2D.py:145-154)
//   step           Euler + the wrap of theta (quad2D.py:83-86)
// Rows and solves are those of the single-solve kernels: cbf_row<SC_MODEL_QUAD2D> + qp2_solve (sc_models.hpp, sc_qp2.hpp),
// od_build_row<SC_MODEL_QUAD2D> + od_solve<true> (od_qp.hpp).  The Quad2D nominal input and Euler step are restated below from
// csrc/tracking_quad.hip, which keeps them in an anonymous namespace behind its run-time model switch; the collision test is the shared
// one of tracking_common.hpp.
#include <hip/hip_runtime.h>

#include "od_qp.hpp"
#include "sc_dispatch.hpp"
#include "sc_qp2.hpp"
#include "tracking_common.hpp"

namespace sc {

hipError_t advance_obstacle_table_launch(bool f32, void* table, int M, int n_steps, double dt, hipStream_t stream);   // tracking.hip

namespace {

template <typename T>
struct Quad2dConsts { T mass, r_over_I, inv_R, f_min, f_max, dt, reached; };

template <typename T>
__device__ __forceinline__ T clip_(T v, T lo, T hi) { return fmin_(fmax_(v, lo), hi); }

// Quad2D.nominal_input (quad2D.py:88-143) with its default gains (3, .5 | .1, .5 | .05, .05)
template <typename T>
__device__ __forceinline__ void q2_nominal(const T x, const T z, const T th, const T vx, const T vz, const T thd, const T gx, const T gz,
                                           const Quad2dConsts<T>& q, T& u0, T& u1) {
    const T ax = T(3.0) * (gx - x) + T(0.5) * (-vx);
    const T az = T(0.1) * (gz - z) + T(0.5) * (-vz) + T(9.81);
    const T thrust = q.mass * sqrt_(ax * ax + az * az);
    const T th_d = -atan2_(ax, az);
    T e = th_d - th;
    T se, ce;
    sincos_(e, &se, &ce);
    e = atan2_(se, ce);
    const T tau = clip_(T(0.05) * e + T(0.05) * (-thd), T(-1), T(1));
    u0 = clip_((thrust + tau * q.inv_R) / T(2), q.f_min, q.f_max);
    u1 = clip_((thrust - tau * q.inv_R) / T(2), q.f_min, q.f_max);
}

}  // namespace

template <typename TIO, typename TC, int CTRL, int KMAX>
__global__ __launch_bounds__(64) void tracking_quad2d_rollout_kernel(
        const sc_tracking_quad2d_params pq, const long long B, const int M,
        TIO* __restrict__ X, const TIO* __restrict__ waypoints, const int* __restrict__ n_wp,
        int* __restrict__ wp_index, int* __restrict__ state_machine, TIO* __restrict__ goal,
        const TIO* __restrict__ obs_table, TIO* __restrict__ u_last, int* __restrict__ ret_out, int* __restrict__ ret_step,
        TIO* __restrict__ traj_X, TIO* __restrict__ traj_U, TIO* __restrict__ omega, TIO* __restrict__ min_h,
        TIO* __restrict__ traj_omega) {
    constexpr bool OD = CTRL == SC_QUAD2D_CTRL_OD_CBF_QP;
    constexpr int MODEL = SC_MODEL_QUAD2D;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    TC* table = reinterpret_cast<TC*>(smem_raw);                     // [M][7]
    const sc_tracking_od_params& po = pq.od;
    const sc_tracking_params& p = po.track;
    const int lane = threadIdx.x;
    const long long agent = (long long)blockIdx.x * 64 + lane;
    const bool active = agent < B;
    const long long ag = active ? agent : 0;

    for (int e = lane; e < M * 7; e += 64) table[e] = TC(obs_table[e]);
    __syncthreads();

    const CbfConsts<TC> k = make_consts<TC>(p.qp);
    Quad2dConsts<TC> q;
    q.mass = TC(p.qp.mass); q.r_over_I = TC(p.qp.robot_radius / pq.inertia); q.inv_R = TC(1.0 / p.qp.robot_radius);
    q.f_min = k.lo0; q.f_max = k.hi0; q.dt = TC(p.qp.dt); q.reached = TC(p.reached_threshold);
    const int enable_rotation = p.enable_rotation, dyn_obs = p.dyn_obs, K = p.num_constraints;
    const TC wr1 = TC(po.omega_ref[0]), wr2 = TC(po.omega_ref[1]);
    const TC p1 = TC(po.p_sb[0]), p2 = TC(po.p_sb[1]);

    // ---- agent state -> registers ------------------------------------------------------------
    TC x = TC(X[ag * 6 + 0]), z = TC(X[ag * 6 + 1]), th = TC(X[ag * 6 + 2]);
    TC vx = TC(X[ag * 6 + 3]), vz = TC(X[ag * 6 + 4]), thd = TC(X[ag * 6 + 5]);
    int wp = wp_index[ag], sm = state_machine[ag];
    TC gx = TC(goal[ag * 3 + 0]), gz = TC(goal[ag * 3 + 1]);
    bool gvalid = goal[ag * 3 + 2] != TIO(0);
    int ret = active ? ret_out[ag] : -2;
    int rstep = active ? ret_step[ag] : -1;                          // kept for agents frozen in an earlier launch
    const int W = p.max_waypoints;
    const TIO* wps = waypoints + (p.waypoints_shared ? 0 : (size_t)ag * W * 2);
    const int nw = n_wp[p.waypoints_shared ? 0 : ag];
    TC ul0 = TC(u_last[ag * 2 + 0]), ul1 = TC(u_last[ag * 2 + 1]);     // the last input applied so far
    TC om1 = wr1, om2 = wr2, hmin = num<TC>::inf();
    if constexpr (OD) {
        om1 = TC(omega[ag * 2 + 0]); om2 = TC(omega[ag * 2 + 1]);      // the decay of the last solve so far
        hmin = TC(min_h[ag]);
    }

    auto wp_x = [&](int i) { return TC(wps[2 * i]); };
    auto wp_z = [&](int i) { return TC(wps[2 * i + 1]); };

    // tracking.py:497-535
    auto update_goal = [&]() {
        if (sm == SC_SM_ROTATE) {
            const int i = wp < nw ? wp : (nw > 0 ? nw - 1 : 0);
            const TC rx = wp_x(i), rz = wp_z(i);
            const TC goal_angle = atan2_(rz - z, rx - x);
            sm = SC_SM_TRACK;                                          // Quad2D skips 'rotate' (:512-513)
            if (fabs_(th - goal_angle) > TC(p.rotation_threshold)) { gx = rx; gz = rz; gvalid = true; return; }
        }
        if (wp >= nw) { gvalid = false; return; }
        {
            const TC dx = x - wp_x(wp), dz = z - wp_z(wp);
            if (sqrt_(dx * dx + dz * dz) < q.reached) {
                wp += 1;
                if (wp >= nw) { sm = SC_SM_IDLE; gvalid = false; return; }
            }
        }
        gx = wp_x(wp); gz = wp_z(wp); gvalid = true;
    };

    for (int step = 0; step < p.n_steps; ++step) {
        const bool run = (ret == 0);
        if (run) {
            // ---- state machine / goal (tracking.py:569-577) ----------------------------------
            if (sm == SC_SM_STOP) {
                if (sqrt_(vx * vx + vz * vz) < TC(0.05)) {               // quad2D.py:156-158
                    sm = enable_rotation ? SC_SM_ROTATE : SC_SM_TRACK;
                    update_goal();
                }
            } else {
                update_goal();
            }
        }
        const Agent<TC> agn = make_agent_m<TC, MODEL>(x, z, th, vx, vz);
        // ---- nearest obstacles (tracking.py:345-403 with the full circle as the unpassed cone) and their rows, from the table as the
        // selection saw it
        [[maybe_unused]] TC nn[KMAX], c[KMAX];        // both thrusts enter every row alike: one coefficient per row
        [[maybe_unused]] TC poison = TC(0);
        OdRow<TC> row = od_row_none<TC>();
        bool has_obs = false;
        if constexpr (OD) {
            // the nearest only: strict < keeps the lower index on a tie, as the stable sorted insertion does
            TC bd = num<TC>::inf();
            int bi = -1;
            for (int m = 0; m < M; ++m) {
                const TC dx = table[7 * m] - x, dz = table[7 * m + 1] - z;
                const TC cd = sqrt_(dx * dx + dz * dz);
                if (cd < bd) { bd = cd; bi = m; }
            }
            has_obs = bi >= 0;
            if (has_obs) row = od_build_row<TC, MODEL>(agn, table + 7 * bi, k);
        } else {
            TC sd[KMAX];
            int si[KMAX];
#pragma unroll
            for (int j = 0; j < KMAX; ++j) { sd[j] = num<TC>::inf(); si[j] = -1; }
            for (int m = 0; m < M; ++m) {
                const TC dx = table[7 * m] - x, dz = table[7 * m + 1] - z;
                TC cd = sqrt_(dx * dx + dz * dz);
                int ci = m;
                bool moved = false;                    // stable: once the candidate is placed, everything after it shifts
#pragma unroll
                for (int j = 0; j < KMAX; ++j) {
                    const bool sw = moved || (cd < sd[j]);
                    moved = sw;
                    const TC td = sd[j]; const int ti = si[j];
                    sd[j] = sw ? cd : td; si[j] = sw ? ci : ti;
                    cd = sw ? td : cd; ci = sw ? ti : ci;
                }
            }
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {
                const bool used = (j < K) && (si[j] >= 0);
                const TC* orow = table + 7 * (si[j] >= 0 ? si[j] : 0);
                TC o[7];
#pragma unroll
                for (int f = 0; f < 7; ++f) o[f] = orow[f];
                TC h, a0, a1, cc;
                cbf_row<TC, MODEL, true>(agn, o, k, a0, a1, cc, h);       // Quad2D's barrier has no flag test: never a bad obstacle
                a0 = used ? a0 : TC(0); a1 = used ? a1 : TC(0); cc = used ? cc : TC(0);
                normalise_row(a0, a1, cc, poison);
                nn[j] = a0; c[j] = cc;                                      // a1 == a0 bit for bit, before and after the normalisation
            }
        }
        // moving obstacles advance AFTER the selection (dynamic_env/main.py:147-152): the solve sees the old table
        __syncthreads();
        if (dyn_obs) {
            for (int m = lane; m < M; m += 64) {
                table[7 * m] += table[7 * m + 3] * q.dt;
                table[7 * m + 1] += table[7 * m + 4] * q.dt;
            }
        }
        __syncthreads();
        // ---- reference input (tracking.py:589-604): 'rotate' is never held past update_goal, stop() aims at the own position ----
        TC ur0, ur1;
        q2_nominal<TC>(x, z, th, vx, vz, thd, gvalid ? gx : x, gvalid ? gz : z, q, ur0, ur1);
        // ---- solve, in every state-machine state -------------------------------------------------
        TC u0, u1, w1 = wr1, w2 = wr2;
        int st;
        if constexpr (OD) {
            st = od_solve<TC, true>(row, ur0, ur1, wr1, wr2, p1, p2, k, u0, u1, w1, w2);      // optimal_decay_cbf_qp.py:131-158
        } else {
            if (M == 0) { u0 = ur0; u1 = ur1; st = SC_STATUS_OPTIMAL; }    // obs_list None: u_ref unsolved (cbf_qp.py:113-118)
            else st = qp2_solve<TC, KMAX>(nn, nn, c, K, ur0, ur1, poison, k, u0, u1);          // cbf_qp.py:108-199
        }
        // ---- collision / status / step (tracking.py:627-646) ---------------------------------------
        // pre-step: infeasible or already colliding -> -2, the robot does not move
        const bool pre_fail = (st != SC_STATUS_OPTIMAL) || collides<TC>(x, z, table, M, k.R);
        // quad2D.py:46-86: X + (f + g u) dt, theta wrapped
        const TC thrust = u0 + u1;
        const TC nx = x + vx * q.dt, nz = z + vz * q.dt;
        const TC nth = angle_normalize(th + thd * q.dt);
        const TC nvx = vx + (-agn.s * k.inv_mass * thrust) * q.dt;
        const TC nvz = vz + (TC(-9.81) + agn.c * k.inv_mass * thrust) * q.dt;
        const TC nthd = thd + (q.r_over_I * (u0 - u1)) * q.dt;
        int code;
        if (pre_fail) code = -2;
        else if (collides<TC>(nx, nz, table, M, k.R)) code = -2;             // post-step: the robot HAS moved
        else code = (!gvalid && sm != SC_SM_STOP) ? -1 : 0;                  // tracking.py:666-667
        if (run) {
            if constexpr (OD) {
                if (st == SC_STATUS_OPTIMAL) { om1 = w1; om2 = w2; }
                if (has_obs) hmin = fmin_(hmin, row.h);
            }
            if (!pre_fail) { x = nx; z = nz; th = nth; vx = nvx; vz = nvz; thd = nthd; ul0 = u0; ul1 = u1; }
            if (code != 0) { ret = code; rstep = p.step_offset + step; }
        }
        if (active && traj_X) {
            TIO* tx = traj_X + ((size_t)step * B + agent) * 6;
            tx[0] = TIO(x); tx[1] = TIO(z); tx[2] = TIO(th); tx[3] = TIO(vx); tx[4] = TIO(vz); tx[5] = TIO(thd);
        }
        if (active && traj_U) {
            TIO* tu = traj_U + ((size_t)step * B + agent) * 2;
            tu[0] = TIO(ul0); tu[1] = TIO(ul1);
        }
        if constexpr (OD) {
            if (active && traj_omega) {
                TIO* tw = traj_omega + ((size_t)step * B + agent) * 2;
                tw[0] = TIO(om1); tw[1] = TIO(om2);
            }
        }
    }

    if (active) {
        TIO* xo = X + agent * 6;
        xo[0] = TIO(x); xo[1] = TIO(z); xo[2] = TIO(th); xo[3] = TIO(vx); xo[4] = TIO(vz); xo[5] = TIO(thd);
        wp_index[agent] = wp; state_machine[agent] = sm;
        goal[agent * 3 + 0] = TIO(gx); goal[agent * 3 + 1] = TIO(gz); goal[agent * 3 + 2] = gvalid ? TIO(1) : TIO(0);
        u_last[agent * 2 + 0] = TIO(ul0); u_last[agent * 2 + 1] = TIO(ul1);
        if constexpr (OD) {
            omega[agent * 2 + 0] = TIO(om1); omega[agent * 2 + 1] = TIO(om2);
            min_h[agent] = TIO(hmin);
        }
        ret_out[agent] = ret; ret_step[agent] = rstep;
    }
}

hipError_t tracking_quad2d_launch(const sc_tracking_quad2d_params& p, long long B, int M, void* X, const void* wps, const int* n_wp,
                                  int* wp_index, int* sm, void* goal, void* table, void* u_last, int* ret, int* ret_step,
                                  void* tX, void* tU, void* omega, void* min_h, void* tW, hipStream_t stream) {
    const unsigned blocks = (unsigned)((B + 63) / 64);
    const size_t lds = (size_t)(M > 0 ? M : 1) * 7 * sizeof(double);
    hipError_t e = dispatch_io(p.od.track.qp.io_dtype, [&](auto tio) {
        auto go = [&](auto ctrl, auto kmax) {                            // closed loops amplify rounding: arithmetic is always f64
            return launch(tracking_quad2d_rollout_kernel<tag_t<decltype(tio)>, double, decltype(ctrl)::value, decltype(kmax)::value>, blocks, 64,
                          lds, stream, p, B, M, X, wps, n_wp, wp_index, sm, goal, table, u_last, ret, ret_step, tX, tU, omega, min_h, tW);
        };
        if (p.controller == SC_QUAD2D_CTRL_OD_CBF_QP) return go(int_tag<SC_QUAD2D_CTRL_OD_CBF_QP>{}, int_tag<1>{});
        if (p.od.track.num_constraints <= 4) return go(int_tag<SC_QUAD2D_CTRL_CBF_QP>{}, int_tag<4>{});
        if (p.od.track.num_constraints <= 8) return go(int_tag<SC_QUAD2D_CTRL_CBF_QP>{}, int_tag<8>{});
        return go(int_tag<SC_QUAD2D_CTRL_CBF_QP>{}, int_tag<16>{});
    });
    if (e != hipSuccess || !p.od.track.dyn_obs || M == 0) return e;
    // every block advanced its own LDS copy: the stream-ordered follow-up writes the table where n_steps put it
    return advance_obstacle_table_launch(p.od.track.qp.io_dtype == SC_DTYPE_F32, table, M, p.od.track.n_steps, p.od.track.qp.dt, stream);
}

}  // namespace sc
