// Fused closed loop with the optimal-decay CBF-QP as its position controller: one launch = n_steps iterations of
//   LocalTrackingController.control_step        tracking.py:559-668
//   LocalTrackingControllerDyn.control_step     dynamic_env/main.py:126-236 (moving obstacles)
// under controller_type {'pos': 'optimal_decay_cbf_qp'} (tracking.py:148-150, main.py:167-179).  Built as tracking_rollout_kernel
// (csrc/tracking.hip) is -- one agent per lane, its state in registers for the whole rollout, the shared obstacle table in LDS -- and
// different from it where the reference treats this controller differently:
//   gains        'track' calls nominal_input(goal, k_omega=3.0, k_a=0.5, k_v=0.5) (tracking.py:601-602); stop() keeps its own gain
//                (robots/dynamic_unicycle2D.py:106-108) and rotate_to its 2.0
//   one obstacle the controller sees the nearest unpassed obstacle only (row 0 of get_nearest_unpassed_obs): a running minimum
//                replaces the K-row sorted insertion
//   no obstacle  the QP is solved with A = b = h = h_dot = 0 (optimal_decay_cbf_qp.py:133-137), so the input box still applies
//   every state  the QP is solved in 'track', 'stop' and 'rotate' alike
// The row build and the 1 + 9 active-set solve are those of the single-solve kernel (od_qp.hpp).
#include <hip/hip_runtime.h>

#include "od_qp.hpp"
#include "sc_dispatch.hpp"
#include "tracking_common.hpp"

namespace sc {

hipError_t advance_obstacle_table_launch(bool f32, void* table, int M, int n_steps, double dt, hipStream_t stream);   // tracking.hip

template <typename TIO, typename TC, int MODEL>
__global__ __launch_bounds__(64) void tracking_od_rollout_kernel(
        const sc_tracking_od_params po, const long long B, const int M,
        TIO* __restrict__ X, const TIO* __restrict__ waypoints, const int* __restrict__ n_wp,
        int* __restrict__ wp_index, int* __restrict__ state_machine, TIO* __restrict__ goal,
        const TIO* __restrict__ obs_table, TIO* __restrict__ u_last, int* __restrict__ ret_out, int* __restrict__ ret_step,
        TIO* __restrict__ traj_X, TIO* __restrict__ traj_U, TIO* __restrict__ omega, TIO* __restrict__ min_h,
        TIO* __restrict__ traj_omega) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    TC* table = reinterpret_cast<TC*>(smem_raw);                     // [M][7]
    const sc_tracking_params& p = po.track;
    const int lane = threadIdx.x;
    const long long agent = (long long)blockIdx.x * 64 + lane;
    const bool active = agent < B;
    const long long ag = active ? agent : 0;

    for (int e = lane; e < M * 7; e += 64) table[e] = TC(obs_table[e]);
    __syncthreads();

    const CbfConsts<TC> k = make_consts<TC>(p.qp);
    TrackConsts<TC> t;
    t.reached = TC(p.reached_threshold); t.rot_thr = TC(p.rotation_threshold);
    t.v_max = TC(p.v_max); t.v_min = TC(p.v_min);
    t.k_omega = TC(p.k_omega); t.k_a = TC(p.k_a); t.k_v = TC(p.k_v);                 // the 'track' gains
    t.delta_max = TC(p.delta_max); t.wheel_base = TC(p.wheel_base); t.Lr = TC(p.qp.rear_ax_dist); t.dt = TC(p.qp.dt); t.a_max = TC(p.qp.u_max[0]);
    t.enable_rotation = p.enable_rotation; t.dyn_obs = p.dyn_obs; t.K = 1;
    const TC k_a_stop = TC(po.k_a_stop);
    const TC wr1 = TC(po.omega_ref[0]), wr2 = TC(po.omega_ref[1]);
    const TC p1 = TC(po.p_sb[0]), p2 = TC(po.p_sb[1]);
    constexpr bool REL2 = od_rel2<MODEL>::value;
    const TC pi = TC(3.14159265358979323846);
    const TC half_unpassed = TC(1.2) * pi / TC(2);                   // DynamicUnicycle2D (tracking.py:352-357)

    // ---- agent state -> registers ------------------------------------------------------------
    TC x = TC(X[ag * 4 + 0]), y = TC(X[ag * 4 + 1]), th = TC(X[ag * 4 + 2]), v = TC(X[ag * 4 + 3]);
    int wp = wp_index[ag], sm = state_machine[ag];
    TC gx = TC(goal[ag * 3 + 0]), gy = TC(goal[ag * 3 + 1]);
    bool gvalid = goal[ag * 3 + 2] != TIO(0);
    int ret = active ? ret_out[ag] : -2;
    int rstep = active ? ret_step[ag] : -1;                          // kept for agents frozen in an earlier launch
    const int W = p.max_waypoints;
    const TIO* wps = waypoints + (p.waypoints_shared ? 0 : (size_t)ag * W * 2);
    const int nw = n_wp[p.waypoints_shared ? 0 : ag];
    TC ul0 = TC(u_last[ag * 2 + 0]), ul1 = TC(u_last[ag * 2 + 1]);     // the last input applied so far
    TC om1 = TC(omega[ag * 2 + 0]), om2 = TC(omega[ag * 2 + 1]);       // the decay of the last solve so far
    TC hmin = TC(min_h[ag]);

    auto wp_x = [&](int i) { return TC(wps[2 * i]); };
    auto wp_y = [&](int i) { return TC(wps[2 * i + 1]); };

    // tracking.py:497-535
    auto update_goal = [&]() {
        if (sm == SC_SM_ROTATE) {
            const int i = wp < nw ? wp : nw - 1;
            const TC rx = wp_x(i), ry = wp_y(i);
            const TC goal_angle = atan2_(ry - y, rx - x);
            if (!t.enable_rotation) sm = SC_SM_TRACK;
            if (fabs_(th - goal_angle) > t.rot_thr) { gx = rx; gy = ry; gvalid = true; return; }
            sm = SC_SM_TRACK;
        }
        if (wp >= nw) { gvalid = false; return; }
        {
            const TC dx = x - wp_x(wp), dy = y - wp_y(wp);
            if (sqrt_(dx * dx + dy * dy) < t.reached) {
                wp += 1;
                if (wp >= nw) { sm = SC_SM_IDLE; gvalid = false; return; }
            }
        }
        gx = wp_x(wp); gy = wp_y(wp); gvalid = true;
    };

    for (int step = 0; step < p.n_steps; ++step) {
        const bool run = (ret == 0);
        if (run) {
            // ---- state machine / goal (tracking.py:569-577) ----------------------------------
            if (sm == SC_SM_STOP) {
                if (has_stopped<TC, MODEL>(th, v)) {
                    sm = t.enable_rotation ? SC_SM_ROTATE : SC_SM_TRACK;
                    update_goal();
                }
            } else {
                update_goal();
            }
        }
        // ---- the nearest unpassed obstacle (tracking.py:345-403, row 0): smallest centre distance among the unpassed rows, among all
        // rows when none is unpassed; strict < keeps the lower index on a tie, as the stable sorted insertion of tracking.hip does.
        // The KinematicBicycle2D family's unpassed cone is the full circle (|angle_normalize(.)| <= pi holds for every finite angle, and
        // a non-finite one leaves no row unpassed, which selects among all rows again), so only DynamicUnicycle2D evaluates the angle.
        TC bd_u = num<TC>::inf(), bd_a = num<TC>::inf();
        int bi_u = -1, bi_a = -1;
        for (int m = 0; m < M; ++m) {
            const TC ox = table[7 * m], oy = table[7 * m + 1];
            const TC dx = ox - x, dy = oy - y;
            const TC cd = sqrt_(dx * dx + dy * dy);
            if (cd < bd_a) { bd_a = cd; bi_a = m; }
            if constexpr (MODEL == SC_MODEL_DYNAMIC_UNICYCLE2D) {
                const TC ang = atan2_(oy - y, ox - x);
                const bool pass = fabs_(angle_normalize(ang - th)) <= half_unpassed;
                if (pass && cd < bd_u) { bd_u = cd; bi_u = m; }
            }
        }
        const int sel = (MODEL == SC_MODEL_DYNAMIC_UNICYCLE2D && bi_u >= 0) ? bi_u : bi_a;
        const bool has_obs = sel >= 0;
        // ---- the row, from the table as the selection saw it --------------------------------------
        const Agent<TC> agn = make_agent_m<TC, MODEL>(x, y, th, v);
        OdRow<TC> row = od_row_none<TC>();
        if (has_obs) row = od_build_row<TC, MODEL>(agn, table + 7 * sel, k);
        // moving obstacles advance AFTER the selection (dynamic_env/main.py:147-150): the solve sees the old table
        __syncthreads();
        if (t.dyn_obs) {
            for (int m = lane; m < M; m += 64) {
                table[7 * m] += table[7 * m + 3] * t.dt;
                table[7 * m + 1] += table[7 * m + 4] * t.dt;
            }
        }
        __syncthreads();
        // ---- nominal input (tracking.py:589-604) ------------------------------------------------
        TC ur0, ur1;
        if (sm == SC_SM_ROTATE) {
            const TC ga = atan2_(gy - y, gx - x);
            ur0 = TC(0); ur1 = TC(2) * angle_normalize(ga - th);           // rotate_to, k = 2
        } else if (!gvalid) {
            stop_input<TC, MODEL>(th, v, k_a_stop, ur0, ur1);               // stop(): its own gain
        } else {
            nominal_input<TC, MODEL>(x, y, th, v, gx, gy, t, ur0, ur1);     // k_omega, k_a, k_v = 3, .5, .5
        }
        // ---- solve (optimal_decay_cbf_qp.py:131-158), in every state-machine state -------------------
        TC u0, u1, w1, w2;
        const int st = od_solve<TC, REL2>(row, ur0, ur1, wr1, wr2, p1, p2, k, u0, u1, w1, w2);
        // ---- collision / status / step (tracking.py:627-646) ---------------------------------------
        // pre-step: infeasible or already colliding -> -2, the robot does not move
        const bool pre_fail = (st != SC_STATUS_OPTIMAL) || collides<TC>(x, y, table, M, k.R);
        TC nx, ny, nth, nv;
        robot_step<TC, MODEL>(agn, u0, u1, t.dt, t.Lr, t.v_min, t.v_max, nx, ny, nth, nv);
        int code;
        if (pre_fail) code = -2;
        else if (collides<TC>(nx, ny, table, M, k.R)) code = -2;             // post-step: the robot HAS moved
        else code = (!gvalid && sm != SC_SM_STOP) ? -1 : 0;                  // tracking.py:666-667
        if (run) {
            if (st == SC_STATUS_OPTIMAL) { om1 = w1; om2 = w2; }
            if (has_obs) hmin = fmin_(hmin, row.h);
            if (!pre_fail) { x = nx; y = ny; th = nth; v = nv; ul0 = u0; ul1 = u1; }
            if (code != 0) { ret = code; rstep = p.step_offset + step; }
        }
        if (active && traj_X) {
            TIO* tx = traj_X + ((size_t)step * B + agent) * 4;
            tx[0] = TIO(x); tx[1] = TIO(y); tx[2] = TIO(th); tx[3] = TIO(v);
        }
        if (active && traj_U) {
            TIO* tu = traj_U + ((size_t)step * B + agent) * 2;
            tu[0] = TIO(ul0); tu[1] = TIO(ul1);
        }
        if (active && traj_omega) {
            TIO* tw = traj_omega + ((size_t)step * B + agent) * 2;
            tw[0] = TIO(om1); tw[1] = TIO(om2);
        }
    }

    if (active) {
        X[agent * 4 + 0] = TIO(x); X[agent * 4 + 1] = TIO(y); X[agent * 4 + 2] = TIO(th); X[agent * 4 + 3] = TIO(v);
        wp_index[agent] = wp; state_machine[agent] = sm;
        goal[agent * 3 + 0] = TIO(gx); goal[agent * 3 + 1] = TIO(gy); goal[agent * 3 + 2] = gvalid ? TIO(1) : TIO(0);
        u_last[agent * 2 + 0] = TIO(ul0); u_last[agent * 2 + 1] = TIO(ul1);
        omega[agent * 2 + 0] = TIO(om1); omega[agent * 2 + 1] = TIO(om2);
        min_h[agent] = TIO(hmin);
        ret_out[agent] = ret; ret_step[agent] = rstep;
    }
}

hipError_t tracking_od_launch(const sc_tracking_od_params& p, long long B, int M, void* X, const void* wps, const int* n_wp,
                              int* wp_index, int* sm, void* goal, void* table, void* u_last, int* ret, int* ret_step,
                              void* tX, void* tU, void* omega, void* min_h, void* tW, hipStream_t stream) {
    const unsigned blocks = (unsigned)((B + 63) / 64);
    const size_t lds = (size_t)(M > 0 ? M : 1) * 7 * sizeof(double);
    hipError_t e = dispatch_io(p.track.qp.io_dtype, [&](auto tio) {
        return dispatch_int_last<SC_MODEL_DYNAMIC_UNICYCLE2D, SC_MODEL_KINEMATIC_BICYCLE2D, SC_MODEL_KINEMATIC_BICYCLE2D_C3BF,
                                 SC_MODEL_KINEMATIC_BICYCLE2D_DPCBF>(p.track.qp.model_id, [&](auto model) {
            // closed loops amplify rounding: arithmetic is always f64
            return launch(tracking_od_rollout_kernel<tag_t<decltype(tio)>, double, decltype(model)::value>, blocks, 64, lds, stream, p, B, M, X,
                          wps, n_wp, wp_index, sm, goal, table, u_last, ret, ret_step, tX, tU, omega, min_h, tW);
        });
    });
    if (e != hipSuccess || !p.track.dyn_obs || M == 0) return e;
    // every block advanced its own LDS copy: the stream-ordered follow-up writes the table where n_steps put it
    return advance_obstacle_table_launch(p.track.qp.io_dtype == SC_DTYPE_F32, table, M, p.track.n_steps, p.track.qp.dt, stream);
}

}  // namespace sc
