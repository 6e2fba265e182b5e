// Fused closed-loop control_step with a camera cone and a heading of its own: one launch = n_steps iterations of
//   LocalTrackingController.control_step        tracking.py:559-668
// including the three parts tracking_rollout_kernel (csrc/tracking.hip) leaves out:
//   unknown obstacles   tracking.py:277-293, :580; utils/detection.py:28-87 ('fov' mode); robots/robot.py:773-834
//   their collisions    tracking.py:445-460 (every unknown row, sighted or not)
//   the integrators' yaw / u_att and the attitude controllers
//                       tracking.py:506-521, :589-594, :620-624; robots/robot.py:441-448;
//                       attitude_control/simple_attitude.py, attitude_control/velocity_tracking_yaw.py:35-64
// One agent per lane, as tracking_rollout_kernel: the agent's state (X, waypoint index, state machine, goal, yaw, u_att and the
// 64-bit mask of sighted rows) lives in registers for the whole rollout; the known table [M,7], the unknown table [Mu,7] and the
// unknown rows' detection radii live in LDS.  Both tables are static.  Polygon geometry ('ray' detection, sensing footprints,
// return code 1, the visibility / gatekeeper attitude controllers) is not built.
#include <hip/hip_runtime.h>

#include "sc_qp2.hpp"
#include "sc_dispatch.hpp"
#include "tracking_common.hpp"
#include "tracking_sense_common.hpp"

namespace sc {

template <typename TIO, typename TC, int KMAX, int MODEL>
__global__ __launch_bounds__(64) void tracking_sense_kernel(
        const sc_tracking_params p, const sc_sense_params sp, const long long B, const int M,
        TIO* __restrict__ X, const TIO* __restrict__ waypoints, const int* __restrict__ n_wp,
        int* __restrict__ wp_index, int* __restrict__ state_machine, TIO* __restrict__ goal,
        const TIO* __restrict__ obs_table, const TIO* __restrict__ unknown_table, long long* __restrict__ seen,
        TIO* __restrict__ yaw_io, TIO* __restrict__ u_att_io, TIO* __restrict__ u_last,
        int* __restrict__ ret_out, int* __restrict__ ret_step,
        TIO* __restrict__ traj_X, TIO* __restrict__ traj_U, TIO* __restrict__ traj_yaw, long long* __restrict__ traj_seen) {
    constexpr bool INTEGRATOR = MODEL == SC_MODEL_SINGLE_INTEGRATOR2D || MODEL == SC_MODEL_DOUBLE_INTEGRATOR2D;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int Mu = sp.n_unknown;
    TC* table = reinterpret_cast<TC*>(smem_raw);                     // [M][7] known rows, then ..
    TC* utab = table + (size_t)M * 7;                                 // .. [Mu][7] unknown rows as given: candidate c is row c of both
    TC* urad = utab + (size_t)Mu * 7;                                 // [Mu] radius of the circle a sighted row is taken for
    const int lane = threadIdx.x;
    const long long agent = (long long)blockIdx.x * 64 + lane;
    const bool active = agent < B;
    const long long ag = active ? agent : 0;

    for (int e = lane; e < M * 7; e += 64) table[e] = TC(obs_table[e]);
    for (int e = lane; e < Mu * 7; e += 64) utab[e] = TC(unknown_table[e]);
    for (int j = lane; j < Mu; j += 64) {                             // detection.py:65-69: a superellipsoid is seen as its outer circle
        const TC a = TC(unknown_table[7 * j + 2]), b = TC(unknown_table[7 * j + 3]);
        urad[j] = (TC(unknown_table[7 * j + 6]) >= TC(0.5)) ? fmax_(fmax_(a, b), TC(0)) : a;
    }
    __syncthreads();

    const CbfConsts<TC> k = make_consts<TC>(p.qp);
    TrackConsts<TC> t;
    t.reached = TC(p.reached_threshold); t.rot_thr = TC(p.rotation_threshold);
    t.v_max = TC(p.v_max); t.v_min = TC(p.v_min);
    t.k_omega = TC(p.k_omega); t.k_a = TC(p.k_a); t.k_v = TC(p.k_v);
    t.delta_max = TC(p.delta_max); t.wheel_base = TC(p.wheel_base); t.Lr = TC(p.qp.rear_ax_dist); t.dt = TC(p.qp.dt); t.a_max = TC(p.qp.u_max[0]);
    t.enable_rotation = p.enable_rotation; t.dyn_obs = 0; t.K = p.num_constraints;
    SenseConsts s;
    s.half_fov = sp.fov_angle / 2; s.cam_range = sp.cam_range; s.w_max = sp.w_max; s.att_kp = sp.att_kp;
    s.att_preview = sp.att_preview_time; s.simple_rate = sp.simple_yaw_rate;
    s.n_unknown = Mu; s.persistent = sp.persistent; s.att_type = sp.att_type;
    const bool rotates = INTEGRATOR && p.enable_rotation && sp.att_type != SC_ATT_NONE;   // tracking.py:156: att_controller is not None
    const TC pi = TC(3.14159265358979323846);
    const TC half_unpassed = (MODEL == SC_MODEL_DYNAMIC_UNICYCLE2D) ? TC(1.2) * pi / TC(2) : pi;   // tracking.py:352-357

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
    unsigned long long mask = (unsigned long long)seen[ag];           // bit j: unknown row j is remembered
    TC yaw = (INTEGRATOR && yaw_io) ? TC(yaw_io[ag]) : TC(0);         // the integrators' heading (robots/robot.py:66-72)
    TC u_att = (INTEGRATOR && u_att_io) ? TC(u_att_io[ag]) : num<TC>::nan();   // NaN: the reference's None

    auto wp_x = [&](int i) { return TC(wps[2 * i]); };
    auto wp_y = [&](int i) { return TC(wps[2 * i + 1]); };

    // tracking.py:497-535; the integrators turn `yaw`, and leaving 'rotate' drops u_att (:516-521)
    auto update_goal = [&]() {
        if (sm == SC_SM_ROTATE) {
            const int i = wp < nw ? wp : nw - 1;
            const TC rx = wp_x(i), ry = wp_y(i);
            const TC goal_angle = atan2_(ry - y, rx - x);
            if (!t.enable_rotation) sm = SC_SM_TRACK;
            const TC cur = INTEGRATOR ? yaw : th;
            if (fabs_(cur - goal_angle) > t.rot_thr) { gx = rx; gy = ry; gvalid = true; return; }
            sm = SC_SM_TRACK;
            if constexpr (INTEGRATOR) u_att = num<TC>::nan();
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
    // tracking.py:451-460: every unknown row, sighted or not, as the circle of its own radius
    auto collides_unknown = [&](const TC px, const TC py) {
        bool hit = false;
        for (int j = 0; j < Mu; ++j) {
            const TC dx = px - utab[7 * j], dy = py - utab[7 * j + 1];
            hit |= sqrt_(dx * dx + dy * dy) < utab[7 * j + 2] + k.R;
        }
        return hit;
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
        const TC hd = INTEGRATOR ? yaw : th;                             // robot.get_orientation()
        // ---- detection (tracking.py:580; robots/robot.py:799-834) -------------------------------
        if (run) {
            unsigned long long now = 0ull;
            for (int j = 0; j < Mu; ++j)
                if (circle_in_fov(x, y, hd, utab[7 * j], utab[7 * j + 1], urad[j], s)) now |= 1ull << j;
            mask = s.persistent ? (mask | now) : now;
        }
        // ---- nearest unpassed obstacles (tracking.py:345-403): K smallest centre distances over the known rows and the
        //      remembered unknown rows (candidate c >= M is unknown row c - M) --------------------------------------------
        TC sd[KMAX];
        int si[KMAX];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) { sd[j] = num<TC>::inf(); si[j] = -1; }
        const int NC = M + Mu;
        auto is_cand = [&](int c) { return c < M || ((mask >> (c - M)) & 1ull) != 0ull; };
        int n_unpassed = 0;
        for (int m = 0; m < NC; ++m) {
            if (!is_cand(m)) continue;
            const TC ang = atan2_(table[7 * m + 1] - y, table[7 * m] - x);
            n_unpassed += (fabs_(angle_normalize(ang - hd)) <= half_unpassed) ? 1 : 0;
        }
        const bool use_all = n_unpassed == 0;
        int n_cand = 0;
        for (int m = 0; m < NC; ++m) {
            if (!is_cand(m)) continue;
            n_cand += 1;
            const TC ox = table[7 * m], oy = table[7 * m + 1];
            const TC ang = atan2_(oy - y, ox - x);
            const bool pass = use_all || (fabs_(angle_normalize(ang - hd)) <= half_unpassed);
            const TC dx = ox - x, dy = oy - y;
            TC cd = pass ? sqrt_(dx * dx + dy * dy) : num<TC>::inf();
            int ci = pass ? m : -1;
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
        // ---- rows in registers (selection order = distance order, as the reference passes them) ---
        const Agent<TC> agn = make_agent_m<TC, MODEL>(x, y, th, v);
        TC n0[KMAX], n1[KMAX], c[KMAX];
        bool bad_obs = false;
        TC poison = TC(0);
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            const bool used = (j < t.K) && (si[j] >= 0);
            const int sj = si[j] >= 0 ? si[j] : 0;
            const TC* orow = table + 7 * sj;
            TC o[7];
#pragma unroll
            for (int f = 0; f < 7; ++f) o[f] = orow[f];
            if (sj >= M) {                                               // a remembered unknown row: [x, y, r, 0, 0, 0, 0]
                o[2] = urad[sj - M];
                o[3] = TC(0); o[4] = TC(0); o[5] = TC(0); o[6] = TC(0);
            }
            TC h, a0, a1, cc;
            const bool ok = cbf_row<TC, MODEL, true>(agn, o, k, a0, a1, cc, h);
            bad_obs |= used && !ok;
            a0 = used ? a0 : TC(0); a1 = used ? a1 : TC(0); cc = used ? cc : TC(0);
            normalise_row(a0, a1, cc, poison);
            n0[j] = a0; n1[j] = a1; c[j] = cc;
        }
        // ---- nominal input (tracking.py:589-604) ------------------------------------------------
        TC ur0, ur1;
        if (sm == SC_SM_ROTATE) {
            const TC ga = atan2_(gy - y, gx - x);
            if constexpr (INTEGRATOR) {                                      // :592-594: the yaw rate turns, the position input brakes
                if (run) u_att = fmin_(fmax_(TC(2) * angle_normalize(ga - yaw), -s.w_max), s.w_max);
                stop_input<TC, MODEL>(th, v, t.k_a, ur0, ur1);
            } else {
                ur0 = TC(0); ur1 = TC(2) * angle_normalize(ga - th);       // rotate_to, k = 2
            }
        } else if (!gvalid) {
            stop_input<TC, MODEL>(th, v, t.k_a, ur0, ur1);                  // stop()
        } else {
            nominal_input<TC, MODEL>(x, y, th, v, gx, gy, t, ur0, ur1);
        }
        // ---- solve (cbf_qp.py:108-199) -----------------------------------------------------------
        TC u0, u1;
        int st;
        if (n_cand == 0) { u0 = ur0; u1 = ur1; st = SC_STATUS_OPTIMAL; }    // obs_list None: u_ref unclipped
        else {
            st = qp2_solve<TC, KMAX>(n0, n1, c, t.K, ur0, ur1, poison, k, u0, u1);
            if (bad_obs) st = SC_STATUS_BAD_OBSTACLE;
        }
        // ---- attitude controller (tracking.py:620-624), in 'track' only -----------------------------
        if constexpr (INTEGRATOR) {
            if (run && rotates && sm == SC_SM_TRACK) {
                if (s.att_type == SC_ATT_SIMPLE) u_att = s.simple_rate;      // simple_attitude.py
                else {                                                      // velocity_tracking_yaw.py:35-64
                    TC vx, vy;
                    if constexpr (MODEL == SC_MODEL_SINGLE_INTEGRATOR2D) { vx = u0; vy = u1; }
                    else {
                        vx = th; vy = v;                                    // X[2:4]
                        if (s.att_preview > TC(0)) { vx = vx + s.att_preview * u0; vy = vy + s.att_preview * u1; }
                    }
                    if (sqrt_(vx * vx + vy * vy) < TC(1e-2)) u_att = TC(0);
                    else u_att = fmin_(fmax_(s.att_kp * angle_normalize(atan2_(vy, vx) - yaw), -s.w_max), s.w_max);
                }
            }
        }
        // ---- collision / status / step (tracking.py:627-646) ---------------------------------------
        // pre-step: infeasible or already colliding -> -2, the robot does not move
        const bool pre_fail = (st != SC_STATUS_OPTIMAL) || collides<TC>(x, y, table, M, k.R) || collides_unknown(x, y);
        TC nx, ny, nth, nv;
        robot_step<TC, MODEL>(agn, u0, u1, t.dt, t.Lr, t.v_min, t.v_max, nx, ny, nth, nv);
        int code;
        if (pre_fail) code = -2;
        else if (collides<TC>(nx, ny, table, M, k.R) || collides_unknown(nx, ny)) code = -2;   // post-step: the robot HAS moved
        else code = (!gvalid && sm != SC_SM_STOP) ? -1 : 0;                  // tracking.py:666-667
        if (run) {
            if (!pre_fail) {
                x = nx; y = ny; th = nth; v = nv; ul0 = u0; ul1 = u1;
                if constexpr (INTEGRATOR) {                                  // robots/robot.py:446-448, step_rotate
                    if (u_att == u_att) yaw = angle_normalize(yaw + u_att * t.dt);
                }
            }
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
        if (active && traj_yaw) traj_yaw[(size_t)step * B + agent] = TIO(INTEGRATOR ? yaw : th);
        if (active && traj_seen) traj_seen[(size_t)step * B + agent] = (long long)mask;
    }

    if (active) {
        X[agent * 4 + 0] = TIO(x); X[agent * 4 + 1] = TIO(y); X[agent * 4 + 2] = TIO(th); X[agent * 4 + 3] = TIO(v);
        wp_index[agent] = wp; state_machine[agent] = sm;
        goal[agent * 3 + 0] = TIO(gx); goal[agent * 3 + 1] = TIO(gy); goal[agent * 3 + 2] = gvalid ? TIO(1) : TIO(0);
        u_last[agent * 2 + 0] = TIO(ul0); u_last[agent * 2 + 1] = TIO(ul1);
        ret_out[agent] = ret; ret_step[agent] = rstep;
        seen[agent] = (long long)mask;
        if (yaw_io) yaw_io[agent] = TIO(INTEGRATOR ? yaw : th);
        if (INTEGRATOR && u_att_io) u_att_io[agent] = TIO(u_att);
    }
}

hipError_t tracking_sense_launch(const sc_tracking_params& p, const sc_sense_params& sp, long long B, int M, void* X, const void* wps,
                                 const int* n_wp, int* wp_index, int* sm, void* goal, const void* table, const void* utable,
                                 long long* seen, void* yaw, void* u_att, void* u_last, int* ret, int* ret_step, void* tX, void* tU,
                                 void* tYaw, long long* tSeen, hipStream_t stream) {
    const unsigned blocks = (unsigned)((B + 63) / 64);
    const size_t lds = ((size_t)M * 7 + (size_t)sp.n_unknown * 8 + 1) * sizeof(double);
    // arithmetic in f64 (closed loops amplify rounding), storage follows io_dtype -- as tracking_launch
    return dispatch_io(p.qp.io_dtype, [&](auto tio) {
        return dispatch_int_last<SC_MODEL_SINGLE_INTEGRATOR2D, SC_MODEL_DOUBLE_INTEGRATOR2D, SC_MODEL_DYNAMIC_UNICYCLE2D>(p.qp.model_id, [&](auto model) {
            auto go = [&](auto kmax) {
                return launch(tracking_sense_kernel<tag_t<decltype(tio)>, double, decltype(kmax)::value, decltype(model)::value>, blocks, 64, lds,
                              stream, p, sp, B, M, X, wps, n_wp, wp_index, sm, goal, table, utable, seen, yaw, u_att, u_last, ret, ret_step,
                              tX, tU, tYaw, tSeen);
            };
            if (p.num_constraints <= 8) return go(int_tag<8>{});
            return go(int_tag<16>{});
        });
    });
}

}  // namespace sc
