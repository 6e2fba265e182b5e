// The sensing loop's control_step split around the solve, for position controllers that are their own launch (MPC-CBF):
//   tracking_sense_select_kernel = tracking.py:569-609 with what tracking_sense_kernel (csrc/tracking_sense.hip) adds to it:
//                                  the integrators' heading, 'fov' detection, the memory of sighted rows, the combined candidates
//   tracking_sense_apply_kernel  = tracking.py:620-668: the attitude controller, both collision tests against the known table and
//                                  every unknown row, robot.step, the yaw step, return codes
// They are tracking_select_kernel / tracking_apply_kernel (csrc/tracking.hip) with those parts, and compute what they compute when
// there is no unknown row and no attitude controller.  One agent per lane; the known table [M,7], the unknown table [Mu,7] and the
// unknown rows' detection radii sit in LDS in tracking_sense_kernel's layout.  Both tables are static.
#include <hip/hip_runtime.h>

#include "sc_qp2.hpp"
#include "sc_dispatch.hpp"
#include "tracking_common.hpp"
#include "tracking_sense_common.hpp"

namespace sc {

template <typename TIO, typename TC, int KMAX, int MODEL>
__global__ __launch_bounds__(64) void tracking_sense_select_kernel(
        const sc_tracking_params p, const sc_sense_params sp, const long long B, const int M,
        const TIO* __restrict__ X, const TIO* __restrict__ waypoints, const int* __restrict__ n_wp,
        int* __restrict__ wp_index, int* __restrict__ state_machine, TIO* __restrict__ goal,
        const TIO* __restrict__ obs_table, const TIO* __restrict__ unknown_table, long long* __restrict__ seen,
        const TIO* __restrict__ yaw_in, TIO* __restrict__ u_att_io, const int* __restrict__ ret_in,
        TIO* __restrict__ obs_out, TIO* __restrict__ goal_out, TIO* __restrict__ u_ref_out, int* __restrict__ track_out) {
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

    TrackConsts<TC> t;
    t.reached = TC(p.reached_threshold); t.rot_thr = TC(p.rotation_threshold);
    t.v_max = TC(p.v_max); t.v_min = TC(p.v_min);
    t.k_omega = TC(p.k_omega); t.k_a = TC(p.k_a); t.k_v = TC(p.k_v);
    t.delta_max = TC(p.delta_max); t.wheel_base = TC(p.wheel_base); t.Lr = TC(p.qp.rear_ax_dist); t.dt = TC(p.qp.dt); t.a_max = TC(p.qp.u_max[0]);
    t.enable_rotation = p.enable_rotation; t.dyn_obs = 0; t.K = p.num_constraints;
    const SenseConsts s = make_sense_consts(sp);
    const TC pi = TC(3.14159265358979323846);
    const TC half_unpassed = (MODEL == SC_MODEL_DYNAMIC_UNICYCLE2D) ? TC(1.2) * pi / TC(2) : pi;   // tracking.py:352-357

    const TC x = TC(X[ag * 4 + 0]), y = TC(X[ag * 4 + 1]), th = TC(X[ag * 4 + 2]), v = TC(X[ag * 4 + 3]);
    int wp = wp_index[ag], sm = state_machine[ag];
    TC gx = TC(goal[ag * 3 + 0]), gy = TC(goal[ag * 3 + 1]);
    bool gvalid = goal[ag * 3 + 2] != TIO(0);
    const bool run = active && ret_in[ag] == 0;
    const int W = p.max_waypoints;
    const TIO* wps = waypoints + (p.waypoints_shared ? 0 : (size_t)ag * W * 2);
    const int nw = n_wp[p.waypoints_shared ? 0 : ag];
    unsigned long long mask = (unsigned long long)seen[ag];           // bit j: unknown row j is remembered
    const TC yaw = (INTEGRATOR && yaw_in) ? TC(yaw_in[ag]) : TC(0);    // the integrators' heading (robots/robot.py:66-72)
    TC u_att = (INTEGRATOR && u_att_io) ? TC(u_att_io[ag]) : num<TC>::nan();   // NaN: the reference's None
    const TC hd = INTEGRATOR ? yaw : th;                               // robot.get_orientation()

    auto wp_x = [&](int i) { return TC(wps[2 * i]); };
    auto wp_y = [&](int i) { return TC(wps[2 * i + 1]); };
    // tracking.py:497-535; the integrators turn `yaw`, and leaving 'rotate' drops u_att (:516-521)
    auto update_goal = [&]() {
        if (sm == SC_SM_ROTATE) {
            const int i = wp < nw ? wp : nw - 1;
            const TC rx = wp_x(i), ry = wp_y(i);
            const TC goal_angle = atan2_(ry - y, rx - x);
            if (!t.enable_rotation) sm = SC_SM_TRACK;
            if (fabs_(hd - goal_angle) > t.rot_thr) { gx = rx; gy = ry; gvalid = true; return; }
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
    if (run) {
        // ---- state machine / goal (tracking.py:569-577) --------------------------------------
        if (sm == SC_SM_STOP) {
            if (has_stopped<TC, MODEL>(th, v)) {
                sm = t.enable_rotation ? SC_SM_ROTATE : SC_SM_TRACK;
                update_goal();
            }
        } else {
            update_goal();
        }
        // ---- detection (tracking.py:580; robots/robot.py:799-834) ----------------------------
        unsigned long long now = 0ull;
        for (int j = 0; j < Mu; ++j)
            if (circle_in_fov(x, y, hd, utab[7 * j], utab[7 * j + 1], urad[j], s)) now |= 1ull << j;
        mask = s.persistent ? (mask | now) : now;
    }
    // ---- nearest unpassed obstacles (tracking.py:345-403): K smallest centre distances over the known rows and the
    //      remembered unknown rows (candidate c >= M is unknown row c - M) ----------------------------------------------
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
    for (int m = 0; m < NC; ++m) {
        if (!is_cand(m)) continue;
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
    // ---- nominal input (tracking.py:589-604) ----------------------------------------------------
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
    if (active) {
        wp_index[agent] = wp; state_machine[agent] = sm;
        goal[agent * 3 + 0] = TIO(gx); goal[agent * 3 + 1] = TIO(gy); goal[agent * 3 + 2] = gvalid ? TIO(1) : TIO(0);
        seen[agent] = (long long)mask;
        if (INTEGRATOR && u_att_io) u_att_io[agent] = TIO(u_att);
        // obstacle rows for the solve, padded like MPCCBF.update_tvp (mpc_cbf.py:338-364)
        TIO* oo = obs_out + (size_t)agent * t.K * 7;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            if (j >= t.K) break;
            const bool have = si[j] >= 0;
            const int sj = have ? si[j] : 0;
            const bool unk = have && sj >= M;                            // a remembered unknown row: [x, y, r, 0, 0, 0, 0]
            const TC* orow = table + 7 * sj;
#pragma unroll
            for (int f = 0; f < 7; ++f) {
                TC val = orow[f];
                if (unk && f == 2) val = urad[sj - M];
                if (unk && f > 2) val = TC(0);
                oo[j * 7 + f] = have ? TIO(val) : (f < 2 ? TIO(1000) : TIO(0));
            }
        }
        goal_out[agent * 2 + 0] = TIO(gvalid ? gx : x); goal_out[agent * 2 + 1] = TIO(gvalid ? gy : y);
        u_ref_out[agent * 2 + 0] = TIO(ur0); u_ref_out[agent * 2 + 1] = TIO(ur1);
        track_out[agent] = (run && sm == SC_SM_TRACK && gvalid) ? 1 : 0;
    }
}

template <typename TIO, typename TC, int MODEL>
__global__ __launch_bounds__(64) void tracking_sense_apply_kernel(
        const sc_tracking_params p, const sc_sense_params sp, const long long B, const int M, const int step_index,
        TIO* __restrict__ X, const int* __restrict__ state_machine, const TIO* __restrict__ goal,
        const TIO* __restrict__ obs_table, const TIO* __restrict__ unknown_table, TIO* __restrict__ yaw_io,
        TIO* __restrict__ u_att_io, const TIO* __restrict__ u, const int* __restrict__ u_status,
        TIO* __restrict__ u_last, int* __restrict__ ret_out, int* __restrict__ ret_step) {
    constexpr bool INTEGRATOR = MODEL == SC_MODEL_SINGLE_INTEGRATOR2D || MODEL == SC_MODEL_DOUBLE_INTEGRATOR2D;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int Mu = sp.n_unknown;
    TC* table = reinterpret_cast<TC*>(smem_raw);                     // [M][7] known rows, then [Mu][7] unknown rows
    TC* utab = table + (size_t)M * 7;
    const int lane = threadIdx.x;
    const long long agent = (long long)blockIdx.x * 64 + lane;
    const bool active = agent < B;
    const long long ag = active ? agent : 0;
    for (int e = lane; e < M * 7; e += 64) table[e] = TC(obs_table[e]);
    for (int e = lane; e < Mu * 7; e += 64) utab[e] = TC(unknown_table[e]);
    __syncthreads();

    const TC R = TC(p.qp.robot_radius);                              // CbfConsts::R
    const SenseConsts s = make_sense_consts(sp);
    const TC dt = TC(p.qp.dt), Lr = TC(p.qp.rear_ax_dist);
    const bool rotates = INTEGRATOR && p.enable_rotation && sp.att_type != SC_ATT_NONE;   // tracking.py:156: att_controller is not None
    const TC x = TC(X[ag * 4 + 0]), y = TC(X[ag * 4 + 1]), th = TC(X[ag * 4 + 2]), v = TC(X[ag * 4 + 3]);
    const int sm = state_machine[ag];
    const bool gvalid = goal[ag * 3 + 2] != TIO(0);
    const TC u0 = TC(u[ag * 2 + 0]), u1 = TC(u[ag * 2 + 1]);
    const int st = u_status ? u_status[ag] : SC_STATUS_OPTIMAL;
    const bool run = active && ret_out[ag] == 0;
    TC yaw = (INTEGRATOR && yaw_io) ? TC(yaw_io[ag]) : TC(0);
    TC u_att = (INTEGRATOR && u_att_io) ? TC(u_att_io[ag]) : num<TC>::nan();

    // tracking.py:451-460: every unknown row, sighted or not, as the circle of its own radius
    auto collides_unknown = [&](const TC px, const TC py) {
        bool hit = false;
        for (int j = 0; j < Mu; ++j) {
            const TC dx = px - utab[7 * j], dy = py - utab[7 * j + 1];
            hit |= sqrt_(dx * dx + dy * dy) < utab[7 * j + 2] + R;
        }
        return hit;
    };
    // ---- attitude controller (tracking.py:620-624), in 'track' only, from the applied input and the pre-step state ----
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
    const Agent<TC> agn = make_agent_m<TC, MODEL>(x, y, th, v);
    const bool pre_fail = (st != SC_STATUS_OPTIMAL) || collides<TC>(x, y, table, M, R) || collides_unknown(x, y);
    TC nx, ny, nth, nv;
    robot_step<TC, MODEL>(agn, u0, u1, dt, Lr, TC(p.v_min), TC(p.v_max), nx, ny, nth, nv);
    int code;
    if (pre_fail) code = -2;
    else if (collides<TC>(nx, ny, table, M, R) || collides_unknown(nx, ny)) code = -2;   // post-step: the robot HAS moved
    else code = (!gvalid && sm != SC_SM_STOP) ? -1 : 0;                  // tracking.py:666-667
    if (run) {
        if (!pre_fail) {
            X[agent * 4 + 0] = TIO(nx); X[agent * 4 + 1] = TIO(ny); X[agent * 4 + 2] = TIO(nth); X[agent * 4 + 3] = TIO(nv);
            u_last[agent * 2 + 0] = TIO(u0); u_last[agent * 2 + 1] = TIO(u1);
            if constexpr (INTEGRATOR) {                                  // robots/robot.py:446-448, step_rotate
                if (u_att == u_att) yaw = angle_normalize(yaw + u_att * dt);
                if (yaw_io) yaw_io[agent] = TIO(yaw);
            } else {
                if (yaw_io) yaw_io[agent] = TIO(nth);                    // DynamicUnicycle2D looks along X[2]
            }
        }
        if (INTEGRATOR && u_att_io) u_att_io[agent] = TIO(u_att);
        if (code != 0) { ret_out[agent] = code; ret_step[agent] = step_index; }
    }
}

// LDS of both kernels: tracking_sense_kernel's layout, and never less than the one row that a padded slot of the selection reads
static size_t sense_lds_bytes(int M, int Mu) {
    const size_t rows = (size_t)M * 7 + (size_t)Mu * 8;
    return ((rows > 7 ? rows : 7) + 1) * sizeof(double);
}

hipError_t tracking_sense_select_launch(const sc_tracking_params& p, const sc_sense_params& sp, long long B, int M, const void* X,
                                        const void* wps, const int* n_wp, int* wp_index, int* sm, void* goal, const void* table,
                                        const void* utable, long long* seen, const void* yaw, void* u_att, const int* ret,
                                        void* obs_out, void* goal_out, void* u_ref_out, int* track_out, hipStream_t stream) {
    const unsigned blocks = (unsigned)((B + 63) / 64);
    const size_t lds = sense_lds_bytes(M, sp.n_unknown);
    // arithmetic in f64 (closed loops amplify rounding), storage follows io_dtype -- as tracking_select_launch
    return dispatch_io(p.qp.io_dtype, [&](auto tio) {
        return dispatch_int_last<SC_MODEL_SINGLE_INTEGRATOR2D, SC_MODEL_DOUBLE_INTEGRATOR2D, SC_MODEL_DYNAMIC_UNICYCLE2D>(p.qp.model_id, [&](auto model) {
            auto go = [&](auto kmax) {
                return launch(tracking_sense_select_kernel<tag_t<decltype(tio)>, double, decltype(kmax)::value, decltype(model)::value>, blocks,
                              64, lds, stream, p, sp, B, M, X, wps, n_wp, wp_index, sm, goal, table, utable, seen, yaw, u_att, ret, obs_out,
                              goal_out, u_ref_out, track_out);
            };
            if (p.num_constraints <= 8) return go(int_tag<8>{});
            return go(int_tag<16>{});
        });
    });
}

hipError_t tracking_sense_apply_launch(const sc_tracking_params& p, const sc_sense_params& sp, long long B, int M, int step_index,
                                       void* X, const int* sm, const void* goal, const void* table, const void* utable, void* yaw,
                                       void* u_att, const void* u, const int* u_status, void* u_last, int* ret, int* ret_step,
                                       hipStream_t stream) {
    const unsigned blocks = (unsigned)((B + 63) / 64);
    const size_t lds = sense_lds_bytes(M, sp.n_unknown);
    return dispatch_io(p.qp.io_dtype, [&](auto tio) {
        return dispatch_int_last<SC_MODEL_SINGLE_INTEGRATOR2D, SC_MODEL_DOUBLE_INTEGRATOR2D, SC_MODEL_DYNAMIC_UNICYCLE2D>(p.qp.model_id, [&](auto model) {
            return launch(tracking_sense_apply_kernel<tag_t<decltype(tio)>, double, decltype(model)::value>, blocks, 64, lds, stream, p, sp, B, M,
                          step_index, X, sm, goal, table, utable, yaw, u_att, u, u_status, u_last, ret, ret_step);
        });
    });
}

}  // namespace sc
