// Fused closed-loop control_step for B agents: one launch = n_steps iterations of
//   LocalTrackingController.control_step        tracking.py:559-668
//   LocalTrackingControllerDyn.control_step     dynamic_env/main.py:126-236 (moving obstacles)
// with the CBF-QP row builders / solver of the solve kernels behind the boundary.  One agent per
// lane; the agent's state (X, waypoint index, state machine, goal) lives in registers for the
// whole rollout; the shared obstacle table lives in LDS (and moves there when dyn_obs).
// The rollout kernels themselves (tracking_rollout_kernel, tracking_coop_kernel) and their dispatch are in tracking_kernels.hpp,
// which tracking_agents.hip instantiates a second time with per-agent parameters.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "tracking_kernels.hpp"

namespace sc {

// ======================================================================================
// control_step split around the solve, for position controllers that are their own launch (MPC-CBF, optimal-decay
// MPC-CBF): `select` is everything before pos_controller.solve_control_problem (tracking.py:569-609), `apply`
// everything after it (:627-668).  One agent per lane (the solve between them dominates).
template <typename TIO, typename TC, int KMAX, int MODEL>
__global__ __launch_bounds__(64) void tracking_select_kernel(
        const sc_tracking_params p, const long long B, const int M,
        const TIO* __restrict__ X, const TIO* __restrict__ waypoints, const int* __restrict__ n_wp,
        int* __restrict__ wp_index, int* __restrict__ state_machine, TIO* __restrict__ goal,
        const TIO* __restrict__ obs_table, const int* __restrict__ ret_in,
        TIO* __restrict__ obs_out, TIO* __restrict__ goal_out, TIO* __restrict__ u_ref_out, int* __restrict__ track_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    TC* table = reinterpret_cast<TC*>(smem_raw);                     // [M][7]
    const int lane = threadIdx.x;
    const long long agent = (long long)blockIdx.x * 64 + lane;
    const bool active = agent < B;
    const long long ag = active ? agent : 0;
    for (int e = lane; e < M * 7; e += 64) table[e] = TC(obs_table[e]);
    __syncthreads();

    TrackConsts<TC> t;
    t.reached = TC(p.reached_threshold); t.rot_thr = TC(p.rotation_threshold);
    t.v_max = TC(p.v_max); t.v_min = TC(p.v_min);
    t.k_omega = TC(p.k_omega); t.k_a = TC(p.k_a); t.k_v = TC(p.k_v);
    t.delta_max = TC(p.delta_max); t.wheel_base = TC(p.wheel_base); t.Lr = TC(p.qp.rear_ax_dist); t.dt = TC(p.qp.dt); t.a_max = TC(p.qp.u_max[0]);
    t.enable_rotation = p.enable_rotation; t.dyn_obs = 0; t.K = p.num_constraints;
    const TC pi = TC(3.14159265358979323846);
    const TC half_unpassed = (MODEL == SC_MODEL_DYNAMIC_UNICYCLE2D) ? TC(1.2) * pi / TC(2) : pi;

    const TC x = TC(X[ag * 4 + 0]), y = TC(X[ag * 4 + 1]), th = TC(X[ag * 4 + 2]), v = TC(X[ag * 4 + 3]);
    int wp = wp_index[ag], sm = state_machine[ag];
    TC gx = TC(goal[ag * 3 + 0]), gy = TC(goal[ag * 3 + 1]);
    bool gvalid = goal[ag * 3 + 2] != TIO(0);
    const bool run = active && ret_in[ag] == 0;
    const int W = p.max_waypoints;
    const TIO* wps = waypoints + (p.waypoints_shared ? 0 : (size_t)ag * W * 2);
    const int nw = n_wp[p.waypoints_shared ? 0 : ag];
    auto wp_x = [&](int i) { return TC(wps[2 * i]); };
    auto wp_y = [&](int i) { return TC(wps[2 * i + 1]); };
    auto update_goal = [&]() {                                       // tracking.py:497-535
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
    if (run) {
        if (sm == SC_SM_STOP) {
            if (has_stopped<TC, MODEL>(th, v)) {
                sm = t.enable_rotation ? SC_SM_ROTATE : SC_SM_TRACK;
                update_goal();
            }
        } else {
            update_goal();
        }
    }
    // nearest unpassed obstacles (tracking.py:345-403): K smallest centre distances
    TC sd[KMAX];
    int si[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) { sd[j] = num<TC>::inf(); si[j] = -1; }
    int n_unpassed = 0;
    for (int m = 0; m < M; ++m) {
        const TC ang = atan2_(table[7 * m + 1] - y, table[7 * m] - x);
        n_unpassed += (fabs_(angle_normalize(ang - th)) <= half_unpassed) ? 1 : 0;
    }
    const bool use_all = n_unpassed == 0;
    for (int m = 0; m < M; ++m) {
        const TC ox = table[7 * m], oy = table[7 * m + 1];
        const TC ang = atan2_(oy - y, ox - x);
        const bool pass = use_all || (fabs_(angle_normalize(ang - th)) <= half_unpassed);
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
    TC ur0, ur1;
    if (sm == SC_SM_ROTATE) {
        const TC ga = atan2_(gy - y, gx - x);
        ur0 = TC(0); ur1 = TC(2) * angle_normalize(ga - th);
    } else if (!gvalid) {
        stop_input<TC, MODEL>(th, v, t.k_a, ur0, ur1);
    } else {
        nominal_input<TC, MODEL>(x, y, th, v, gx, gy, t, ur0, ur1);
    }
    if (active) {
        wp_index[agent] = wp; state_machine[agent] = sm;
        goal[agent * 3 + 0] = TIO(gx); goal[agent * 3 + 1] = TIO(gy); goal[agent * 3 + 2] = gvalid ? TIO(1) : TIO(0);
        // obstacle rows for the solve, padded like MPCCBF.update_tvp (mpc_cbf.py:338-364)
        TIO* oo = obs_out + (size_t)agent * t.K * 7;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            if (j >= t.K) break;
            const bool have = si[j] >= 0;
            const TC* orow = table + 7 * (have ? si[j] : 0);
#pragma unroll
            for (int f = 0; f < 7; ++f) oo[j * 7 + f] = have ? TIO(orow[f]) : (f < 2 ? TIO(1000) : TIO(0));
        }
        goal_out[agent * 2 + 0] = TIO(gvalid ? gx : x); goal_out[agent * 2 + 1] = TIO(gvalid ? gy : y);
        u_ref_out[agent * 2 + 0] = TIO(ur0); u_ref_out[agent * 2 + 1] = TIO(ur1);
        track_out[agent] = (run && sm == SC_SM_TRACK && gvalid) ? 1 : 0;
    }
}

template <typename TIO, typename TC, int MODEL>
__global__ __launch_bounds__(64) void tracking_apply_kernel(
        const sc_tracking_params p, const long long B, const int M, const int step_index,
        TIO* __restrict__ X, const int* __restrict__ state_machine, const TIO* __restrict__ goal,
        const TIO* __restrict__ obs_table, const TIO* __restrict__ u, const int* __restrict__ u_status,
        TIO* __restrict__ u_last, int* __restrict__ ret_out, int* __restrict__ ret_step) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    TC* table = reinterpret_cast<TC*>(smem_raw);
    const int lane = threadIdx.x;
    const long long agent = (long long)blockIdx.x * 64 + lane;
    const bool active = agent < B;
    const long long ag = active ? agent : 0;
    for (int e = lane; e < M * 7; e += 64) table[e] = TC(obs_table[e]);
    __syncthreads();
    const CbfConsts<TC> k = make_consts<TC>(p.qp);
    const TC dt = TC(p.qp.dt), Lr = TC(p.qp.rear_ax_dist);
    const TC x = TC(X[ag * 4 + 0]), y = TC(X[ag * 4 + 1]), th = TC(X[ag * 4 + 2]), v = TC(X[ag * 4 + 3]);
    const int sm = state_machine[ag];
    const bool gvalid = goal[ag * 3 + 2] != TIO(0);
    const TC u0 = TC(u[ag * 2 + 0]), u1 = TC(u[ag * 2 + 1]);
    const int st = u_status ? u_status[ag] : SC_STATUS_OPTIMAL;
    const bool run = active && ret_out[ag] == 0;
    const Agent<TC> agn = make_agent_m<TC, MODEL>(x, y, th, v);
    const bool pre_fail = (st != SC_STATUS_OPTIMAL) || collides<TC>(x, y, table, M, k.R);
    TC nx, ny, nth, nv;
    robot_step<TC, MODEL>(agn, u0, u1, dt, Lr, TC(p.v_min), TC(p.v_max), nx, ny, nth, nv);
    int code;
    if (pre_fail) code = -2;
    else if (collides<TC>(nx, ny, table, M, k.R)) code = -2;
    else code = (!gvalid && sm != SC_SM_STOP) ? -1 : 0;
    if (run) {
        if (!pre_fail) {
            X[agent * 4 + 0] = TIO(nx); X[agent * 4 + 1] = TIO(ny); X[agent * 4 + 2] = TIO(nth); X[agent * 4 + 3] = TIO(nv);
            u_last[agent * 2 + 0] = TIO(u0); u_last[agent * 2 + 1] = TIO(u1);
        }
        if (code != 0) { ret_out[agent] = code; ret_step[agent] = step_index; }
    }
}

// Moving obstacles: every block of a rollout launch reads the table as it was at launch and advances its own LDS copy
// (a grid larger than one resident wave of blocks starts late blocks after early ones have finished, so nobody may
// write the table while the launch runs).  This stream-ordered follow-up leaves the table where n_steps of
// `obs[:, 0:2] += obs[:, 3:5] * dt` (dynamic_env/main.py:54-58) put it -- the same f64 additions in the same order.
template <typename TIO>
__global__ void advance_obstacle_table_kernel(TIO* __restrict__ obs_table, const int M, const int n_steps, const double dt) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    double x = double(obs_table[7 * m]), y = double(obs_table[7 * m + 1]);
    const double vx = double(obs_table[7 * m + 3]), vy = double(obs_table[7 * m + 4]);
    for (int s = 0; s < n_steps; ++s) { x += vx * dt; y += vy * dt; }
    obs_table[7 * m] = TIO(x); obs_table[7 * m + 1] = TIO(y);
}

// (also the follow-up of the optimal-decay rollout, csrc/tracking_od.hip)
hipError_t advance_obstacle_table_launch(bool f32, void* table, int M, int n_steps, double dt, hipStream_t stream) {
    const unsigned blocks = (unsigned)((M + 255) / 256);
    if (f32) hipLaunchKernelGGL(advance_obstacle_table_kernel<float>, dim3(blocks), dim3(256), 0, stream, (float*)table, M, n_steps, dt);
    else hipLaunchKernelGGL(advance_obstacle_table_kernel<double>, dim3(blocks), dim3(256), 0, stream, (double*)table, M, n_steps, dt);
    return hipGetLastError();
}

hipError_t tracking_select_launch(const sc_tracking_params& p, long long B, int M, const void* X, const void* wps,
                                  const int* n_wp, int* wp_index, int* sm, void* goal, const void* table, const int* ret,
                                  void* obs_out, void* goal_out, void* u_ref_out, int* track_out, hipStream_t stream) {
    const unsigned blocks = (unsigned)((B + 63) / 64);
    const size_t lds = (size_t)(M > 0 ? M : 1) * 7 * sizeof(double);
    return dispatch_io(p.qp.io_dtype, [&](auto tio) {
        return dispatch_int_last<SC_MODEL_DYNAMIC_UNICYCLE2D, SC_MODEL_UNICYCLE2D, SC_MODEL_SINGLE_INTEGRATOR2D,
                                 SC_MODEL_DOUBLE_INTEGRATOR2D, SC_MODEL_KINEMATIC_BICYCLE2D>(p.qp.model_id, [&](auto model) {
            auto go = [&](auto kmax) {
                return launch(tracking_select_kernel<tag_t<decltype(tio)>, double, decltype(kmax)::value, decltype(model)::value>, blocks, 64,
                              lds, stream, p, B, M, X, wps, n_wp, wp_index, sm, goal, table, ret, obs_out, goal_out, u_ref_out, track_out);
            };
            if (p.num_constraints <= 8) return go(int_tag<8>{});
            return go(int_tag<16>{});
        });
    });
}

hipError_t tracking_apply_launch(const sc_tracking_params& p, long long B, int M, int step_index, void* X, const int* sm,
                                 const void* goal, const void* table, const void* u, const int* u_status, void* u_last,
                                 int* ret, int* ret_step, hipStream_t stream) {
    const unsigned blocks = (unsigned)((B + 63) / 64);
    const size_t lds = (size_t)(M > 0 ? M : 1) * 7 * sizeof(double);
    return dispatch_io(p.qp.io_dtype, [&](auto tio) {
        return dispatch_int_last<SC_MODEL_DYNAMIC_UNICYCLE2D, SC_MODEL_UNICYCLE2D, SC_MODEL_SINGLE_INTEGRATOR2D,
                                 SC_MODEL_DOUBLE_INTEGRATOR2D, SC_MODEL_KINEMATIC_BICYCLE2D>(p.qp.model_id, [&](auto model) {
            return launch(tracking_apply_kernel<tag_t<decltype(tio)>, double, decltype(model)::value>, blocks, 64, lds, stream, p, B, M,
                          step_index, X, sm, goal, table, u, u_status, u_last, ret, ret_step);
        });
    });
}

hipError_t tracking_launch(const sc_tracking_params& p, long long B, int M, void* X, const void* wps, const int* n_wp,
                           int* wp_index, int* sm, void* goal, void* table, void* u_last, int* ret, int* ret_step,
                           void* tX, void* tU, hipStream_t stream) {
    return launch_track<false>(p, B, M, X, wps, n_wp, wp_index, sm, goal, table, u_last, ret, ret_step, tX, tU, stream);
}

// ======================================================================================
// Fleet step: agents are each other's moving obstacles (BASELINE configs[3] as a closed loop).  One launch = ONE
// LocalTrackingControllerDyn.control_step (dynamic_env/main.py:126-236) for every local agent, whose obstacle list is
//   obs_i = vstack(T, N_i)      T      the shared table [M,7] (staged in LDS)
//                               N_i    its K_nb nearest other agents [K_nb,7] as sc_neighbor_obstacles_batch_ws wrote them from
//                                      the published states P_t (padding rows, radius 0, are no candidates)
// Candidate c < M is table row c, c >= M neighbour row c - M: the (distance, index) rank of tracking_coop_kernel then breaks ties
// table first, neighbours in their distance order.  G lanes per agent, four candidates per lane (M + K_nb <= 4 G); selection,
// rows, cooperative QP walk and collision tests as in tracking_coop_kernel.  The collision tests use copies of all rows advanced
// by dt (main.py:54-58 runs after the selection); the table itself is advanced by the follow-up kernel when dyn_obs.
// Per agent it also keeps `cause` (0 none, 1 QP not optimal, 2 collision) and `min_sep`, the running minimum over the steps it
// ran of (distance to its nearest other agent in P_t) - 2 R, and publishes P_{t+1} = (x, y, th, ret == 0 ? v : 0) into X_pub.
// Every row is a circle [x, y, r, vx, vy, 0, 0] (columns 3, 4 are velocities, so there are no superellipsoid rows).
__device__ __forceinline__ double advance_row(const double p, const double v, const double dt) {
#pragma clang fp contract(off)
    return p + v * dt;                                                // numpy's obs[:, 0] += obs[:, 3] * dt: no fused multiply-add
}

template <typename TIO, typename TC, int G, int MODEL>
__global__ __launch_bounds__(64) void tracking_fleet_kernel(
        const sc_tracking_params p, const long long B, const int M, const int K_nb, const int step_index,
        TIO* __restrict__ X, TIO* __restrict__ X_pub, const TIO* __restrict__ waypoints, const int* __restrict__ n_wp,
        int* __restrict__ wp_index, int* __restrict__ state_machine, TIO* __restrict__ goal,
        const TIO* __restrict__ obs_table, const TIO* __restrict__ nb_rows, TIO* __restrict__ u_last,
        int* __restrict__ ret_out, int* __restrict__ ret_step, int* __restrict__ cause_out, TIO* __restrict__ min_sep) {
    constexpr int APW = 64 / G;                                       // agents per wave
    constexpr int CM = 4;                                             // candidates per lane (M + K_nb <= CM * G)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    TC* table = reinterpret_cast<TC*>(smem_raw);                     // [M][7]
    TC* nbs = table + (size_t)M * 7;                                  // [APW][K_nb][7]
    int* sel = reinterpret_cast<int*>(nbs + (size_t)APW * K_nb * 7 + (M == 0 && K_nb == 0 ? 1 : 0));   // [64]
    const int lane = threadIdx.x;
    const int sub = lane & (G - 1);
    const int grp_i = lane / G;
    const long long agent = (long long)blockIdx.x * APW + grp_i;
    const bool active = agent < B;
    const long long ag = active ? agent : 0;
    const unsigned long long grp = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << (lane & ~(G - 1));
    const int NC = M + K_nb;

    for (int e = lane; e < M * 7; e += 64) table[e] = TC(obs_table[e]);
    TC* nb = nbs + (size_t)grp_i * K_nb * 7;                          // this agent's rows: the group reads them coalesced
    for (int e = sub; e < K_nb * 7; e += G) nb[e] = TC(nb_rows[(size_t)ag * K_nb * 7 + e]);
    __syncthreads();

    const CbfConsts<TC> k = make_consts<TC>(p.qp);
    TrackConsts<TC> t;
    t.reached = TC(p.reached_threshold); t.rot_thr = TC(p.rotation_threshold);
    t.v_max = TC(p.v_max); t.v_min = TC(p.v_min);
    t.k_omega = TC(p.k_omega); t.k_a = TC(p.k_a); t.k_v = TC(p.k_v);
    t.delta_max = TC(p.delta_max); t.wheel_base = TC(p.wheel_base); t.Lr = TC(p.qp.rear_ax_dist); t.dt = TC(p.qp.dt); t.a_max = TC(p.qp.u_max[0]);
    t.enable_rotation = p.enable_rotation; t.dyn_obs = p.dyn_obs; t.K = p.num_constraints;
    const TC pi = TC(3.14159265358979323846);
    const TC half_unpassed = (MODEL == SC_MODEL_DYNAMIC_UNICYCLE2D) ? TC(1.2) * pi / TC(2) : pi;   // tracking.py:352-357

    TC x = TC(X[ag * 4 + 0]), y = TC(X[ag * 4 + 1]), th = TC(X[ag * 4 + 2]), v = TC(X[ag * 4 + 3]);
    int wp = wp_index[ag], sm = state_machine[ag];
    TC gx = TC(goal[ag * 3 + 0]), gy = TC(goal[ag * 3 + 1]);
    bool gvalid = goal[ag * 3 + 2] != TIO(0);
    int ret = ret_out[ag], rstep = ret_step[ag], cause = cause_out[ag];
    TC msep = TC(min_sep[ag]);
    const int W = p.max_waypoints;
    const TIO* wps = waypoints + (p.waypoints_shared ? 0 : (size_t)ag * W * 2);
    const int nw = n_wp[p.waypoints_shared ? 0 : ag];
    TC ul0 = TC(u_last[ag * 2 + 0]), ul1 = TC(u_last[ag * 2 + 1]);
    const bool run = active && ret == 0;

    auto wp_x = [&](int i) { return TC(wps[2 * i]); };
    auto wp_y = [&](int i) { return TC(wps[2 * i + 1]); };
    auto update_goal = [&]() {                                       // tracking.py:497-535
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
    auto group_any = [&](bool b) { return (__builtin_amdgcn_ballot_w64(b) & grp) != 0ull; };
    auto row_of = [&](int c) -> const TC* { return c < M ? table + 7 * c : nb + 7 * (c - M); };
    auto is_cand = [&](int c) { return c < M || (c < NC && nb[7 * (c - M) + 2] > TC(0)); };   // neighbour padding: radius 0
    auto collides_group = [&](TC px_, TC py_) {                       // against the rows advanced by dt
        bool hit = false;
#pragma unroll
        for (int q = 0; q < CM; ++q) {
            if (q * G >= NC) break;
            const int c = sub + q * G;
            if (is_cand(c)) {
                const TC* r = row_of(c);
                TC o[7];
#pragma unroll
                for (int f = 0; f < 7; ++f) o[f] = r[f];
                o[0] = advance_row(o[0], o[3], t.dt); o[1] = advance_row(o[1], o[4], t.dt);
                hit |= collides_one<TC>(px_, py_, o, k.R);
            }
        }
        return group_any(hit);
    };

    // ---- true separation from the nearest other agent in P_t (neighbour row 0: the search orders by distance) ----
    if (run && K_nb > 0 && nb[2] > TC(0)) {
        const TC dx = nb[0] - x, dy = nb[1] - y;
        msep = fmin_(msep, sqrt_(dx * dx + dy * dy) - TC(2) * k.R);
    }
    if (run) {
        if (sm == SC_SM_STOP) {                                       // tracking.py:569-577
            if (has_stopped<TC, MODEL>(th, v)) {
                sm = t.enable_rotation ? SC_SM_ROTATE : SC_SM_TRACK;
                update_goal();
            }
        } else {
            update_goal();
        }
    }
    // ---- nearest unpassed rows of vstack(T, N_i) (tracking.py:345-403) ---------------------------------
    TC cd[CM];
    int ci[CM];
    bool inview[CM];
    int cnt = 0, nvalid = 0;
#pragma unroll
    for (int q = 0; q < CM; ++q) { cd[q] = num<TC>::inf(); ci[q] = -1; inview[q] = false; }
#pragma unroll
    for (int q = 0; q < CM; ++q) {
        if (q * G >= NC) break;                                       // uniform: only ceil(NC / G) candidates per lane exist
        const int c = sub + q * G;
        const bool valid = is_cand(c);
        const TC* o = row_of(valid ? c : 0);
        const TC ox = valid ? o[0] : TC(0), oy = valid ? o[1] : TC(0);
        const TC ang = atan2_(oy - y, ox - x);
        inview[q] = valid && (fabs_(angle_normalize(ang - th)) <= half_unpassed);
        cnt += inview[q] ? 1 : 0;
        nvalid += valid ? 1 : 0;
        const TC dx = ox - x, dy = oy - y;
        cd[q] = sqrt_(dx * dx + dy * dy);
        ci[q] = valid ? c : -1;
    }
    const bool use_all = group_sum_int<TC, G>(cnt) == 0;
    const bool no_rows = group_sum_int<TC, G>(nvalid) == 0;           // obs_list None (cbf_qp.py:113-118)
#pragma unroll
    for (int q = 0; q < CM; ++q) {
        const bool pass = (ci[q] >= 0) && (use_all || inview[q]);
        cd[q] = pass ? cd[q] : num<TC>::inf();
        ci[q] = pass ? ci[q] : -1;
    }
    int rank[CM] = {0, 0, 0, 0};
    rank_round<TC, G, CM, 0>(cd, rank, sub, std::make_integer_sequence<int, G>{});
    if (NC > G) rank_round<TC, G, CM, 1>(cd, rank, sub, std::make_integer_sequence<int, G>{});
    if (NC > 2 * G) rank_round<TC, G, CM, 2>(cd, rank, sub, std::make_integer_sequence<int, G>{});
    if (NC > 3 * G) rank_round<TC, G, CM, 3>(cd, rank, sub, std::make_integer_sequence<int, G>{});
    sel[lane] = -1;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < CM; ++q)
        if (sub + q * G < NC && rank[q] < G) sel[(lane & ~(G - 1)) + rank[q]] = ci[q];
    __syncthreads();
    const int si = sel[lane];
    // ---- this lane's row (the rows as published: the solve sees them before they advance) ----------------
    const Agent<TC> agn = make_agent_m<TC, MODEL>(x, y, th, v);
    const bool used = (sub < t.K) && (si >= 0);
    TC a0, a1, cc;
    TC poison = TC(0);
    bool bad_mine;
    {
        const TC* orow = row_of(si >= 0 ? si : 0);
        TC o[7];
#pragma unroll
        for (int f = 0; f < 7; ++f) o[f] = (si >= 0) ? orow[f] : TC(0);
        TC h;
        const bool ok = cbf_row<TC, MODEL, true, true>(agn, o, k, a0, a1, cc, h);   // circles only: moving rows carry velocities
        bad_mine = used && !ok;
        a0 = used ? a0 : TC(0); a1 = used ? a1 : TC(0); cc = used ? cc : TC(0);
        normalise_row(a0, a1, cc, poison);
    }
    // ---- nominal input (tracking.py:589-604) ------------------------------------------------
    TC ur0, ur1;
    if (sm == SC_SM_ROTATE) {
        const TC ga = atan2_(gy - y, gx - x);
        ur0 = TC(0); ur1 = TC(2) * angle_normalize(ga - th);           // rotate_to, k = 2
    } else if (!gvalid) {
        stop_input<TC, MODEL>(th, v, t.k_a, ur0, ur1);                  // stop()
    } else {
        nominal_input<TC, MODEL>(x, y, th, v, gx, gy, t, ur0, ur1);
    }
    // ---- cooperative solve (cbf_qp.py:108-199) ---------------------------------------------------
    TC u0, u1;
    int st;
    if (no_rows) { u0 = ur0; u1 = ur1; st = SC_STATUS_OPTIMAL; }
    else {
        QpState<TC> S;
        qp_begin(S, ur0, ur1, k);
        if constexpr (G == 8) coop_solve_all8<TC>(S, t.K, sub, lane, a0, a1, cc, k);
        else coop_solve_all16<TC>(S, t.K, sub, lane, a0, a1, cc, k);
        qp_finish_box(S, k);
        TC worst = qp_row_margin(num<TC>::inf(), a0, a1, cc, S.u0, S.u1, poison);
        worst = group_min<TC, G>(worst);
        if (group_any(!(poison == poison))) poison = num<TC>::nan();
        st = qp_status(S, worst, poison, k);
        if (group_any(bad_mine)) st = SC_STATUS_BAD_OBSTACLE;
        u0 = S.u0; u1 = S.u1;
    }
    // ---- collision / status / step (tracking.py:627-646) ---------------------------------------
    const bool qp_fail = st != SC_STATUS_OPTIMAL;
    const bool pre_hit = collides_group(x, y);
    TC nx, ny, nth, nv;
    robot_step<TC, MODEL>(agn, u0, u1, t.dt, t.Lr, t.v_min, t.v_max, nx, ny, nth, nv);
    const bool post_hit = collides_group(nx, ny);
    int code, why = 0;
    if (qp_fail) { code = -2; why = 1; }
    else if (pre_hit || post_hit) { code = -2; why = 2; }               // post-step: the robot HAS moved
    else code = (!gvalid && sm != SC_SM_STOP) ? -1 : 0;                  // tracking.py:666-667
    if (run) {
        if (!qp_fail && !pre_hit) { x = nx; y = ny; th = nth; v = nv; ul0 = u0; ul1 = u1; }
        if (code != 0) { ret = code; rstep = step_index; cause = why; }
    }

    if (active && sub == 0) {
        X[agent * 4 + 0] = TIO(x); X[agent * 4 + 1] = TIO(y); X[agent * 4 + 2] = TIO(th); X[agent * 4 + 3] = TIO(v);
        X_pub[agent * 4 + 0] = TIO(x); X_pub[agent * 4 + 1] = TIO(y); X_pub[agent * 4 + 2] = TIO(th);
        X_pub[agent * 4 + 3] = ret == 0 ? TIO(v) : TIO(0);           // a frozen robot does not move
        wp_index[agent] = wp; state_machine[agent] = sm;
        goal[agent * 3 + 0] = TIO(gx); goal[agent * 3 + 1] = TIO(gy); goal[agent * 3 + 2] = gvalid ? TIO(1) : TIO(0);
        u_last[agent * 2 + 0] = TIO(ul0); u_last[agent * 2 + 1] = TIO(ul1);
        ret_out[agent] = ret; ret_step[agent] = rstep; cause_out[agent] = cause;
        min_sep[agent] = TIO(msep);
    }
}

hipError_t tracking_fleet_launch(const sc_tracking_params& p, long long B, int M, int K_nb, int step_index, void* X, void* X_pub,
                                 const void* wps, const int* n_wp, int* wp_index, int* sm, void* goal, void* table,
                                 const void* nb_rows, void* u_last, int* ret, int* ret_step, int* cause, void* min_sep, hipStream_t stream) {
    // arithmetic in f64 (closed loops amplify rounding), storage follows io_dtype -- as tracking_launch
    hipError_t e = dispatch_io(p.qp.io_dtype, [&](auto tio) {
        return dispatch_int_last<SC_MODEL_DYNAMIC_UNICYCLE2D, SC_MODEL_KINEMATIC_BICYCLE2D, SC_MODEL_KINEMATIC_BICYCLE2D_C3BF,
                                 SC_MODEL_KINEMATIC_BICYCLE2D_DPCBF>(p.qp.model_id, [&](auto model) {
            auto go = [&](auto g) {
                constexpr int G = decltype(g)::value, APW = 64 / G;
                const size_t lds = ((size_t)M * 7 + (size_t)APW * K_nb * 7 + 1) * sizeof(double) + 64 * sizeof(int);
                return launch<false>(tracking_fleet_kernel<tag_t<decltype(tio)>, double, G, decltype(model)::value>,
                                     (unsigned)((B + APW - 1) / APW), 64, lds, stream, p, B, M, K_nb, step_index, X, X_pub, wps, n_wp, wp_index, sm,
                                     goal, table, nb_rows, u_last, ret, ret_step, cause, min_sep);
            };
            if (p.num_constraints <= 8 && M + K_nb <= 32) return go(int_tag<8>{});
            return go(int_tag<16>{});
        });
    });
    if (e != hipSuccess || !p.dyn_obs || M == 0) return e;
    return advance_obstacle_table_launch(p.qp.io_dtype == SC_DTYPE_F32, table, M, 1, p.qp.dt, stream);
}

}  // namespace sc
