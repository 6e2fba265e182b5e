// The drift-car scenario of the reference on the device (examples/drift_car/test_drift.py): DynamicBicycle2D.step with the
// Fiala tyre, DriftingCar.step(X, U), LaneChangeController / StoppingController and the collision tests of a straight
// DriftingEnv.  Written statement for statement like the reference's scalar numpy code; a translation unit that includes
// this header is compiled WITHOUT floating-point contraction (the pragma below holds to its end).  The device's tan, atan,
// atan2, tanh, sin and cos are not glibc's to the last bit, so values agree with the CPU to rounding, not to the bit
// (DESIGN.md 9c).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/safe_control_amd.h"

#pragma clang fp contract(off)

namespace sc {
namespace drift {

constexpr double kPi = 3.141592653589793;
constexpr double kGravity = 9.81;                                 // dynamic_bicycle2D.py:88

struct Env {                      // constants of one launch
    double dt, R, sm;
    double a, b, m, Iz, Ccf, Ccr, rw, gamma, Fzf, Fzr;
    double dmax, tmax, rmax, bmax, vmin, vmax;
    double L, hw, cstep;
};

__device__ __forceinline__ Env make_env(const sc_drift_shield_params& p) {
    Env E;
    E.dt = p.dt; E.R = p.robot_radius; E.sm = p.safety_margin;
    E.a = p.a; E.b = p.b; E.m = p.m; E.Iz = p.Iz; E.Ccf = p.Cc_f; E.Ccr = p.Cc_r; E.rw = p.r_w; E.gamma = p.gamma;
    const double Lw = p.a + p.b;                                  // _compute_normal_forces (:93-101)
    E.Fzf = p.m * kGravity * p.b / Lw; E.Fzr = p.m * kGravity * p.a / Lw;
    E.dmax = p.delta_max; E.tmax = p.tau_max; E.rmax = p.r_max; E.bmax = p.beta_max; E.vmin = p.v_min; E.vmax = p.v_max;
    E.L = p.track_length; E.hw = p.track_width / 2;
    E.cstep = p.track_length / (SC_DRIFT_CENTER_SAMPLES - 1);     // np.linspace(0, L, 100): sample i = i * step, the last = L
    return E;
}

__device__ __forceinline__ double clip(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }
__device__ __forceinline__ double sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// x ** 3 the way libm's pow rounds it (one rounding): the product's error terms are carried with two fused operations
__device__ __forceinline__ double cube(double x) {
    const double x2 = x * x, e2 = __builtin_fma(x, x, -x2);
    const double p = x2 * x, e3 = __builtin_fma(x2, x, -p);
    return p + __builtin_fma(e2, x, e3);
}

// angle_normalize (dynamic_bicycle2D.py:23-26): Python's %, whose result has the divisor's sign
__device__ __forceinline__ double angle_normalize(double x) {
    double m = fmod(x + kPi, 2 * kPi);
    if (m != 0.0) { if (m < 0.0) m += 2 * kPi; } else { m = 0.0; }
    return m - kPi;
}

// _compute_lateral_force (dynamic_bicycle2D.py:179-197)
__device__ __forceinline__ double lateral_force(double alpha, double Cc, double Fz, double Fx, double mu, double gamma) {
    const double muFz = mu * Fz;
    const double Fy_max_sq = muFz * muFz - gamma * (Fx * Fx);
    const double Fy_max = sqrt(fmax(Fy_max_sq, 1.0));
    const double alpha_sl = atan(3 * Fy_max / Cc);
    const double ta = tan(alpha);
    if (fabs(alpha) < alpha_sl)
        return (-Cc * ta + (Cc * Cc / (3 * Fy_max)) * fabs(ta) * ta) - (cube(Cc) / (27 * (Fy_max * Fy_max))) * cube(ta);
    return -Fy_max * sign(alpha);
}

// DriftingCar.step(X, U) (drifting_car.py:500-522) around DynamicBicycle2D.step (:347-388, f :264-320), in place.
// X = x, y, theta, r, beta, V, delta, tau.  The position moves with the NEXT V, beta and the OLD theta.
__device__ __noinline__ void car_step(double* X, double u0, double u1, double mu, const Env& E) {
    const double r = X[3], beta = X[4], V = X[5], delta = X[6], tau = X[7];
    const double V_safe = fmax(V, 0.1);
    const double sb = sin(beta), cb = cos(beta);
    const double alpha_f = atan2(V * sb + E.a * r, V_safe * cb) - delta;
    const double alpha_r = atan2(V * sb - E.b * r, V_safe * cb);
    const double Fx_f = 0.0;
    const double F_lim = mu * E.Fzr;                              // _compute_longitudinal_force (:216-232)
    const double Fx_r = F_lim * tanh(tau / (E.rw * fmax(F_lim, 1.0)));
    const double Fy_f = lateral_force(alpha_f, E.Ccf, E.Fzf, Fx_f, mu, E.gamma);
    const double Fy_r = lateral_force(alpha_r, E.Ccr, E.Fzr, Fx_r, mu, E.gamma);
    const double sd = sin(delta), cd = cos(delta), sdb = sin(delta - beta), cdb = cos(delta - beta);
    const double r_dot = (E.a * (Fx_f * sd + Fy_f * cd) - E.b * Fy_r) / E.Iz;
    const double beta_dot = (Fx_f * sdb + Fy_f * cdb - Fx_r * sb + Fy_r * cb) / (E.m * V_safe) - r;
    const double V_dot = (Fx_f * cdb - Fy_f * sdb + Fx_r * cb + Fy_r * sb) / E.m;
    const double rn = clip(r + (r_dot + 0.0) * E.dt, -E.rmax, E.rmax);
    const double bn = clip(beta + (beta_dot + 0.0) * E.dt, -E.bmax, E.bmax);
    const double Vn = clip(V + (V_dot + 0.0) * E.dt, E.vmin, E.vmax);
    const double dn = clip(delta + (0.0 + u0) * E.dt, -E.dmax, E.dmax);
    const double tn = clip(tau + (0.0 + u1) * E.dt, -E.tmax, E.tmax);
    const double theta = X[2];
    const double vxg = Vn * cos(theta + bn), vyg = Vn * sin(theta + bn);
    X[0] = X[0] + vxg * E.dt; X[1] = X[1] + vyg * E.dt; X[2] = angle_normalize(theta + rn * E.dt);
    X[3] = rn; X[4] = bn; X[5] = Vn; X[6] = dn; X[7] = tn;
}

// LaneChangeController.compute_control (backup_controller.py:126-195) / StoppingController.compute_control (:305-354)
__device__ __forceinline__ void control(const double* X, const sc_drift_controller& c, double& delta_dot, double& tau_dot) {
    const double y = X[1], theta = X[2], r = X[3], beta = X[4], delta = X[6], tau = X[7];
    if (c.kind == SC_DRIFT_LANE_CHANGE) {
        const double V = fmax(X[5], 0.1);
        const double y_error = c.target_y - y;
        const double course = angle_normalize(theta + beta);
        const double vy = V * sin(course);
        const double theta_des = clip(atan(c.kp_y * y_error - c.kd_y * vy), -c.theta_des_max, c.theta_des_max);
        const double theta_error = angle_normalize(theta_des - course);
        const double delta_des = clip(c.kp_theta * theta_error - c.kd_theta * r, -c.delta_max, c.delta_max);
        delta_dot = clip(c.kp_delta * (delta_des - delta), -c.delta_dot_max, c.delta_dot_max);
        const double tau_des = clip(c.kp_v * (c.v_target - V), -c.tau_max, c.tau_max);
        tau_dot = clip(c.kp_tau_dot * (tau_des - tau), -c.tau_dot_max, c.tau_dot_max);
    } else {
        const double V = X[5];
        double tau_des = V > c.stop_velocity ? fmin(-c.kp_v * V, c.min_braking_torque) : c.holding_torque;
        tau_des = clip(tau_des, -c.tau_max, c.tau_max);
        const double tau_error = tau_des - tau;
        tau_dot = clip(5000.0 * sign(tau_error) * fmin(fabs(tau_error) / 50.0, 1.0), -c.tau_dot_max, c.tau_dot_max);
        const double delta_des = clip(-c.kd_theta * r, -c.delta_max, c.delta_max);
        delta_dot = clip(c.kp_delta * (delta_des - delta), -c.delta_dot_max, c.delta_dot_max);
    }
}

// x <- step(x, control(x)) under friction mu: one step of Gatekeeper._forward_simulate_backup (gatekeeper.py:271-307)
__device__ __forceinline__ void ctrl_step(double* X, const sc_drift_controller& c, double mu, const Env& E, double& u0, double& u1) {
    control(X, c, u0, u1);
    car_step(X, u0, u1, mu, E);
}

// DriftingEnv.check_collision (drifting_env.py:340-371) on a straight track: the nearest centre-line sample (np.argmin: the
// first minimum), then dist_from_center + radius > half_width.  Only the samples around x / step can be the nearest.
__device__ __forceinline__ bool boundary_hit(double x, double y, const Env& E) {
    const int last = SC_DRIFT_CENTER_SAMPLES - 1;
    const int i0 = (int)fmin(fmax(floor(x / E.cstep), 0.0), (double)last);
    const int lo = max(i0 - 1, 0), hi = min(i0 + 2, last);
    double best = INFINITY;
    for (int j = lo; j <= hi; ++j) {
        const double cx = j == last ? E.L : (double)j * E.cstep;
        const double dx = cx - x, dy = 0.0 - y;
        const double d = sqrt(dx * dx + dy * dy);
        if (d < best) best = d;
    }
    return best + E.R > E.hw;
}

// Gatekeeper._is_collision (gatekeeper.py:380-425) for a candidate state at time t: boundary, static circles with the plain
// radius (check_obstacle_collision, drifting_env.py:675-697), moving rectangles at t with radius + safety margin
// (_check_moving_obstacle_collision :434-466 on get_dynamic_obstacle_states(t) :660-673)
__device__ __forceinline__ bool state_hits(double x, double y, double t, const double* sob, int ns, const double* mob, int nm, const Env& E) {
    if (boundary_hit(x, y, E)) return true;
    for (int j = 0; j < ns; ++j) {
        const double dx = x - sob[3 * j], dy = y - sob[3 * j + 1];
        if (sqrt(dx * dx + dy * dy) < sob[3 * j + 2] + E.R) return true;
    }
    const double Rm = E.R + E.sm;
    for (int j = 0; j < nm; ++j) {
        const double* o = mob + 7 * j;
        const double ox = o[0] + o[2] * t, oy = o[1] + o[3] * t;
        const double cx = clip(x, ox - o[4] / 2, ox + o[4] / 2), cy = clip(y, oy - o[5] / 2, oy + o[5] / 2);
        const double dx = x - cx, dy = y - cy;
        if (sqrt(dx * dx + dy * dy) < Rm) return true;
    }
    return false;
}

// DriftingEnv.get_friction_at_position (drifting_env.py:466-484)
__device__ __forceinline__ double friction_at(double x, double y, const sc_drift_shield_params& p) {
    for (int j = 0; j < p.n_puddles; ++j) {
        const double dx = x - p.puddles[j][0], dy = y - p.puddles[j][1];
        if (sqrt(dx * dx + dy * dy) <= p.puddles[j][2]) return p.puddles[j][3];
    }
    return p.mu_default;
}

// DriftingCarSimulator.check_collision (drifting_car.py:676-711) after the step: check_collision_detailed's signed distance
// (= y on a straight track) against half_width - radius, then circles for the static and the (already stepped) moving obstacles
__device__ __forceinline__ bool sim_hit(double x, double y, const double* sob, int ns, const double* mob, int nm, const Env& E) {
    if (y > E.hw - E.R || y < -(E.hw - E.R)) return true;
    for (int j = 0; j < ns; ++j) {
        const double dx = x - sob[3 * j], dy = y - sob[3 * j + 1];
        if (sqrt(dx * dx + dy * dy) < sob[3 * j + 2] + E.R) return true;
    }
    for (int j = 0; j < nm; ++j) {
        const double dx = x - mob[7 * j], dy = y - mob[7 * j + 1];
        if (sqrt(dx * dx + dy * dy) < mob[7 * j + 6] + E.R) return true;
    }
    return false;
}

}  // namespace drift
}  // namespace sc
