// The evade scenario of the reference on the device (examples/evade/test_evade.py): DoubleIntegrator2D.step, the example's
// nominal controller, EvadeBackupController and the EvadeEnv collision tests.  Written operation for operation like the
// reference's scalar numpy code; a translation unit that includes this header is compiled WITHOUT floating-point
// contraction (the pragma below holds to its end), so a decision taken on these values agrees with the CPU to the bit.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/safe_control_amd.h"

#pragma clang fp contract(off)

namespace sc {
namespace evade {

struct Env {                      // constants of one launch
    double dt, R, amax, vmax, sm, kp, kd;
    double L, hw, pxmin, pxmax, pymin, pymax, gxmin, gxmax, bspeed, blen, bwid, bstart, cx, cy;
};

__device__ __forceinline__ Env make_env(const sc_backupcbf_params& p) {
    Env E;
    E.dt = p.dt; E.R = p.robot_radius; E.amax = p.a_max; E.vmax = p.v_max; E.sm = p.safety_margin; E.kp = p.backup_kp; E.kd = p.backup_kd;
    E.L = p.hallway_length; E.hw = p.half_width; E.pxmin = p.pocket_x_min; E.pxmax = p.pocket_x_max;
    E.pymin = p.pocket_y_min; E.pymax = p.pocket_y_max; E.gxmin = p.goal_x_min; E.gxmax = p.goal_x_max;
    E.bspeed = p.bullet_speed; E.blen = p.bullet_length; E.bwid = p.bullet_width; E.bstart = p.bullet_start_x;
    E.cx = (p.pocket_x_min + p.pocket_x_max) / 2; E.cy = (p.pocket_y_min + p.pocket_y_max) / 2;   // evade_env.py:70-73
    return E;
}

// _clamp_control (backup_controller.py:551-557) / the example's nominal clamp (test_evade.py:160-164)
__device__ __forceinline__ void clamp(double& ax, double& ay, double amax) {
    const double am = sqrt(ax * ax + ay * ay);
    if (am > amax) { ax = ax * amax / am; ay = ay * amax / am; }
}

// EvadeNominalController.compute_control (examples/evade/test_evade.py:141-166)
__device__ __forceinline__ void nominal(const double* x, const Env& E, double& ax, double& ay) {
    ax = 2.0 * (E.vmax - x[2]);
    ay = 2.0 * (0.0 - x[1]) + 2.0 * (0.0 - x[3]);
    clamp(ax, ay, E.amax);
}

// EvadeBackupController.compute_control (backup_controller.py:456-549)
__device__ __forceinline__ void backup(const double* x, const Env& E, double& ax, double& ay) {
    const double px = x[0], py = x[1], vx = x[2], vy = x[3];
    const double margin = E.R + 0.1;
    const double ddx = px - E.cx, ddy = py - E.cy;
    const double dist = sqrt(ddx * ddx + ddy * ddy);
    const bool in_goal = E.gxmin <= px && px <= E.gxmax && -E.hw <= py && py <= E.hw;
    const bool x_safe = E.pxmin + margin <= px && px <= E.pxmax - margin;
    const bool deep = x_safe && E.pymin + margin <= py && py <= E.pymax - margin && dist < 1.0;
    if (in_goal || deep) {
        ax = -E.kd * vx; ay = -E.kd * vy;
    } else if (E.pxmin - 2.0 <= px && px <= E.pxmax + 2.0) {
        const double ty = x_safe ? E.cy : (py > E.pymin ? fmax(py, 3.0) : 0.0);
        ax = E.kp * (E.cx - px) - E.kd * vx;
        ay = E.kp * (ty - py) - E.kd * vy;
    } else {
        const double ty = (py > E.pymin && px > E.pxmax) ? fmax(py, 3.0) : 0.0;
        const double ex = E.cx - px, ey = ty - py;
        const double sg = ex > 0.0 ? 1.0 : (ex < 0.0 ? -1.0 : 0.0);
        ax = E.kp * sg * fmin(fabs(ex), 3.0) - E.kd * vx;
        ay = E.kp * ey - E.kd * vy;
    }
    clamp(ax, ay, E.amax);
}

// DoubleIntegrator2D.step (double_integrator2D.py:79-107): Euler, then the speed rescaled to v_max
__device__ __forceinline__ void step(const double* x, double ax, double ay, const Env& E, double* xn) {
    xn[0] = x[0] + x[2] * E.dt; xn[1] = x[1] + x[3] * E.dt;
    xn[2] = x[2] + ax * E.dt; xn[3] = x[3] + ay * E.dt;
    const double vm = sqrt(xn[2] * xn[2] + xn[3] * xn[3]);
    if (vm > E.vmax) { const double s = E.vmax / vm; xn[2] *= s; xn[3] *= s; }
}

// x <- step(x, backup(x)): one step of Gatekeeper._forward_simulate_backup (gatekeeper.py:265-299)
__device__ __forceinline__ void backup_step(double* x, const Env& E, double& ax, double& ay) {
    backup(x, E, ax, ay);
    double xn[4];
    step(x, ax, ay, E, xn);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = xn[j];
}

// EvadeEnv.check_collision (envs/evade_env.py:408-452): hallway walls and the pocket
__device__ __forceinline__ bool walls_hit(double x, double y, const Env& E) {
    const double r = E.R;
    if (y - r < -E.hw) return true;
    if (y + r > E.hw) {
        if (E.pxmin <= x && x <= E.pxmax) {
            if (y + r > E.pymax) return true;
            if (x - r < E.pxmin && y > E.hw) return true;
            if (x + r > E.pxmax && y > E.hw) return true;
        } else {
            return true;
        }
    }
    if (x - r < 0) return true;
    return x + r > E.L;
}

// distance from (x, y) to the box [x0, x1] x [y0, y1] the way np.clip + np.sqrt compute it
__device__ __forceinline__ double box_dist(double x, double y, double x0, double x1, double y0, double y1) {
    const double cx = fmin(fmax(x, x0), x1), cy = fmin(fmax(y, y0), y1);
    const double dx = x - cx, dy = y - cy;
    return sqrt(dx * dx + dy * dy);
}

// EvadeEnv.check_obstacle_collision (evade_env.py:454-485): the bullet where it is now, nose included
__device__ __forceinline__ bool bullet_hit_now(double x, double y, double bx, const Env& E) {
    return box_dist(x, y, bx - E.blen / 2, bx + E.blen / 2 + E.blen / 3, 0.0 - E.bwid / 2, 0.0 + E.bwid / 2) < E.R;
}

// Gatekeeper._check_moving_obstacle_collision (gatekeeper.py:434-466) against get_obstacles(t) (test_evade.py:373-384,
// evade_env.py:386-406): centre bullet_x + L / 6 moving at vx, length 4 L / 3, robot radius + safety margin
__device__ __forceinline__ bool bullet_hit_pred(double x, double y, double bx, double t, const Env& E) {
    const double ox = (bx + E.blen / 6) + E.bspeed * t;
    const double ol = E.blen * (1 + 1.0 / 3);
    return box_dist(x, y, ox - ol / 2, ox + ol / 2, 0.0 - E.bwid / 2, 0.0 + E.bwid / 2) < E.R + E.sm;
}

// Gatekeeper._is_collision (gatekeeper.py:380-425) for candidate state k at t = k * dt
__device__ __forceinline__ bool state_hits(double x, double y, double t, double bx, bool predict, const Env& E) {
    if (walls_hit(x, y, E) || bullet_hit_now(x, y, bx, E)) return true;
    return predict && bullet_hit_pred(x, y, bx, t, E);
}

}  // namespace evade
}  // namespace sc
