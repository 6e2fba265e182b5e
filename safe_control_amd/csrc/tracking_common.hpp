// Per-model pieces of the closed loop that the rollout kernels share (csrc/tracking.hip, csrc/tracking_sense.hip):
// nominal input, stop(), has_stopped(), the robot step and the known-obstacle collision test.
#pragma once
#include "sc_qp2.hpp"

namespace sc {

template <typename T>
struct TrackConsts {
    T reached, rot_thr, v_max, v_min, k_omega, k_a, k_v, delta_max, wheel_base, Lr, dt, a_max;
    int enable_rotation, dyn_obs, K;
};

// nominal_input: DU robots/dynamic_unicycle2D.py:80-104 ; KB robots/kinematic_bicycle2D.py:125-147
// (gains as BaseRobot forwards them, robots/robot.py:401-408)
template <typename T, int MODEL>
__device__ __forceinline__ void nominal_input(const T x, const T y, const T th, const T v, const T gx, const T gy,
                                              const TrackConsts<T>& t, T& u0, T& u1) {
    if constexpr (MODEL == SC_MODEL_SINGLE_INTEGRATOR2D || MODEL == SC_MODEL_DOUBLE_INTEGRATOR2D) {
        // single_integrator2D.py:72-90 / double_integrator2D.py:113-140 (th, v carry vx, vy for the double integrator):
        // dead-banded position error -> desired velocity, saturated in norm; DI: acceleration towards it, saturated in norm
        const T ex = gx - x, ey = gy - y;
        T vx = t.k_v * copysign(fmax_(fabs_(ex) - T(0.05), T(0)), ex), vy = t.k_v * copysign(fmax_(fabs_(ey) - T(0.05), T(0)), ey);
        const T vm = sqrt_(vx * vx + vy * vy);
        if (vm > t.v_max) { vx = vx * t.v_max / vm; vy = vy * t.v_max / vm; }
        if constexpr (MODEL == SC_MODEL_SINGLE_INTEGRATOR2D) { u0 = vx; u1 = vy; }
        else {
            T ax = t.k_a * (vx - th), ay = t.k_a * (vy - v);
            const T am = sqrt_(ax * ax + ay * ay);
            if (am > t.a_max) { ax = ax * t.a_max / am; ay = ay * t.a_max / am; }
            u0 = ax; u1 = ay;
        }
        return;
    }
    const T pi = T(3.14159265358979323846);
    const T dx = x - gx, dy = y - gy;
    const T dist = sqrt_(dx * dx + dy * dy);
    const T err = angle_normalize(atan2_(gy - y, gx - x) - th);
    T sn, cs;
    sincos_(err, &sn, &cs);
    if constexpr (MODEL == SC_MODEL_DYNAMIC_UNICYCLE2D) {
        const T d = fmax_(dist - T(0.05), T(0));
        const T vd = (fabs_(err) > pi / T(2)) ? T(0) : fmin_(t.k_v * d * cs, t.v_max);
        u0 = t.k_a * (vd - v);
        u1 = t.k_omega * err;
    } else if constexpr (MODEL == SC_MODEL_UNICYCLE2D) {
        // robots/unicycle2D.py:69-85 with the gains BaseRobot forwards (robots/robot.py:404-405): d_min .05,
        // k_omega 2, k_v 1; the speed command is not clipped
        const T d = fmax_(dist - T(0.05), T(0.05));
        u0 = (fabs_(err) > pi / T(2)) ? T(0) : T(1) * d * cs;
        u1 = T(2) * err;
    } else {
        const T d = fmax_(dist - T(0.05), T(0.05));
        const T delta = fmin_(fmax_(t.k_omega * err, -t.delta_max), t.delta_max);
        u1 = atan(double((t.Lr / t.wheel_base) * tan(double(delta))));
        const T vcmd = t.k_v * d * fmax_(T(0), cs);
        const T vd = fmin_(fmax_(vcmd, t.v_min), t.v_max);
        u0 = t.k_a * (vd - v);
    }
}

// stop(): DU brakes with k_a (dynamic_unicycle2D.py:106-111); KB and Unicycle2D return zeros (kinematic_bicycle2D.py:149-150,
// unicycle2D.py:87-88)
// SingleIntegrator2D: zeros (single_integrator2D.py:100-103); DoubleIntegrator2D brakes both components
// (double_integrator2D.py:149-156; th, v carry vx, vy)
template <typename T, int MODEL>
__device__ __forceinline__ void stop_input(const T th, const T v, const T k_a, T& u0, T& u1) {
    if constexpr (MODEL == SC_MODEL_DOUBLE_INTEGRATOR2D) { u0 = k_a * (T(0) - th); u1 = k_a * (T(0) - v); }
    else { u0 = (MODEL == SC_MODEL_DYNAMIC_UNICYCLE2D) ? k_a * (T(0) - v) : T(0); u1 = T(0); }
}
// has_stopped(): |v| < .05 (DU :113-114, KB :152-153); the kinematic unicycle always has (unicycle2D.py:90-92)
template <typename T, int MODEL>
__device__ __forceinline__ bool has_stopped(const T th, const T v) {
    if constexpr (MODEL == SC_MODEL_UNICYCLE2D || MODEL == SC_MODEL_SINGLE_INTEGRATOR2D) return true;
    else if constexpr (MODEL == SC_MODEL_DOUBLE_INTEGRATOR2D) return sqrt_(th * th + v * v) < T(0.05);   // |(vx, vy)|
    else return fabs_(v) < T(0.05);
}
// step(): X + (f + g u) dt, heading wrapped (DU :75-78 ; KB :113-123, speed clipped ; Unicycle2D unicycle2D.py:64-67,
// whose 4th state column is padding and stays as it is)
template <typename T, int MODEL>
__device__ __forceinline__ void robot_step(const Agent<T>& a, const T u0, const T u1, const T dt, const T Lr, const T v_min,
                                           const T v_max, T& nx, T& ny, T& nth, T& nv) {
    if constexpr (MODEL == SC_MODEL_SINGLE_INTEGRATOR2D) {               // single_integrator2D.py:64-66; columns 2, 3 are padding
        nx = a.x + (T(0) + u0) * dt; ny = a.y + (T(0) + u1) * dt; nth = a.th; nv = a.v;
        return;
    } else if constexpr (MODEL == SC_MODEL_DOUBLE_INTEGRATOR2D) {        // double_integrator2D.py:79-107: speed rescaled to v_max
        nx = a.x + (a.f0 + T(0)) * dt; ny = a.y + (a.f1 + T(0)) * dt;
        nth = a.f0 + (T(0) + u0) * dt; nv = a.f1 + (T(0) + u1) * dt;
        const T vm = sqrt_(nth * nth + nv * nv);
        if (vm > v_max) { const T sc = v_max / vm; nth *= sc; nv *= sc; }
        return;
    } else if constexpr (MODEL == SC_MODEL_DYNAMIC_UNICYCLE2D) {
        nx = a.x + (a.f0) * dt; ny = a.y + (a.f1) * dt;
        nth = a.th + (T(0) + u1) * dt; nv = a.v + (T(0) + u0) * dt;
    } else if constexpr (MODEL == SC_MODEL_UNICYCLE2D) {
        nx = a.x + (T(0) + a.c * u0) * dt; ny = a.y + (T(0) + a.s * u0) * dt;
        nth = a.th + (T(0) + u1) * dt; nv = a.v;
    } else {
        nx = a.x + (a.f0 + (-a.f1) * u1) * dt;
        ny = a.y + (a.f1 + a.f0 * u1) * dt;
        nth = a.th + (T(0) + (a.v / Lr) * u1) * dt;
        nv = a.v + (T(0) + u0) * dt;
        nv = fmin_(fmax_(nv, v_min), v_max);                              // np.clip in KinematicBicycle2D.step
    }
    nth = angle_normalize(nth);
}

// tracking.py:445-495 known-obstacle collision test (circle / superellipsoid, geometry rule :428-443)
template <typename T>
__device__ __forceinline__ bool collides(const T x, const T y, const T* table, int M, T R) {
    bool hit = false;
    for (int m = 0; m < M; ++m) {
        const T* o = table + 7 * m;
        const bool superell = (fabs_(o[6] - T(1)) <= T(1e-8) + T(1e-5)) && (o[4] >= T(2));     // np.isclose(flag, 1)
        if (!superell) {
            const T dx = x - o[0], dy = y - o[1];
            hit |= sqrt_(dx * dx + dy * dy) < o[2] + R;
        } else {
            T st, ct;
            sincos_(o[5], &st, &ct);
            const T px = ct * (x - o[0]) + st * (y - o[1]);
            const T py = -st * (x - o[0]) + ct * (y - o[1]);
            const T h = pow_(px / (o[2] + R), o[4]) + pow_(py / (o[3] + R), o[4]) - T(1);
            hit |= h <= T(0);
        }
    }
    return hit;
}

}  // namespace sc
