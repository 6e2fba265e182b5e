// What the kernels of the sensing loop share (csrc/tracking_sense.hip, csrc/tracking_sense_split.hip): the attitude side's
// constants and the 'fov' detection test.
#pragma once
#include "sc_qp2.hpp"

namespace sc {

// what the attitude side of a step needs (sc_sense_params in f64)
struct SenseConsts {
    double half_fov, cam_range, w_max, att_kp, att_preview, simple_rate;
    int n_unknown, persistent, att_type;
};

__device__ __forceinline__ SenseConsts make_sense_consts(const sc_sense_params& sp) {
    SenseConsts s;
    s.half_fov = sp.fov_angle / 2; s.cam_range = sp.cam_range; s.w_max = sp.w_max; s.att_kp = sp.att_kp;
    s.att_preview = sp.att_preview_time; s.simple_rate = sp.simple_yaw_rate;
    s.n_unknown = sp.n_unknown; s.persistent = sp.persistent; s.att_type = sp.att_type;
    return s;
}

// utils/detection.py:28-42 (_circle_intersects_fov): does the camera cone of half angle half_fov and range cam_range, at
// (x, y) looking along yaw, touch the circle (cx, cy, r)?
__device__ __forceinline__ bool circle_in_fov(const double x, const double y, const double yaw, const double cx, const double cy,
                                              const double r, const SenseConsts& s) {
    const double dx = cx - x, dy = cy - y;
    const double d = sqrt_(dx * dx + dy * dy);
    if (d <= r) return true;
    if (d - r > s.cam_range) return false;
    const double ad = fabs_(angle_normalize(atan2_(dy, dx) - yaw));
    if (ad <= s.half_fov) return true;
    const double ar = asin(fmin_(fmax_(r / fmax_(d, 1e-9), 0.0), 1.0));          // only the lanes that got here
    return ad <= s.half_fov + ar;
}

}  // namespace sc
