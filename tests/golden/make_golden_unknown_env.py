"""Generates tests/golden/unknown_env.npz in the build container (needs the reference checkout, see _ref_import.py).

EXECUTES the reference's ``LocalTrackingController.control_step`` (tracking.py:559-668) in its examples/test_unknown_env.py
setting: ``robot_spec['sensor'] = 'rgbd'`` (which defines ``cam_range``, robots/robot.py:57-59), ``set_unknown_obs``, 'fov'
detection with and without the persistent memory, ``enable_rotation=True`` with the 'simple' and 'velocity_tracking_yaw' attitude
controllers for the integrators.  The QP is solved by make_golden.OracleProblem (cvxpy is not installed); under the import shim the
sensing-footprint polygons (update_sensing_footprints / is_beyond_sensing_footprints, shapely) are inert and return 0, which is the
part the library leaves out.

Per step the fixture holds the state after the step (X, yaw), the input applied so far (U), u_att (NaN for None), the state machine,
the return code, current_goal_index and the mask over the unknown table of the rows detect_unknown_obs passed on to the controller.
For every step and every unknown row the generator also computes the sighting margin (tests/_unknown_env_oracle.sighting) and asserts
that no rule of utils/detection.py:28-42 was decided by less than 1e-6: that makes an event-for-event comparison well posed.

The fixture holds arrays only."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden import DT, LocalTrackingController, OracleProblem, ref_env  # noqa: E402  (installs the import shim)
from _unknown_env_oracle import normalise_unknown, sighting_margins  # noqa: E402

SM = ["idle", "track", "stop", "rotate"]
KNOWN = np.array([[4.0, 3.5, 0.6, 0, 0, 0, 0]], dtype=np.float64)
WPS = np.array([[2, 2], [2, 12], [12, 12], [12, 2]], dtype=np.float64)
CIRCLES = [[2.5, 6, .4], [1.4, 9, .5], [7, 12.6, .5], [12.5, 8, .6], [6, 6, .5]]
WITH_SE = CIRCLES + [[9, 11.2, .3, .6, 2, .3, 1]]
DI = {"model": "DoubleIntegrator2D", "v_max": 1.0, "a_max": 1.0}
SCENES = [
    # tag, spec, attitude, x0, unknown rows, steps
    ("di_vty", DI, "velocity_tracking_yaw", [2.0, 2.0, 0.0, 0.0, 0.0], CIRCLES, 1200),
    ("si_simple", {"model": "SingleIntegrator2D", "v_max": 1.0}, "simple", [2.0, 2.0, -1.0], CIRCLES, 1200),
    ("du", {"model": "DynamicUnicycle2D", "w_max": 0.5, "a_max": 0.5}, None, [2.0, 2.0, 0.0], CIRCLES, 400),
    ("di_se", DI, "velocity_tracking_yaw", [2.0, 2.0, 0.0, 0.0, 0.0], WITH_SE, 1200),
    ("di_forget", dict(DI, unknown_obs_persistent_fov=False), "velocity_tracking_yaw", [2.0, 2.0, 0.0, 0.0, 0.0], WITH_SE, 1200),
]


def pad7(rows):
    return np.array([list(r) + [0.0] * (7 - len(r)) for r in rows], dtype=np.float64)


def run_scene(tag, spec, att, x0, unknown, steps, out, inert_safety_area=False):
    spec = dict(spec, radius=0.25, sensor="rgbd")
    ctype = {"pos": "cbf_qp"}
    if att is not None:
        ctype["att"] = att
    ctl = LocalTrackingController(np.array(x0, dtype=float), spec, controller_type=ctype, dt=DT, env=ref_env.Env(), enable_rotation=True)
    if spec["model"] == "DynamicUnicycle2D":
        hi = np.array([spec["a_max"], spec["w_max"]])
    elif spec["model"] == "SingleIntegrator2D":
        hi = np.array([spec["v_max"]] * 2)
    else:
        hi = np.array([spec["a_max"]] * 2)
    ctl.pos_controller.cbf_controller = OracleProblem(ctl.pos_controller, -hi, hi)
    ctl.obs = KNOWN.copy()
    table = pad7(unknown)
    ragged = len({len(r) for r in unknown}) > 1                    # the reference takes one rectangular array (tracking.py:278)
    ctl.set_unknown_obs(table if ragged else unknown)
    assert np.array_equal(ctl.unknown_obs, normalise_unknown(table if ragged else unknown)) and np.array_equal(ctl.unknown_obs, table)
    ctl.set_waypoints(WPS.copy())

    log = {"mask": 0, "margin": math.inf}
    inner = ctl.robot.detect_unknown_obs

    def detect(unknown_obs, *a, **k):
        """Records what the reference's detection passes on, and how far every row was from being decided otherwise."""
        hit, margin = sighting_margins(ctl.robot.get_position(), ctl.robot.get_orientation(), ctl.robot.fov_angle, ctl.robot.cam_range, table)
        log["margin"] = min(log["margin"], float(np.abs(margin).min()))
        rows = inner(unknown_obs, *a, **k)
        mask = 0
        for r in np.asarray(rows, dtype=float).reshape(-1, 7):
            j = [i for i in range(len(table)) if table[i, 0] == r[0] and table[i, 1] == r[1]]
            assert len(j) == 1
            mask |= 1 << j[0]
        now = sum(1 << int(i) for i in np.flatnonzero(hit))
        assert (mask & now) == now and (spec.get("unknown_obs_persistent_fov", True) or mask == now), "the margin rule disagrees with the reference"
        log["mask"] = mask
        return rows

    ctl.robot.detect_unknown_obs = detect
    if inert_safety_area:
        ctl.robot.update_safety_area = lambda: None
    sm0 = SM.index(ctl.state_machine)
    rec = {k: [] for k in ("X", "U", "yaw", "u_att", "sm", "ret", "idx", "mask")}
    for _ in range(steps):
        ret = ctl.control_step()
        u = ctl.get_control_input()
        rec["X"].append(ctl.robot.X.reshape(-1).copy())
        rec["U"].append(np.zeros(2) if u is None else np.asarray(u, dtype=float).reshape(-1).copy())
        rec["yaw"].append(float(ctl.robot.yaw))
        rec["u_att"].append(math.nan if ctl.u_att is None else float(np.asarray(ctl.u_att).reshape(-1)[0]))
        rec["sm"].append(SM.index(ctl.state_machine))
        rec["ret"].append(int(ret))
        rec["idx"].append(int(ctl.current_goal_index))
        rec["mask"].append(log["mask"])
        if ret != 0:
            break
    assert log["margin"] > 1e-6, f"{tag}: a sighting was decided by {log['margin']:.3e}: nudge the scene"
    out[f"{tag}/model"] = np.array(["DynamicUnicycle2D", "SingleIntegrator2D", "DoubleIntegrator2D"].index(spec["model"]))
    out[f"{tag}/att"] = np.array([None, "simple", "velocity_tracking_yaw"].index(att))
    out[f"{tag}/persistent"] = np.array(int(spec.get("unknown_obs_persistent_fov", True)))
    out[f"{tag}/x0"] = np.array(x0, dtype=np.float64)
    out[f"{tag}/obs"] = KNOWN
    out[f"{tag}/unknown"] = table
    out[f"{tag}/waypoints"] = WPS
    out[f"{tag}/sm0"] = np.array(sm0)
    out[f"{tag}/min_margin"] = np.array(log["margin"])
    for k in ("X", "U", "yaw", "u_att"):
        out[f"{tag}/{k}"] = np.array(rec[k], dtype=np.float64)
    for k in ("sm", "ret", "idx"):
        out[f"{tag}/{k}"] = np.array(rec[k], dtype=np.int64)
    out[f"{tag}/mask"] = np.array(rec["mask"], dtype=np.uint64)
    m = np.array(rec["mask"], dtype=np.uint64)
    sm = np.array(rec["sm"])
    print(f"{tag}: {len(rec['ret'])} steps, last ret {rec['ret'][-1]}, first state {SM[sm0]}, 'track' first after step "
          f"{int(np.argmax(sm == 1)) if (sm == 1).any() else -1}, mask changes at {[0] + [int(i) + 1 for i in np.flatnonzero(m[1:] != m[:-1])]}, "
          f"min |margin| {log['margin']:.2e}")


def gen():
    out = {}
    for scene in SCENES:
        run_scene(*scene, out)
    # DynamicUnicycle2D: update_safety_area (robots/robot.py:703-725, part of the sensing-footprint code the library leaves out) adds
    # the yaw increments of its braking arc to robot.yaw itself, so after a turning step get_orientation() is ahead of X[2] until the
    # next step() resets it.  The library looks along X[2].  Run the scene again with that method inert: every recorded array but yaw
    # must be the same, and the fixture keeps this run, whose yaw is X[2].
    alt = {}
    run_scene(*SCENES[2], alt, inert_safety_area=True)
    for k, v in alt.items():
        if k not in ("du/yaw", "du/min_margin"):
            assert np.array_equal(out[k], v, equal_nan=v.dtype.kind == "f"), k
    assert np.array_equal(alt["du/yaw"], alt["du/X"][:, 2])
    out.update(alt)
    np.savez_compressed(os.path.join(HERE, "unknown_env.npz"), **out)


if __name__ == "__main__":
    gen()
