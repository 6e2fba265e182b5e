"""Float64 restatement of LocalTrackingController.control_step with unknown obstacles and a heading of its own.

TEST INFRASTRUCTURE ONLY.  Extends oracle.tracking.TrackingOracle (which leaves sensing and the attitude controllers
out) with the pieces csrc/tracking_sense.hip runs on the device:

    'fov' detection              utils/detection.py:28-87, called at tracking.py:580
    the memory of sighted rows   robots/robot.py:773-834 (persistent) or the instantaneous set (:828-834)
    the combined candidate list  tracking.py:359-366 (known rows, then the rows passed on)
    is_collide_unknown           tracking.py:445-460 (every unknown row, seen or not)
    yaw / u_att                  robots/robot.py:441-448 (step_rotate), tracking.py:506-521, :589-594, :620-624
    SimpleAtt                    attitude_control/simple_attitude.py
    VelocityTrackingYaw          attitude_control/velocity_tracking_yaw.py:35-64

The memory keeps first-sighting order like the reference; that order only matters when two centre distances are exactly equal.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                             # the fleet workers below run this file as a script
    sys.path.insert(0, ROOT)

from oracle import cbf_qp, robots as R  # noqa: E402
from oracle.qp import STATUS_OPTIMAL  # noqa: E402
from oracle.tracking import TrackingOracle, get_nearest_unpassed_obs, is_collide  # noqa: E402

SM_INDEX = {"idle": 0, "track": 1, "stop": 2, "rotate": 3}


def seen_circle(row):
    """detection.py:62-69: the zero-padded row; a superellipsoid (flag >= 0.5) is seen as its outer circle."""
    p = np.zeros(7)
    p[: min(len(row), 7)] = np.asarray(row, dtype=np.float64)[:7]
    if p[6] >= 0.5:
        p[2] = max(p[2], p[3], 0.0)
        p[3:6] = 0.0
        p[6] = 0.0
    return p


def sighting(pos, yaw, fov_angle, cam_range, center, radius):
    """detection.py:28-42 (_circle_intersects_fov).  Returns (sighted, margin): margin is the smallest |slack| of the rules that
    were evaluated on the way to the decision, signed by the decision (positive: sighted)."""
    dx, dy = center[0] - pos[0], center[1] - pos[1]
    dist = math.sqrt(dx * dx + dy * dy)
    slack = [radius - dist]
    if dist <= radius:
        return True, abs(slack[0])
    slack.append(cam_range - (dist - radius))
    if dist - radius > cam_range:
        return False, -min(abs(s) for s in slack)
    ad = abs(R.angle_normalize(math.atan2(dy, dx) - yaw))
    slack.append(fov_angle / 2 - ad)
    if ad <= fov_angle / 2:
        return True, min(abs(s) for s in slack)
    ar = math.asin(min(max(radius / max(dist, 1e-9), 0.0), 1.0))
    slack.append(fov_angle / 2 + ar - ad)
    hit = ad <= fov_angle / 2 + ar
    m = min(abs(s) for s in slack)
    return hit, (m if hit else -m)


def sighting_margins(pos, yaw, fov_angle, cam_range, unknown):
    """One (sighted, margin) pair per unknown row."""
    circles = [seen_circle(o) for o in unknown]
    out = [sighting(pos, yaw, fov_angle, cam_range, c[:2], c[2]) for c in circles]
    return np.array([h for h, _ in out], dtype=bool), np.array([m for _, m in out], dtype=np.float64)


def normalise_unknown(rows):
    """tracking.py:277-291."""
    u = np.array([] if rows is None else rows, dtype=np.float64)
    if u.ndim == 1 and u.size > 0:
        u = u.reshape(1, -1)
    if u.size == 0:
        return np.empty((0, 7))
    if u.shape[1] < 7:
        u = np.hstack((u, np.zeros((u.shape[0], 7 - u.shape[1]))))
    return u[:, :7].copy()


class UnknownEnvOracle(TrackingOracle):
    """Single-agent closed loop with FOV sensing of unknown obstacles and (integrators) yaw control."""

    def __init__(self, model, X0, spec, dt=0.05, obs=None, unknown_obs=None, num_constraints=10, enable_rotation=True,
                 att="velocity_tracking_yaw", yaw0=None, cbf_param=None):
        integrator = model in (R.MODEL_SI, R.MODEL_DI)
        super().__init__(model, X0, spec, dt=dt, obs=obs, num_constraints=num_constraints,
                         enable_rotation=(enable_rotation and not integrator), cbf_param=cbf_param, yaw0=yaw0)
        self.enable_rotation = enable_rotation
        if self.obs.ndim == 2 and self.obs.shape[0] and self.obs.shape[1] < 7:
            self.obs = np.hstack((self.obs, np.zeros((self.obs.shape[0], 7 - self.obs.shape[1]))))
        self.att = att if (integrator and enable_rotation) else None               # tracking.py:156-181
        if self.att not in (None, "simple", "velocity_tracking_yaw"):
            raise ValueError(f"attitude controller {att!r}")
        self.u_att = None                                                           # tracking.py:102
        s = self.spec
        self.cam_range = float(s.get("cam_range", 3.0))                             # robots/robot.py:57-59
        self.w_max = float(s.get("w_max", 0.5))
        self.persistent = bool(s.get("unknown_obs_persistent_fov", True))
        self.simple_yaw_rate = float(s.get("simple_yaw_rate", self.w_max))
        self.att_kp = float(s.get("velocity_tracking_yaw_kp", 1.5))
        self.att_preview = float(s.get("velocity_tracking_yaw_preview_time", 0.0))
        self.set_unknown_obs(unknown_obs)
        self.min_margin = math.inf

    # -- unknown obstacles ------------------------------------------------------------------------
    def set_unknown_obs(self, rows):
        self.unknown_obs = normalise_unknown(rows)
        self.unknown_seen = np.array([seen_circle(o) for o in self.unknown_obs]).reshape(-1, 7)   # what a sighted row is taken for
        self.memory = []                        # indices into unknown_obs, in first-sighting order (robots/robot.py:773-797)
        self.passed_on = []                     # the rows the controller got in the last step

    def heading(self):
        return self.yaw if self.integrator else self.X[2]                          # robot.get_orientation()

    def seen_mask(self):
        return sum(1 << j for j in self.passed_on)

    def detect(self):
        """robots/robot.py:799-834 in 'fov' mode: the circles handed to the controller, as (indices, rows)."""
        pos, yaw = (float(self.X[0]), float(self.X[1])), float(self.heading())
        res = [sighting(pos, yaw, self.fov_angle, self.cam_range, (c[0], c[1]), c[2]) for c in self.unknown_seen.tolist()]
        hit = [h for h, _ in res]
        if res:
            self.min_margin = min(self.min_margin, min(abs(m) for _, m in res))
        d = np.linalg.norm(self.unknown_obs[:, :2] - self.X[:2], axis=1) if len(self.unknown_obs) else np.zeros(0)
        now = [int(j) for j in np.argsort(d, kind="stable") if hit[j]]              # detection.py:52-54: sorted by distance
        if self.persistent:
            for j in now:
                if j not in self.memory:
                    self.memory.append(j)
            self.passed_on = list(self.memory)
        else:
            self.passed_on = now
        return [self.unknown_seen[j] for j in self.passed_on]

    def collides(self):
        """tracking.py:445-495: unknown rows as circles of their own radius, then the known table."""
        u = self.unknown_obs
        if len(u) and (np.sqrt((self.X[0] - u[:, 0]) ** 2 + (self.X[1] - u[:, 1]) ** 2) < u[:, 2] + self.spec["radius"]).any():
            return True
        return is_collide(self.X, self.obs, self.spec["radius"])

    # -- goal ----------------------------------------------------------------------------------------
    def update_goal(self):
        """tracking.py:497-535 with the heading the robot reports (yaw for the integrators) and u_att dropped on leaving 'rotate'."""
        if self.state_machine == "rotate":
            rg = self.waypoints[self.current_goal_index]
            goal_angle = math.atan2(rg[1] - self.X[1], rg[0] - self.X[0])
            if not self.enable_rotation:
                self.state_machine = "track"
            if abs(self.heading() - goal_angle) > self.rotation_threshold:
                return rg[:2]
            self.state_machine = "track"
            self.u_att = None
        if self.current_goal_index >= len(self.waypoints):
            return None
        wp = self.waypoints[self.current_goal_index]
        if np.linalg.norm(self.X[:2] - wp[:2]) < self.reached_threshold:
            self.current_goal_index += 1
            if self.current_goal_index >= len(self.waypoints):
                self.state_machine = "idle"
                return None
        return np.array(self.waypoints[self.current_goal_index][0:2])

    # -- attitude ----------------------------------------------------------------------------------
    def attitude(self, u):
        if self.att == "simple":                                                    # simple_attitude.py
            return self.simple_yaw_rate
        if self.model == R.MODEL_SI:                                                # velocity_tracking_yaw.py:35-64
            vx, vy = u[0], u[1]
        else:
            vx, vy = self.X[2], self.X[3]
            if self.att_preview > 0.0:
                vx, vy = vx + self.att_preview * u[0], vy + self.att_preview * u[1]
        if math.hypot(vx, vy) < 1e-2:
            return 0.0
        err = R.angle_normalize(math.atan2(vy, vx) - self.yaw)
        return float(np.clip(self.att_kp * err, -self.w_max, self.w_max))

    # -- one control step ------------------------------------------------------------------------
    def control_step(self):
        """tracking.py:559-668 (return code 1, the sensing footprint's, is not produced)."""
        m = self.model
        if self.state_machine == "stop":                                            # :569-577
            if R.has_stopped(m, self.X):
                self.state_machine = "rotate" if self.enable_rotation else "track"
                self.goal = self.update_goal()
        else:
            self.goal = self.update_goal()

        detected = self.detect()                                                    # :580
        all_obs = np.vstack([self.obs.reshape(-1, 7)] + [np.array(detected).reshape(-1, 7)])   # :359-366
        self.nearest_multi_obs = get_nearest_unpassed_obs(m, all_obs, self.X[:2], self.heading(), self.num_constraints)

        if self.state_machine == "rotate":                                          # :589-596
            ga = math.atan2(self.goal[1] - self.X[1], self.goal[0] - self.X[0])
            if self.integrator:                                                     # *_integrator2D.py rotate_to: k_omega 2, clipped
                self.u_att = float(np.clip(2.0 * R.angle_normalize(ga - self.yaw), -self.w_max, self.w_max))
                u_ref = R.stop(m, self.X, self.spec)
            else:
                u_ref = R.rotate_to(m, self.X, ga)
        elif self.goal is None:
            u_ref = R.stop(m, self.X, self.spec)
        else:
            u_ref = R.nominal_input(m, self.X, self.goal, self.spec)

        obs_list = None if self.nearest_multi_obs is None else list(self.nearest_multi_obs)
        r = cbf_qp.solve(m, self.X, u_ref, obs_list, self.spec, self.cbf_param, num_obs=self.num_constraints, dt=self.dt)
        u, self.status = r["u"], r["status"]

        if self.state_machine == "track" and self.att is not None and u is not None:   # :620-624
            self.u_att = self.attitude(np.asarray(u, dtype=np.float64).reshape(-1))

        if self.status != STATUS_OPTIMAL or self.collides():                        # :627-634
            return -2
        self.X = R.step(m, self.X, u, self.dt, self.spec)                           # :637, robots/robot.py:441-448
        if self.integrator and self.u_att is not None:
            self.yaw = R.angle_normalize(self.yaw + self.u_att * self.dt)
        self.u_pos = np.asarray(u, dtype=np.float64).reshape(-1)
        if self.collides():                                                         # :640-646
            return -2
        if self.goal is None and self.state_machine != "stop":                      # :666-667
            return -1
        return 0


def run(oracle, n_steps):
    """Run up to n_steps steps; per-step records in the layout of tests/golden/unknown_env.npz (state AFTER each step)."""
    rec = {k: [] for k in ("X", "U", "yaw", "u_att", "sm", "ret", "idx", "mask")}
    for _ in range(n_steps):
        ret = oracle.control_step()
        rec["X"].append(oracle.X.copy())
        rec["U"].append(np.zeros(2) if oracle.u_pos is None else oracle.u_pos.copy())
        rec["yaw"].append(oracle.heading())
        rec["u_att"].append(math.nan if oracle.u_att is None else oracle.u_att)
        rec["sm"].append(SM_INDEX[oracle.state_machine])
        rec["ret"].append(ret)
        rec["idx"].append(oracle.current_goal_index)
        rec["mask"].append(oracle.seen_mask())
        if ret != 0:
            break
    out = {k: np.array(v, dtype=np.float64) for k, v in rec.items() if k in ("X", "U", "yaw", "u_att")}
    out.update({k: np.array(rec[k], dtype=np.int64) for k in ("sm", "ret", "idx")})
    out["mask"] = np.array(rec["mask"], dtype=np.uint64)
    return out


# ---- cases the CPU and the GPU tests share ---------------------------------------------------------------------------------
MODELS = (R.MODEL_DU, R.MODEL_SI, R.MODEL_DI)                      # the fixture's `model` index
MODEL_NAMES = ("DynamicUnicycle2D", "SingleIntegrator2D", "DoubleIntegrator2D")
ATTS = (None, "simple", "velocity_tracking_yaw")                   # the fixture's `att` index
FIXTURE_TAGS = ("di_vty", "si_simple", "du", "di_se", "di_forget")


def fixture_spec(z, tag):
    """The robot_spec of a scene of tests/golden/unknown_env.npz (make_golden_unknown_env.py: SCENES) without its model name."""
    model = int(z[f"{tag}/model"])
    spec = {"radius": 0.25, "v_max": 1.0}
    if model == 0:
        spec.update(w_max=0.5, a_max=0.5)
    elif model == 2:
        spec.update(a_max=1.0)
    if not int(z[f"{tag}/persistent"]):
        spec["unknown_obs_persistent_fov"] = False
    return spec


def state_and_yaw(model_index, x0):
    """tracking.py:60-76: X0 = [x, y, (vx, vy,) yaw] for the integrators -> the four state columns and the heading."""
    x0 = np.asarray(x0, dtype=np.float64)
    if model_index == 1:
        return np.array([x0[0], x0[1], 0.0, 0.0]), float(x0[2])
    if model_index == 2:
        return x0[:4].copy(), float(x0[4])
    return np.array([x0[0], x0[1], x0[2], 0.0]), float(x0[2])


def oracle_from_fixture(z, tag):
    mi = int(z[f"{tag}/model"])
    X, yaw = state_and_yaw(mi, z[f"{tag}/x0"])
    o = UnknownEnvOracle(MODELS[mi], X, fixture_spec(z, tag), obs=z[f"{tag}/obs"], unknown_obs=z[f"{tag}/unknown"],
                         att=ATTS[int(z[f"{tag}/att"])] or "velocity_tracking_yaw", yaw0=yaw)
    o.set_waypoints(z[f"{tag}/waypoints"])
    return o


# ---- every kernel the sensing launchers can pick (the fused loop and the select / apply pair) -------------------------------------
RUNG_UNKNOWN = np.array([[5.0, 5.0, 0.3125, 0, 0, 0, 0], [8.0, 9.0, 0.25, 0, 0, 0, 0], [2.5, 7.5, 0.375, 0, 0, 0, 0],
                         [10.5, 6.5, 0.3125, 0, 0, 0, 0], [6.5, 11.5, 0.25, 0, 0, 0, 0]])     # f32 numbers


def rung_records(case, T, num_constraints, make=None):
    """One oracle per agent of a tests/_agent_params_cases.py rung_case (every agent the first agent's spec) with RUNG_UNKNOWN as its
    unknown rows: the run() record of each, with `min_margin`.  ``make(*args, **kwargs)`` builds the oracle (default: UnknownEnvOracle)."""
    import _agent_params_cases as AC
    m, ospec, cp = AC.oracle_args(case["specs"][0])
    out = []
    for x0 in case["X0"]:
        integ = m in (R.MODEL_SI, R.MODEL_DI)
        nst = 2 if m == R.MODEL_SI else 4
        xs = np.concatenate([x0[:nst], np.zeros(4 - nst)]) if integ else x0
        o = (make or UnknownEnvOracle)(m, xs, ospec, dt=AC.DT, obs=case["obs"], unknown_obs=RUNG_UNKNOWN, num_constraints=num_constraints,
                                       yaw0=x0[nst] if integ else None, cbf_param=cp)
        o.set_waypoints(case["wl"][len(out)])
        r = run(o, T)
        r["min_margin"] = np.array(o.min_margin)
        out.append(r)
    return out


def assert_records(ref, tX, tU, tY, tS, ret, rstep, sm, tol):
    """What test_batch_against_the_oracle asserts of every agent, at rtol = atol = tol; no agent's sighting may be decided by less."""
    for i, r in enumerate(ref):
        assert float(r["min_margin"]) >= tol, f"agent {i}: a sighting decided by less than the comparison's tolerance"
        n = len(r["ret"])
        np.testing.assert_allclose(tX[:n, i], r["X"], rtol=tol, atol=tol, err_msg=f"agent {i}")
        np.testing.assert_allclose(tU[:n, i], r["U"], rtol=tol, atol=tol, err_msg=f"agent {i}")
        np.testing.assert_allclose(tY[:n, i], r["yaw"], rtol=tol, atol=tol, err_msg=f"agent {i}")
        assert np.array_equal(tS[:n, i], r["mask"]), f"agent {i}: sighted rows"
        last = int(r["ret"][-1])
        assert ret[i] == last and rstep[i] == (n - 1 if last != 0 else -1) and sm[i] == r["sm"][-1], f"agent {i}"


FLEET_B, FLEET_STEPS, FLEET_MU, FLEET_M = 130, 300, 33, 12
FLEET_SPEC = {"radius": 0.25, "v_max": 1.0, "a_max": 1.0}
FLEET_WPS = np.array([[2.0, 2.0], [2.0, 12.0], [12.0, 12.0], [12.0, 2.0]])


def fleet_scene(seed=2024):
    """130 DoubleIntegrator2D agents (two full blocks and a two-lane tail) with perturbed starts and headings around the
    fixtures' first waypoint, 12 known circles and 33 unknown circles (bits on both sides of the mask's 32-bit half) scattered along
    the first leg of the route, none closer than 1.2 m to the start area's centre and no two overlapping."""
    rng = np.random.default_rng(seed)
    rows = []
    while len(rows) < FLEET_M + FLEET_MU:
        c = np.array([rng.uniform(-0.5, 5.5), rng.uniform(2.0, 13.5)])
        r = rng.uniform(0.12, 0.3)
        if np.linalg.norm(c - [2.0, 2.0]) < 1.6 + r:
            continue
        if any(np.linalg.norm(c - q[:2]) < r + q[2] + 0.2 for q in rows):
            continue
        rows.append(np.array([c[0], c[1], r, 0, 0, 0, 0]))
    rows = np.array(rows)
    order = rng.permutation(len(rows))
    known, unknown = rows[order[:FLEET_M]], rows[order[FLEET_M:]]
    X0 = np.zeros((FLEET_B, 5))
    X0[:, 0:2] = 2.0 + rng.uniform(-0.4, 0.4, (FLEET_B, 2))
    X0[:, 2:4] = rng.uniform(-0.2, 0.2, (FLEET_B, 2))
    X0[:, 4] = rng.uniform(-np.pi, np.pi, FLEET_B)
    return dict(X0=X0, obs=known, unknown=unknown, waypoints=FLEET_WPS)


def _fleet_slice(num_constraints, lo, hi):
    sc = fleet_scene()
    out = []
    for i in range(lo, hi):
        o = UnknownEnvOracle(R.MODEL_DI, sc["X0"][i, :4], FLEET_SPEC, obs=sc["obs"], unknown_obs=sc["unknown"],
                             num_constraints=num_constraints, yaw0=sc["X0"][i, 4])
        o.set_waypoints(sc["waypoints"])
        r = run(o, FLEET_STEPS)
        r["min_margin"] = np.array(o.min_margin)
        out.append(r)
    return out


_FLEET_CACHE = {}


def fleet_oracle(num_constraints, workers=16):
    """Every agent of fleet_scene() through the oracle, once per session and num_constraints: a list of run() records with
    `min_margin`.  The agents are spread over plain child processes (``python tests/_unknown_env_oracle.py nc lo hi out.npz``), so
    nothing depends on fork semantics of a parent that may hold a HIP context."""
    if num_constraints in _FLEET_CACHE:
        return _FLEET_CACHE[num_constraints]
    import subprocess
    import tempfile
    bounds = np.linspace(0, FLEET_B, workers + 1).astype(int)
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for w in range(workers):
            outp = os.path.join(tmp, f"o{w}.npz")
            procs.append((outp, int(bounds[w]), subprocess.Popen(
                [sys.executable, os.path.abspath(__file__), str(num_constraints), str(bounds[w]), str(bounds[w + 1]), outp])))
        res = []
        for outp, lo, pr in procs:
            if pr.wait() != 0:
                raise RuntimeError("an oracle worker failed")
            d = np.load(outp)
            n = len({k.split("/")[0] for k in d.files})
            res += [{k.split("/", 1)[1]: d[k] for k in d.files if k.startswith(f"{j}/")} for j in range(n)]
    _FLEET_CACHE[num_constraints] = res
    return res


if __name__ == "__main__":
    nc_, lo_, hi_, outp_ = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    recs = _fleet_slice(nc_, lo_, hi_)
    np.savez(outp_, **{f"{j}/{k}": v for j, r in enumerate(recs) for k, v in r.items()})
