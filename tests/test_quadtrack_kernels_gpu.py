"""GPU: quadtrack_select_kernel<8|16> and quadtrack_apply_kernel (csrc/tracking_quad.hip) against oracle/tracking_quad.py's
select() / apply(u), agent by agent, with no MPC solve in between: the injected batches of tests/_quadtrack_cases.py (every state of
the state machine, tables shorter and longer than K, circles and superellipsoids, collisions before and after the step, the VTOL2D
cone, ground and pitch tests, exact distance ties, angle wraps, frozen agents, shared waypoints), shuffled so that the lanes of a
wave take different branches.  EVERY agent is compared and none is excused: tests/test_quadtrack_cases.py shows on the CPU that no
comparison the oracle makes on these batches is within 1e-9 of its threshold, except the cases built to sit on it exactly.

Copies (state machine, indices, flags, stored goal, goal_out, the K rows with their padding, u_last, untouched states) are compared
bit for bit.  Computed values differ from the oracle only through the device's transcendentals and, for Quad3D, the closed-form
inverse of the allocation matrix against numpy's pinv.  Largest |kernel - oracle| measured on the MI355X over every launch below:
                     u_ref       X            against closed_loop_quads.npz
    Quad2D           1.8e-15     2.7e-15      nominal_input 3.6e-15, stop 8.9e-16, step 1.8e-15
    Quad3D           2.5e-14     4.4e-16      nominal_input 1.1e-14, stop 1.8e-15, rotate_to 6.2e-15, step 2.2e-16
    VTOL2D           0 (zeros)   1.8e-15      (the reference's VTOL2D loop cannot be run without its NLP solver: no recording)
The asserted bound is 16 x that, rounded up to a power of ten, and never looser than tests/test_tracking_vtol_gpu.py's 1e-12 on
inputs and 1e-11 on states (BOUND_U, BOUND_X).  Against the reference's own outputs (closed_loop_quads.npz) the bound is the one
tests/test_oracle_tracking_quad.py holds the oracle to, plus that.  f32 storage: the oracle is given the f32-rounded inputs, copies
are equal, every computed output is within one f32 ulp of the f32 rounding of the oracle's value.
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import _quadtrack_cases as Q  # noqa: E402
from oracle import tracking_quad as T  # noqa: E402
from safe_control_amd import _lib  # noqa: E402

DEV = "cuda:0"
MEASURED_U = {"Quad2D": 1.776e-15, "Quad3D": 2.487e-14, "VTOL2D": 0.0}       # largest |kernel - oracle| on the MI355X (module docstring)
MEASURED_X = {"Quad2D": 2.665e-15, "Quad3D": 4.441e-16, "VTOL2D": 1.776e-15}


def bound(measured, cap):
    """16 x the measured deviation, rounded up to a power of ten, at most `cap`; 0 where kernel and oracle agreed exactly."""
    return min(cap, 10.0 ** math.ceil(math.log10(16.0 * measured))) if measured > 0 else 0.0


BOUND_U = {m: bound(v, 1e-12) for m, v in MEASURED_U.items()}                 # 1e-13, 1e-12, 0
BOUND_X = {m: bound(v, 1e-11) for m, v in MEASURED_X.items()}                 # 1e-13, 1e-14, 1e-13
SENTINEL = -12345.0


def params(model, cfg, io, shared=False, spec=None):
    s = dict(T.default_spec(model), **(spec or {}))
    p = _lib.QuadTrackParams()
    p.model, p.io_dtype = Q.MODELS.index(model), _lib.DTYPE_F32 if io == "f32" else _lib.DTYPE_F64
    p.max_waypoints, p.waypoints_shared = Q.W, int(shared)
    p.enable_rotation, p.num_constraints = cfg["enable_rotation"], cfg["K"]
    p.dt, p.reached_threshold, p.rotation_threshold, p.robot_radius = Q.DT, cfg["reached_threshold"], 0.1, s["radius"]
    p.mass = s["mass"]
    if model == "VTOL2D":
        for i, key in enumerate(_lib.VTOL_AIRFRAME_KEYS):
            p.airframe[i] = s[key]
        p.pitch_limit = s["pitch_max"]
    elif model == "Quad3D":
        p.Ix, p.Iy, p.Iz, p.L, p.nu, p.u_min, p.u_max = (s[k] for k in ("Ix", "Iy", "Iz", "L", "nu", "u_min", "u_max"))
    else:
        p.inertia, p.f_min, p.f_max = s["inertia"], s["f_min"], s["f_max"]
    return p


def launch(c, cfg, io="f64", idx=None, shared=False, table=None, spec=None, apply=True, expect=_lib.SC_OK):
    """sc_quadtrack_select_batch, then sc_quadtrack_apply_batch on what it left, as BatchedQuadTrackingController chains them.  Returns
    numpy arrays named as in Q.run_oracle.  With `expect` != SC_OK both calls have to return that code and leave every output alone."""
    model = c["model"]
    nx, nu, npos = Q.dims(model)
    idx = np.arange(len(c["X"])) if idx is None else np.asarray(idx)
    n, K = len(idx), cfg["K"]
    ft = torch.float32 if io == "f32" else torch.float64
    tf = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=ft, device=DEV)
    ti = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.int32, device=DEV)
    table = c["table"][: cfg["M"]] if table is None else table
    M = len(table)
    X, goal, tab = tf(c["X"][idx]), tf(c["goal"][idx]), tf(table) if M else None
    wps = tf(c["waypoints"] if shared else c["waypoints"][idx] if c["waypoints"].ndim == 3 else np.tile(c["waypoints"], (n, 1, 1)))
    n_wp = ti(c["n_wp"][idx] if shared or c["waypoints"].ndim == 3 else np.full(n, c["n_wp_shared"]))
    if shared:
        assert idx[0] == 0                                       # entry 0 carries the launch's count
    wp_index, sm, ret, ret_step = ti(c["wp_index"][idx]), ti(c["sm"][idx]), ti(c["ret_in"][idx]), ti(c["ret_step_in"][idx])
    u, u_last = tf(c["u"][idx]), tf(c["u_last"][idx])
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=ft, device=DEV)
    obs_out, goal_out, u_ref, track = full(n, K, 7), full(n, npos), full(n, nu), torch.full((n,), -7, dtype=torch.int32, device=DEV)
    p = params(model, cfg, io, shared, spec)
    lib = _lib.load()
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.sc_quadtrack_select_batch(C.byref(p), n, M, ptr(X), ptr(wps), ptr(n_wp), ptr(wp_index), ptr(sm), ptr(goal), ptr(tab), ptr(ret),
                                       ptr(obs_out), ptr(goal_out), ptr(u_ref), ptr(track), None)
    assert rc == expect, lib.sc_last_error()
    if apply:
        rc = lib.sc_quadtrack_apply_batch(C.byref(p), n, M, Q.STEP_INDEX, ptr(X), ptr(sm), ptr(goal), ptr(tab), ptr(u), ptr(u_last), ptr(ret),
                                          ptr(ret_step), None)
        assert rc == expect, lib.sc_last_error()
    torch.cuda.synchronize()
    out = dict(sm=sm, wp_index=wp_index, goal=goal, obs_out=obs_out, goal_out=goal_out, u_ref=u_ref, track=track, ret=ret,
               ret_step=ret_step, X=X, u_last=u_last)
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def same(got, want, what):
    """Bit for bit (a copy of an input: -0.0 and 0.0 differ)."""
    want = np.asarray(want).astype(got.dtype)
    assert got.shape == want.shape, what
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(len(got), -1).any(axis=1)) if got.dtype.kind == "f" else np.flatnonzero(
        (got != want).reshape(len(got), -1).any(axis=1))
    assert bad.size == 0, f"{what}: rows {bad[:10]} differ, first: got {got[bad[0]]}, want {want[bad[0]]}"


def close(got, want, bound, what, io="f64"):
    """f64 storage: |got - want| <= bound.  f32 storage: within one f32 ulp of the f32 rounding of `want`."""
    if got.size == 0:
        return 0.0
    if io == "f32":
        w32 = want.astype(np.float32)
        err, lim = np.abs(got.astype(np.float64) - w32.astype(np.float64)), np.spacing(np.abs(w32)).astype(np.float64)
        j = np.unravel_index(np.argmax(err - lim), err.shape)
        assert (err <= lim).all(), f"{what}: more than one f32 ulp from the oracle at {j}: got {got[j]!r}, want {w32[j]!r}"
        return float((err / lim).max())
    err = np.abs(got - want)
    print(f"{what}: max |kernel - oracle| = {err.max():.3e} (bound {bound:.0e})")
    j = np.unravel_index(np.argmax(err), err.shape)
    assert err.max() <= bound, f"{what}: {err.max():.3e} > {bound:.0e} at {j}: got {got[j]!r}, want {want[j]!r}"
    return float(err.max())


def compare(c, g, r, idx, model, io="f64", apply=True, what=""):
    """Every agent of a launch against the oracle run `r` (rows `idx` of the batch `c`)."""
    run, frozen = r["running"], ~r["running"]
    assert len(g["sm"]) == len(run)
    # select
    same(g["sm"], r["sm"], what + " state_machine")              # frozen agents: r carries their inputs
    same(g["wp_index"], r["wp_index"], what + " wp_index")
    same(g["goal"], r["goal"], what + " goal (gx, gy, gz, valid)")
    same(g["track"], r["track"], what + " track_out")            # 0 for frozen agents
    assert (g["track"][frozen] == 0).all()
    same(g["obs_out"][run], r["obs_out"][run], what + " obs_out")
    same(g["goal_out"][run], r["goal_out"][run], what + " goal_out")
    close(g["u_ref"][run], r["u_ref"][run], BOUND_U[model], what + " u_ref", io)
    if not apply:
        return
    # apply
    same(g["ret"], r["ret"], what + " ret")
    same(g["ret_step"], r["ret_step"], what + " ret_step")
    st = r["stepped"]
    close(g["X"][st], r["X"][st], BOUND_X[model], what + " X", io)
    same(g["u_last"][st], c["u"][idx][st], what + " u_last of agents that stepped")
    same(g["X"][~st], c["X"][idx][~st], what + " X of frozen agents and of agents that collided before the step")
    same(g["u_last"][~st], c["u_last"][idx][~st], what + " u_last of frozen agents and of agents that collided before the step")
    assert (g["ret"][r["hit_after"]] == -2).all() and (g["ret"][r["hit_before"]] == -2).all()
    if r["hit_after"].any():                                     # tracking.py:636-646: the robot has stepped when the second test fails
        assert (np.abs(g["X"][r["hit_after"]] - c["X"][idx][r["hit_after"]]).max(axis=1) > 1e-3).all()


@functools.lru_cache(maxsize=None)
def main_launch(model, ci, io="f64"):
    c = Q.cases(model)
    return launch(Q.f32_rounded(c) if io == "f32" else c, Q.CONFIGS[ci], io)


@pytest.mark.parametrize("ci", range(len(Q.MAIN)))
@pytest.mark.parametrize("model", Q.MODELS)
def test_full_batch_f64(model, ci):
    """B = 200 (three waves and a partial one) over the 40-row table with K = 9, 8, 16, 1: both instantiations, enable_rotation 1 and
    0, reached_threshold 0.3 and 0.5."""
    c = Q.cases(model)
    compare(c, main_launch(model, ci), Q.reference(model, ci), np.arange(Q.B_MAIN), model, what=f"{model} {Q.CONFIGS[ci]}")


@pytest.mark.parametrize("model", Q.MODELS)
def test_table_length_edges_f64(model):
    """M in {0, 1, K - 1, K} for K in {1, 8, 9, 16} on the first 65 agents (a wave and one lane): padding rows, the empty table."""
    c = Q.cases(model)
    idx = np.arange(Q.N_SUB)
    for e, cfg in enumerate(Q.EDGE):
        g = launch(c, cfg, idx=idx)
        r = Q.reference(model, len(Q.MAIN) + e, "main", False, Q.N_SUB)
        compare(c, g, r, idx, model, what=f"{model} {cfg}")
        pad = g["obs_out"][r["running"]][:, min(cfg["M"], cfg["K"]):]
        assert (pad[:, :, :2] == 1000.0).all() and (pad[:, :, 2:] == 0.0).all()


@pytest.mark.parametrize("ci", [0, 1])
@pytest.mark.parametrize("model", Q.MODELS)
def test_full_batch_f32_storage(model, ci):
    c = Q.f32_rounded(Q.cases(model))
    g = main_launch(model, ci, "f32")
    assert g["X"].dtype == np.float32 and g["obs_out"].dtype == np.float32
    compare(c, g, Q.reference(model, ci, "main", True), np.arange(Q.B_MAIN), model, io="f32", what=f"{model} f32 {Q.CONFIGS[ci]}")


@pytest.mark.parametrize("io", ["f64", "f32"])
@pytest.mark.parametrize("model", Q.MODELS)
def test_small_batches_reproduce_their_rows(model, io):
    """B = 1 and B = 65 give the rows of the B = 200 launch bit for bit."""
    c = Q.cases(model)
    c = Q.f32_rounded(c) if io == "f32" else c
    big = main_launch(model, 0, io)
    for n in (1, Q.N_SUB):
        small = launch(c, Q.CONFIGS[0], io, idx=np.arange(n))
        for k, v in small.items():
            same(v, big[k][:n], f"{model} B = {n}: {k}")


@pytest.mark.parametrize("model", Q.MODELS)
def test_shared_waypoints(model):
    """waypoints_shared = 1 ([W,3] and n_wp[0]) against the oracle, and bit for bit against the per-agent launch with the list tiled."""
    s = Q.shared_cases(model)
    assert (s["n_wp"][1:] != 3).any()                            # only entry 0 belongs to a shared launch
    tiled = launch(s, Q.CONFIGS[0])
    compare(s, tiled, Q.reference(model, 0, "shared"), np.arange(Q.B_MAIN), model, what=f"{model} tiled waypoints")
    shared = launch(s, Q.CONFIGS[0], shared=True)
    for k, v in shared.items():
        same(v, tiled[k], f"{model} waypoints_shared: {k}")


@pytest.mark.parametrize("model", ["Quad2D", "VTOL2D"])
def test_largest_table(model):
    """M = 1170 rows (65 520 B of LDS, the most check_quadtrack accepts): the nearest rows by brute force; 1171 rows are refused with
    SC_ERR_UNSUPPORTED and nothing is written."""
    c = dict(Q.cases(model), table=Q.big_table())
    assert len(c["table"]) == 1170 and 1170 * 56 <= 65536 < 1171 * 56
    idx = np.arange(Q.N_SUB)
    g = launch(c, Q.BIG, idx=idx, table=c["table"], apply=False)
    r = Q.reference(model, -1, "main", False, Q.N_SUB)
    compare(c, g, r, idx, model, apply=False, what=f"{model} M = 1170")
    where = {tuple(row): m for m, row in enumerate(c["table"])}
    picked = {where[tuple(row)] for row in g["obs_out"][r["running"]].reshape(-1, 7)}
    assert min(picked) < 64 and max(picked) >= 1100              # rows from both ends of the staged table
    # the brute-force statement itself, without the oracle class (Quad2D: every row counts)
    if model == "Quad2D":
        for j in np.flatnonzero(r["running"])[:8]:
            d = np.hypot(c["table"][:, 0] - c["X"][j, 0], c["table"][:, 1] - c["X"][j, 1])
            same(g["obs_out"][j], c["table"][np.argsort(d, kind="stable")[:16]], "brute force")
    one_more = np.vstack([c["table"], c["table"][:1]])
    h = launch(c, Q.BIG, idx=idx, table=one_more, expect=_lib.SC_ERR_UNSUPPORTED)
    assert (h["obs_out"] == SENTINEL).all() and (h["u_ref"] == SENTINEL).all() and (h["track"] == -7).all()
    same(h["X"], c["X"][idx], "X after a refused launch")
    same(h["ret"], c["ret_in"][idx], "ret after a refused launch")
    same(h["sm"], c["sm"][idx], "state machine after a refused launch")


G = np.load(os.path.join(os.path.dirname(__file__), "golden", "closed_loop_quads.npz"))
FREE = dict(K=9, M=0, enable_rotation=1, reached_threshold=1e-6)     # no recorded state is that close to its goal: none counts as reached


def golden_batch(model, modes):
    """The 48 recorded states of closed_loop_quads.npz once per mode, as one batch: 'nominal' (in 'track' with the recorded goal),
    'stop' ('idle', no goal), 'has_stopped' ('stop': the state machine moves on exactly where the reference's has_stopped() is true)
    and, for Quad3D, 'rotate_to' ('rotate' with a waypoint 5 m away in the recorded direction).  Every agent applies the recorded
    input."""
    q = "q3" if model == "Quad3D" else "q2"
    nx, nu, npos = Q.dims(model)
    X, goal, U = G[f"{q}/X"], G[f"{q}/goal"], G[f"{q}/U"]
    n = len(X)
    far = np.zeros((n, 3))
    far[:, :2] = X[:, :2] + 50.0                                 # a waypoint nobody has reached
    assert (np.linalg.norm(X[:, :2] - goal[:, :2], axis=1) > 1e-3).all()
    c = dict(model=model, table=np.zeros((0, 7)), X=np.tile(X, (len(modes), 1)), u=np.tile(U, (len(modes), 1)))
    sm, g4, wps, idx, nwp = [], [], [], [], []
    for mode in modes:
        w = np.full((n, Q.W, 3), Q.JUNK)
        gg = np.zeros((n, 4))
        if mode == "nominal":
            w[:, 0, :npos] = goal[:, :npos]
            w[:, 0, npos:] = 0.0
            gg[:, :npos], gg[:, 3] = goal[:, :npos], 1.0
            sm.append(np.full(n, Q.TRACK)); idx.append(np.zeros(n)); nwp.append(np.ones(n))
        elif mode == "stop":
            w[:, 0] = far
            sm.append(np.full(n, Q.IDLE)); idx.append(np.ones(n)); nwp.append(np.ones(n))
        elif mode == "has_stopped":
            w[:, 0] = far
            sm.append(np.full(n, Q.STOP)); idx.append(np.zeros(n)); nwp.append(np.ones(n))
        else:
            ang = G["q3/ang"]
            w[:, 0, 0], w[:, 0, 1], w[:, 0, 2] = X[:, 0] + 5.0 * np.cos(ang), X[:, 1] + 5.0 * np.sin(ang), X[:, 2]
            gg[:, :3], gg[:, 3] = w[:, 0], 1.0
            sm.append(np.full(n, Q.ROTATE)); idx.append(np.zeros(n)); nwp.append(np.ones(n))
        g4.append(gg); wps.append(w)
    B = n * len(modes)
    c.update(sm=np.concatenate(sm).astype(np.int32), goal=np.concatenate(g4), waypoints=np.concatenate(wps),
             wp_index=np.concatenate(idx).astype(np.int32), n_wp=np.concatenate(nwp).astype(np.int32), ret_in=np.zeros(B, dtype=np.int32),
             ret_step_in=np.full(B, -1, dtype=np.int32), u_last=np.zeros((B, nu)))
    return c, n


def test_reference_executed_samples_quad3d():
    """Quad3D.nominal_input / stop / rotate_to / has_stopped / step as the reference itself executed them (closed_loop_quads.npz)."""
    modes = ("nominal", "stop", "has_stopped", "rotate_to")
    c, n = golden_batch("Quad3D", modes)
    g = launch(c, FREE)
    part = {m: slice(k * n, (k + 1) * n) for k, m in enumerate(modes)}
    bu, bx = 1e-11 + MEASURED_U["Quad3D"], 1e-12 + MEASURED_X["Quad3D"]     # tests/test_oracle_tracking_quad.py: 1e-11, 1e-12
    assert (g["sm"][part["nominal"]] == Q.TRACK).all() and (g["track"][part["nominal"]] == 1).all()
    close(g["u_ref"][part["nominal"]], G["q3/nominal"], bu, "q3 nominal_input against the reference")
    close(g["u_ref"][part["stop"]], G["q3/stop"], bu, "q3 stop against the reference")
    assert (g["ret"][part["stop"]] == -1).all()
    moved_on = g["sm"][part["has_stopped"]] != Q.STOP
    assert np.array_equal(moved_on, G["q3/has_stopped"].astype(bool)) and moved_on.any() and not moved_on.all()
    # rotate_to: the samples whose yaw is outside rotation_threshold of the recorded angle stay in 'rotate'
    yaw, ang = G["q3/X"][:, 5], G["q3/ang"]
    out = np.abs(yaw - ang) > 0.1 + 1e-6
    assert out.sum() >= n // 2 and (g["sm"][part["rotate_to"]][out] == Q.ROTATE).all()
    close(g["u_ref"][part["rotate_to"]][out], G["q3/rotate_to"][out], bu, "q3 rotate_to against the reference")
    close(g["X"], np.tile(G["q3/step"], (len(modes), 1)), bx, "q3 step against the reference")
    same(g["u_last"], c["u"], "u_last")


def test_reference_executed_samples_quad2d():
    """Quad2D.nominal_input / stop / has_stopped / step as the reference executed them, with the f_min = 3 of that recording."""
    modes = ("nominal", "stop", "has_stopped")
    c, n = golden_batch("Quad2D", modes)
    g = launch(c, FREE, spec=dict(f_min=3.0, f_max=10.0, radius=0.25))
    part = {m: slice(k * n, (k + 1) * n) for k, m in enumerate(modes)}
    bu, bx = 1e-12 + MEASURED_U["Quad2D"], 1e-12 + MEASURED_X["Quad2D"]     # tests/test_oracle_tracking_quad.py: 1e-12
    assert (g["sm"][part["nominal"]] == Q.TRACK).all() and (g["track"][part["nominal"]] == 1).all()
    close(g["u_ref"][part["nominal"]], G["q2/nominal"], bu, "q2 nominal_input against the reference")
    close(g["u_ref"][part["stop"]], G["q2/stop"], bu, "q2 stop against the reference")
    moved_on = g["sm"][part["has_stopped"]] != Q.STOP
    assert np.array_equal(moved_on, G["q2/has_stopped"].astype(bool)) and moved_on.any() and not moved_on.all()
    close(g["X"], np.tile(G["q2/step"], (len(modes), 1)), bx, "q2 step against the reference")
