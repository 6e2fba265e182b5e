"""CPU: the host logic the MPC position controllers share (safe_control_amd/position_control/_mpc_host.py) under every class built
on it.  The library loads without a GPU, and constructors, parameter builders and input checks run before any HIP call: dispatch of
the two drop-in names; the bytes of every batched class's ``_params`` against its module's builder called with the arguments the
class documents (stated here as a table); the model blob of the Quad3D optimal-decay extension; the one input check with every
class's own numbers (the shape cases on stand-in tensors that say they are device tensors); the drop-ins outside 'track' and their
zero-padded rows."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from safe_control_amd import _lib  # noqa: E402
from safe_control_amd.position_control import (_mpc_host, mpc_cbf as M, mpc_cbf_gn as G, mpc_cbf_linear as L, mpc_cbf_ms as MS,  # noqa: E402
                                               mpc_cbf_vtol as V, mpc_cbf_vtol_ms as VMS, optimal_decay_mpc_cbf as OD,
                                               optimal_decay_mpc_cbf_gn as ODG)

DT, TOL, MAX_ITER, RADIUS = 0.04, 1e-5, 200, 0.3
IO = {"f32": _lib.DTYPE_F32, "f64": _lib.DTYPE_F64}
KB3 = ["KinematicBicycle2D", "KinematicBicycle2D_C3BF", "KinematicBicycle2D_DPCBF"]


class Robot:
    dt, robot_radius = DT, 0.35


def _gn(c, io, sh):
    return G.make_params(c.robot_spec, G.model_constants(c.robot_spec), c.cbf_param, 10, DT, RADIUS, io, obs_shared=sh, tol=TOL, max_iter=MAX_ITER)


def _lin(c, io, sh, **kw):
    return L.make_params(c._mdl, c.cbf_param, 10, RADIUS, io, obs_shared=sh, tol=TOL, max_iter=MAX_ITER, **kw)


def _odlin(c, io, sh, circles_only):
    p = _lin(c, io, sh)
    p.optimal_decay, p.od_omega_ref, p.od_p_sb, p.circles_only = 1, 1.0, 10.0, circles_only
    return p


def _ms(c, io, sh):
    Q, R = M.default_mpc_weights(c.robot_spec["model"])
    return M.make_params(c.robot_spec, c.cbf_param, Q, R, 10, DT, RADIUS, io, obs_shared=sh)         # tolerances and budget travel in sc_ipopt_params


def _du(c, io, sh, **kw):
    Q, R = M.default_mpc_weights(c.robot_spec["model"])
    return M.make_params(c.robot_spec, c.cbf_param, Q, R, 10, DT, RADIUS, io, obs_shared=sh, tol=TOL, max_iter=MAX_ITER, **kw)


def _od(c, io, sh, slack_reset):
    Q, R = M.default_mpc_weights(c.robot_spec["model"])
    return OD.make_od_mpc_params(c.robot_spec, c.cbf_param, Q, R, 10, DT, RADIUS, io, obs_shared=sh, tol=TOL, max_iter=MAX_ITER, slack_reset=slack_reset)


# name: (class, constructor keywords, models served, a model refused, (nx, nu, ng) by model, honours ``resto``, takes tol / max_iter,
#        the module-level builder with the arguments the class documents: (controller, io_dtype, obs_shared) -> struct)
BATCHED = {
    "mpccbf": (M.BatchedMPCCBF, {}, ["DynamicUnicycle2D", "Unicycle2D"], "Quad2D", lambda m: (4, 2, 2), True, True, _du),
    "lin": (L.BatchedLinearMPCCBF, {}, ["SingleIntegrator2D", "Quad3D"], "DynamicUnicycle2D",
            lambda m: (12, 4, 3) if m == "Quad3D" else (2, 2, 2), True, True, lambda c, io, sh: _lin(c, io, sh, input_rterm="du")),
    "lin_u2": (L.BatchedLinearMPCCBF, {"input_rterm": "u2"}, ["Quad3D"], "DynamicUnicycle2D", lambda m: (12, 4, 3), True, True,
               lambda c, io, sh: _lin(c, io, sh, input_rterm="u2")),
    "odlin": (L.BatchedOptimalDecayLinearMPCCBF, {}, ["Quad3D"], "SingleIntegrator2D", lambda m: (12, 4, 3), False, True,
              lambda c, io, sh: _odlin(c, io, sh, 0)),
    "odlin_circles": (L.BatchedOptimalDecayLinearMPCCBF, {"superellipsoids": False}, ["Quad3D"], "SingleIntegrator2D", lambda m: (12, 4, 3),
                      False, True, lambda c, io, sh: _odlin(c, io, sh, 1)),
    "gn": (G.BatchedGnMPCCBF, {}, ["DoubleIntegrator2D", "Quad2D"] + KB3, "DynamicUnicycle2D", lambda m: (6 if m == "Quad2D" else 4, 2, 2),
           True, True, lambda c, io, sh: _gn(c, io, sh)),
    "vtol": (V.BatchedVtolMPCCBF, {}, ["VTOL2D"], "DynamicUnicycle2D", lambda m: (6, 4, 2), True, True,
             lambda c, io, sh: V.make_params(c.robot_spec, c.cbf_param, 30, DT, RADIUS, io, obs_shared=sh, tol=TOL, max_iter=MAX_ITER, slack_reset=2, kernel=0)),
    "odvtol": (V.BatchedOptimalDecayVtolMPCCBF, {}, ["VTOL2D"], "DynamicUnicycle2D", lambda m: (6, 4, 2), False, True,
               lambda c, io, sh: V.make_od_params(c.robot_spec, c.cbf_param, 30, DT, RADIUS, io, obs_shared=sh, tol=TOL, max_iter=MAX_ITER)),
    "ms": (MS.BatchedMSMPCCBF, {}, ["DynamicUnicycle2D", "Unicycle2D", "SingleIntegrator2D", "DoubleIntegrator2D", "KinematicBicycle2D"], "Quad2D",
           lambda m: (4, 2, 2), False, False, _ms),
    "vtolms": (VMS.BatchedVtolMSMPCCBF, {}, ["VTOL2D"], "DynamicUnicycle2D", lambda m: (6, 4, 2), False, False,
               lambda c, io, sh: V.make_params(c.robot_spec, c.cbf_param, 30, DT, RADIUS, io, obs_shared=sh)),
    "odvtolms": (VMS.BatchedOptimalDecayVtolMSMPCCBF, {}, ["VTOL2D"], "DynamicUnicycle2D", lambda m: (6, 4, 2), False, False,
                 lambda c, io, sh: V.make_od_params(c.robot_spec, c.cbf_param, 30, DT, RADIUS, io, obs_shared=sh)),
    "od": (OD.BatchedOptimalDecayMPCCBF, {}, ["DynamicUnicycle2D"], "Unicycle2D", lambda m: (4, 2, 2), False, True, lambda c, io, sh: _od(c, io, sh, 0)),
    "od_ext": (OD.BatchedOptimalDecayMPCCBF, {"extension": True}, ["DynamicUnicycle2D", "Unicycle2D"], "KinematicBicycle2D", lambda m: (4, 2, 2), False, True,
               lambda c, io, sh: _od(c, io, sh, 2 if c.robot_spec["model"] == "Unicycle2D" else 0)),
    "odgn": (ODG.BatchedOptimalDecayGnMPCCBF, {}, ["KinematicBicycle2D", "Quad2D"], "DoubleIntegrator2D", lambda m: (6 if m == "Quad2D" else 4, 2, 2),
             False, True, lambda c, io, sh: ODG.make_od_params(c.robot_spec, ODG.od_model_constants(c.robot_spec), c.cbf_param, 10, DT, RADIUS, io,
                                                               obs_shared=sh, tol=TOL, max_iter=MAX_ITER)),
}
CASES = [(name, model) for name, row in BATCHED.items() for model in row[2]]


def build(name, model, io="f64"):
    cls, kw, _, _, _, _, budget, _ = BATCHED[name]
    kw = dict(kw, **({"tol": TOL, "max_iter": MAX_ITER} if budget else {}))
    return cls({"model": model, "radius": RADIUS}, dt=DT, io_dtype=io, **kw)


def test_dispatch_of_the_two_drop_in_names():
    want = {"DynamicUnicycle2D": M.MPCCBF, "Unicycle2D": M.MPCCBF, "SingleIntegrator2D": L.LinearMPCCBF, "Quad3D": L.LinearMPCCBF,
            "DoubleIntegrator2D": G.GnMPCCBF, "Quad2D": G.GnMPCCBF, "VTOL2D": V.VtolMPCCBF, **{m: G.GnMPCCBF for m in KB3}}
    for model, cls in want.items():
        assert type(M.MPCCBF(Robot(), {"model": model})) is cls, model
    want = {"DynamicUnicycle2D": OD.OptimalDecayMPCCBF, "KinematicBicycle2D": ODG.OptimalDecayGnMPCCBF, "Quad2D": ODG.OptimalDecayGnMPCCBF,
            "Quad3D": L.OptimalDecayLinearMPCCBF, "VTOL2D": V.OptimalDecayVtolMPCCBF}
    for model, cls in want.items():
        ctl = OD.OptimalDecayMPCCBF(Robot(), {"model": model})
        assert type(ctl) is cls and ctl.omega1 is None and ctl.omega2 is None, model


@pytest.mark.parametrize("name", list(BATCHED))
def test_a_model_the_class_does_not_serve_is_refused(name):
    with pytest.raises(NotImplementedError):
        build(name, BATCHED[name][3])


@pytest.mark.parametrize("io", ["f32", "f64"])
@pytest.mark.parametrize("name,model", CASES)
def test_parameter_struct_is_the_builders(name, model, io):
    ctl, (honours, builder) = build(name, model, io), BATCHED[name][5::2]
    assert ctl.io_dtype == IO[io] and ctl.horizon == (30 if model == "VTOL2D" else 10)
    for shared in (False, True):
        p = ctl._params(shared)
        assert (p.mpc if hasattr(p, "mpc") else p).obs_shared == int(shared)
        assert bytes(p) == bytes(builder(ctl, IO[io], shared)) and bytes(p) == bytes(ctl._params(shared)), (name, model, shared)
    before = bytes(ctl._params())
    ctl.resto = _lib.default_resto(stall_iter=2, stall_theta=1e-9)
    p = ctl._params()
    if honours:
        assert (p.resto.stall_iter, p.resto.stall_theta) == (2, 1e-9) and bytes(p) != before
    else:                                                                     # the optimal-decay and multiple-shooting classes do not read it
        assert bytes(p) == before


def test_what_is_a_class_s_own_reaches_its_struct():
    ctl = build("vtol", "VTOL2D")
    ctl.kernel, ctl.slack_reset = 1, 0
    assert (ctl._params().kernel, ctl._params().slack_reset) == (1, 0)
    assert build("od_ext", "Unicycle2D")._params().mpc.slack_reset == 2 and build("od_ext", "DynamicUnicycle2D")._params().mpc.slack_reset == 0
    assert build("lin_u2", "Quad3D")._params().optimal_decay == 2 and build("lin", "Quad3D")._params().optimal_decay == 0
    assert build("odlin", "Quad3D")._params().circles_only == 0 and build("odlin_circles", "Quad3D")._params().circles_only == 1
    assert build("ms", "DynamicUnicycle2D")._params(False, superellipsoid_rows=1).superellipsoid_rows == 1
    ms = build("ms", "DynamicUnicycle2D")
    assert ms.max_iter == 3000 and ms.iter_slices == () and ms.plan_width == 11 * 4 + 10 * 2 and ms.io_name == "f64"
    ms = MS.BatchedMSMPCCBF(max_iter=77, ipopt={"tol": 1e-7})
    assert ms.max_iter == 77 and ms.ipopt == {"tol": 1e-7, "max_iter": 77}
    vms = VMS.BatchedVtolMSMPCCBF(ipopt={"max_iter": 55})
    assert vms.max_iter == 55 and vms.plan_width == 31 * 6 + 30 * 4 and type(vms.condensed) is V.BatchedVtolMPCCBF and vms.n_fallback == 0
    assert type(VMS.BatchedOptimalDecayVtolMSMPCCBF().condensed) is V.BatchedOptimalDecayVtolMPCCBF
    assert VMS.BatchedOptimalDecayVtolMSMPCCBF(fallback=False).condensed is None
    for name in ("mpccbf", "lin", "gn", "vtol"):                               # the classes that honour it create it
        assert build(name, BATCHED[name][2][-1]).resto is None
    ctl = build("mpccbf", "DynamicUnicycle2D")
    assert ctl.iter_slices == (_lib.FIRST_CAP,) and ctl.classify_first and ctl._slice_ws is None
    for f in ("_mpc_host", "mpc_cbf", "mpc_cbf_linear", "mpc_cbf_gn", "mpc_cbf_vtol", "mpc_cbf_ms", "mpc_cbf_vtol_ms", "optimal_decay_mpc_cbf",
              "optimal_decay_mpc_cbf_gn"):
        src = open(os.path.join(ROOT, "safe_control_amd", "position_control", f + ".py")).read()
        assert not re.search(r"getattr\(self,[^,()]*,", src), f                # no attribute that no constructor creates


def test_blob_of_the_quad3d_extension_is_built_once_from_its_own_struct():
    ctl = build("odlin", "Quad3D")
    assert ctl._blob_dev == {}
    assert np.array_equal(ctl._blob_host, L.build_model_blob(ctl._lib, ctl._params(), ctl._mdl))
    plain = build("lin", "Quad3D")
    assert np.array_equal(plain._blob_host, L.build_model_blob(plain._lib, plain._params(), plain._mdl))
    assert not np.array_equal(ctl._blob_host, plain._blob_host)               # the cost Hessian of the blob depends on the input term
    # ... and on nothing a call may change
    assert np.array_equal(ctl._blob_host, L.build_model_blob(ctl._lib, L.BatchedOptimalDecayLinearMPCCBF({"model": "Quad3D", "radius": RADIUS}, dt=DT)._params(True),
                                                            ctl._mdl))


class Dev:
    """Stands in for a device tensor where the check reads nothing but these."""

    def __init__(self, shape, dtype=torch.float64, cuda=True, contiguous=True):
        self.shape, self.dtype, self.is_cuda, self._contiguous = tuple(shape), dtype, cuda, contiguous

    def is_contiguous(self):
        return self._contiguous

    def dim(self):
        return len(self.shape)


@pytest.mark.parametrize("name,model", CASES)
def test_input_check(name, model):
    ctl = build(name, model)
    nx, nu, ng = BATCHED[name][4](model)
    assert (ctl.nx, ctl.nu, ctl.ng) == (nx, nu, ng)
    B, K = 3, 2
    good = {"X": (B, nx), "u_prev": (B, nu), "goal": (B, ng), "obs": (B, K, 7)}
    order = list(good)
    assert ctl._check(*[Dev(good[k]) for k in order]) == (B, K, False)
    assert ctl._check(*[Dev(good[k]) for k in order[:3]], Dev((K, 7))) == (B, K, True)
    for k in order:                                                           # a host tensor, a wrong dtype, a strided view
        bad = {"host": torch.zeros(good[k], dtype=torch.float64), "dtype": Dev(good[k], dtype=torch.float32), "strided": Dev(good[k], contiguous=False)}
        for why, t in bad.items():
            with pytest.raises(ValueError, match=re.escape(f"{k} must be a contiguous CUDA tensor of dtype torch.float64")):
                ctl.solve(*[t if j == k else Dev(good[j]) for j in order])
    text = re.escape(f"expected X[B,{nx}], u_prev[B,{nu}], goal[B,{ng}], obs[B,K,7] or obs[K,7]")
    # (a SingleIntegrator2D row of two columns is the multiple-shooting class's own: it widens it)
    wrong = {"X": (B, nx + 1), "u_prev": (B, nu + 1), "goal": (B, ng + 1), "obs": (B, K, 6)}
    for k in order:
        with pytest.raises(ValueError, match=text):
            ctl.solve(*[Dev(wrong[k] if j == k else good[j]) for j in order])
    for shape in ((B + 1, K, 7), (K, 6)):                                     # another batch, a shared table of another width
        with pytest.raises(ValueError, match=text):
            ctl.solve(*[Dev(good[k]) for k in order[:3]], Dev(shape))
    with pytest.raises(ValueError, match=text):
        ctl.solve(Dev((B, nx)), Dev((B + 1, nu)), Dev((B, ng)), Dev((B, K, 7)))


DROP_INS = [(M.MPCCBF, "DynamicUnicycle2D", {}, 4, 4, 2), (M.MPCCBF, "Unicycle2D", {}, 3, 4, 2), (M.MPCCBF, "DynamicUnicycle2D", {"mpc_formulation": "condensed"}, 4, 4, 2),
            (M.MPCCBF, "SingleIntegrator2D", {}, 2, 2, 2), (M.MPCCBF, "Quad3D", {}, 12, 12, 3), (M.MPCCBF, "DoubleIntegrator2D", {}, 4, 4, 2),
            (M.MPCCBF, "KinematicBicycle2D", {}, 4, 4, 2), (M.MPCCBF, "Quad2D", {}, 6, 6, 2), (M.MPCCBF, "VTOL2D", {}, 6, 6, 2),
            (OD.OptimalDecayMPCCBF, "DynamicUnicycle2D", {}, 4, 4, 2), (OD.OptimalDecayMPCCBF, "KinematicBicycle2D", {}, 4, 4, 2),
            (OD.OptimalDecayMPCCBF, "Quad2D", {}, 6, 6, 2), (OD.OptimalDecayMPCCBF, "Quad3D", {}, 12, 12, 3), (OD.OptimalDecayMPCCBF, "VTOL2D", {}, 6, 6, 2)]


@pytest.mark.parametrize("cls,model,spec,n_states,row,ng", DROP_INS, ids=[f"{c.__name__}-{m}-{'-'.join(s.values())}" for c, m, s, *_ in DROP_INS])
def test_drop_in_outside_track_and_its_rows(cls, model, spec, n_states, row, ng):
    ctl = cls(Robot(), dict(spec, model=model), num_obs=3)
    assert ctl.n_states == n_states and ctl.status == "optimal" and ctl.solver_status == "optimal" and ctl.iterations == 0
    assert ctl.u_prev.shape == (ctl.n_controls,) and not ctl.u_prev.any() and ctl.z.shape == (ctl.n_controls * ctl.horizon,)
    u_ref = np.array([[0.1], [0.2]])
    seven = [1.0, 2.0, 0.5, 0.1, 0.2, 0.0, 1.0]
    for obs in (None, [], [[1.0, 2.0, 0.5]], [seven, [3.0, 4.0, 0.25]], np.arange(28.0).reshape(4, 7)):
        for sm in ("stop", "rotate", "idle"):
            goal = [4.0, 5.0, 1.5][:ng]
            u = ctl.solve_control_problem(np.zeros(n_states), {"goal": goal, "state_machine": sm, "u_ref": u_ref}, obs)
            assert u is u_ref
            assert np.array_equal(ctl.goal, np.array(goal)) and ctl.obs.shape == (3, 7) and np.array_equal(ctl.obs, M.pad_obstacles(obs, 3))
    assert np.array_equal(ctl.obs, np.arange(21.0).reshape(3, 7))             # extra rows are dropped
    ctl.update_tvp([1.0, 2.0], [[1.0, 2.0, 0.5]])
    assert np.array_equal(ctl.obs[0], [1.0, 2.0, 0.5, 0, 0, 0, 0]) and np.array_equal(ctl.obs[1:], np.tile(_mpc_host.DUMMY_OBS, (2, 1)))
    with pytest.raises(ValueError, match="Invalid obstacle format"):
        ctl.update_tvp([1.0, 2.0], [[1.0, 2.0, 0.5, 0.0]])
    # the rows the library reads: the model's width, a shorter state or goal zero-padded, a longer one cut
    ctl.update_tvp([7.0, 8.0, 9.0, 10.0], None)
    X, g = ctl._rows(np.arange(1.0, 20.0).reshape(-1, 1))
    assert X.dtype == np.float64 and X.flags.c_contiguous and np.array_equal(X, list(range(1, n_states + 1)) + [0.0] * (row - n_states))
    assert g.dtype == np.float64 and np.array_equal(g, [7.0, 8.0, 9.0][:ng])
    ctl.update_tvp([7.0], None)
    X, g = ctl._rows([1.5])
    assert X.shape == (row,) and X[0] == 1.5 and not X[1:].any() and np.array_equal(g, [7.0] + [0.0] * (ng - 1))
