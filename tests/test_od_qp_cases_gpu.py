"""GPU tests of the optimal-decay CBF-QP kernel (csrc/od_cbf_qp.hip over csrc/od_qp.hpp) on the constructed batches of
tests/_od_qp_cases.py (pytest -m gpu): every one of the 18 active sets of od_solve with a margin, the superellipsoid branch of the row
build, all three dtype pairs, and the edges of the launch.  One launch per model and dtype pair; the oracle's answers are computed
once per process (Q.cases / Q.f32_cases) and shared.

tests/test_od_qp_cases.py checks on the CPU that the batches are what they claim to be, that the oracle solves every case and that
the certificate used below accepts the oracle's answers and refuses wrong ones."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import _od_qp_cases as Q  # noqa: E402
import safe_control_amd as sca  # noqa: E402

DEV = "cuda:0"
TOL = {"f64": 1e-7, "f32": 3e-6}                       # the bounds of tests/test_odcbfqp_gpu.py, each scaled by max(1, |value|)
INFEASIBLE, BAD_OBSTACLE = 1, Q.STATUS_BAD_OBSTACLE

# f32 storage AND f32 arithmetic: the worst scaled error against the oracle (on the f32-rounded inputs) per model and class, measured
# on an MI355X, and the bound asserted: four times the worst case, rounded up to one digit (the factor allows for compiler and
# contraction changes between builds).  No bound can be derived here: in the corner classes omega - omega_ref ~ -s / e, and s cancels.
F32_MEASURED = {    # max of the u and omega columns; classes in the order of Q.CLASSES
    "DynamicUnicycle2D": (0.0, 1.5e-09, 1.5e-09, 3.0e-09, 3.0e-09, 3.0e-09, 3.0e-09, 3.0e-09, 3.0e-09, 1.6e-07, 1.6e-07, 3.0e-07, 3.6e-06, 1.5e-07, 1.6e-07, 1.3e-06, 7.7e-08, 1.6e-07),
    "KinematicBicycle2D": (0.0, 7.5e-10, 7.5e-10, 1.2e-08, 1.2e-08, 1.2e-08, 1.2e-08, 1.2e-08, 1.2e-08, 1.2e-07, 1.4e-07, 2.5e-07, 2.4e-05, 9.5e-08, 1.0e-07, 9.3e-07, 4.1e-06, 1.1e-07),
    "KinematicBicycle2D_C3BF": (0.0, 7.5e-10, 7.5e-10, 1.2e-08, 1.2e-08, 1.2e-08, 1.2e-08, 1.2e-08, 1.2e-08, 5.0e-07, 7.3e-07, 3.6e-06, 8.1e-07, 7.1e-06, 1.7e-06, 5.3e-06, 7.0e-06, 3.0e-06),
    "KinematicBicycle2D_DPCBF": (0.0, 7.5e-10, 7.5e-10, 1.2e-08, 1.2e-08, 1.2e-08, 1.2e-08, 1.2e-08, 1.2e-08, 4.4e-07, 4.5e-07, 4.3e-07, 1.4e-06, 5.7e-07, 3.9e-07, 5.7e-06, 1.2e-06, 8.7e-07),
    "Quad2D": (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.4e-07, 2.2e-07, 1.9e-07, 2.8e-07, 4.2e-07, 7.1e-07, 2.4e-07, 7.3e-07, 7.0e-07),
}


def _four_times_rounded_up(v):
    """4 v rounded up to one significant digit (0 stays 0: where both sides only clamp and copy, the outputs are equal)."""
    if v == 0.0:
        return 0.0
    e = math.floor(math.log10(4.0 * v))
    return math.ceil(4.0 * v / 10.0 ** e - 1e-9) * 10.0 ** e


F32_BOUND = {key: dict(zip(Q.CLASSES, map(_four_times_rounded_up, row))) for key, row in F32_MEASURED.items()}


def launch(c, io, comp, X=None, u_ref=None, obs=None, has_obs="ones", idx=None):
    """One launch of the kernel on the batch c (inputs optionally replaced / selected by idx): u, omega, status, h as numpy (f64)."""
    X, u_ref, obs = (c[k] if a is None else a for k, a in (("X", X), ("u_ref", u_ref), ("obs", obs)))
    if idx is not None:
        X, u_ref, obs = X[idx], u_ref[idx], obs[idx]
    ctl = sca.BatchedOptimalDecayCBFQP(dict(c["spec"]), io_dtype=io, compute_dtype=comp)
    tX, tu, to = (torch.tensor(np.ascontiguousarray(a), dtype=ctl.torch_dtype, device=DEV) for a in (X, u_ref, obs))
    if isinstance(has_obs, str):
        th = None if has_obs == "none" else torch.ones(len(X), dtype=torch.int32, device=DEV)
    else:
        th = torch.tensor(np.asarray(has_obs if idx is None else has_obs[idx], dtype=np.int32), device=DEV)
    u, w, st, h = ctl.solve(tX, tu, to, th)
    torch.cuda.synchronize()
    return u.double().cpu().numpy(), w.double().cpu().numpy(), st.cpu().numpy(), h.double().cpu().numpy()


def scaled_errors(c, u, w, h):
    """Per case: |u - u*| / max(1, |u*|max), |omega - omega*| / max(1, |omega*|max), |h - h*| / max(1, |h*|)."""
    eu = np.abs(u - c["u"]).max(axis=1) / np.maximum(1.0, np.abs(c["u"]).max(axis=1))
    ew = np.abs(w - c["omega"]).max(axis=1) / np.maximum(1.0, np.abs(c["omega"]).max(axis=1))
    eh = np.abs(h - c["h"]) / np.maximum(1.0, np.abs(c["h"]))
    return eu, ew, eh


def per_class(c, err):
    return {k: float(err[c["cls"] == k].max()) for k in Q.CLASSES if (c["cls"] == k).any()}


def report(title, c, eu, ew, eh):
    print(f"\n{title}: B = {len(c['X'])}")
    print(f"  {'class':16s} {'n':>4s} {'u':>10s} {'omega':>10s} {'h':>10s}")
    for k in Q.CLASSES:
        m = c["cls"] == k
        if m.any():
            print(f"  {k:16s} {int(m.sum()):4d} {eu[m].max():10.2e} {ew[m].max():10.2e} {eh[m].max():10.2e}")


# superellipsoid barriers reach 1e4 .. 1e8: compared in f64 storage only, as in tests/test_cbfqp_gpu.py
@pytest.mark.parametrize("key,io,comp", [(k, "f64", "f64") for k in Q.KEYS] + [(k, "f32", "f64") for k in Q.MODEL_NAMES])
def test_every_active_set_against_oracle_and_certificate(key, io, comp):
    """Status equal on every case, no exemptions; u, omega, h within the project's bounds of the oracle; and, in f64 storage, the
    certificate accepts the kernel's own output: by strong convexity it is then within 1e-7 of THE minimiser, whatever the oracle says."""
    c = Q.cases(key) if io == "f64" else Q.f32_cases(key)
    u, w, st, h = launch(c, io, comp)
    eu, ew, eh = scaled_errors(c, u, w, h)
    report(f"{key} {io}/{comp}", c, eu, ew, eh)
    assert np.array_equal(st, c["status"]), np.flatnonzero(st != c["status"])
    for name, e in (("u", eu), ("omega", ew), ("h", eh)):
        assert e.max() <= TOL[io], (name, int(e.argmax()), c["cls"][e.argmax()], float(e.max()))
    if io == "f64":
        worst = 0.0
        for i, qp in enumerate(c["qp"]):
            x = np.concatenate([u[i], w[i]])[:len(qp[0])]
            cert = Q.certificate(*qp, x)
            assert Q.accepts(cert, x, TOL[io]), (i, c["cls"][i], cert)
            worst = max(worst, cert["bound"] / max(1.0, float(np.abs(x).max())))
        print(f"  certificate: every output within {worst:.2e} (scaled) of the minimiser")
        if c["model"] not in Q.R.REL_DEG2:
            assert (w[:, 1] == 1.0).all()                     # the inert omega2 of the rel-degree-1 models is reported at its reference


@pytest.mark.parametrize("key", Q.MODEL_NAMES)
def test_f32_arithmetic(key):
    """odcbfqp_kernel<float, float, M>: tol_feas is 1e-5 there and p_sb = 1e4 sits in e*e/p.  The class margins are a thousand times
    tol_feas, so the status equals the oracle's on every case; u and omega are held to F32_BOUND = 4 x F32_MEASURED, the table
    measured on an MI355X (worst scaled error of u and omega against the oracle on the f32-rounded inputs).  Its worst figures:

      model    row inactive (9 classes)   row active, worst class      the four corner classes
      DU       0 .. 3.0e-9                3.6e-6  (act/lo/free)        7.7e-8 .. 1.6e-7
      KB       0 .. 1.2e-8                2.4e-5  (act/lo/free)        9.5e-8 .. 4.1e-6
      C3BF     0 .. 1.2e-8                7.1e-6  (act/lo/lo)          1.7e-6 .. 7.1e-6
      DPCBF    0 .. 1.2e-8                5.7e-6  (act/hi/free)        3.9e-7 .. 1.2e-6
      Quad2D   0 (exact)                  7.3e-7  (act/hi/lo)          4.2e-7 .. 7.3e-7

    With the row inactive the kernel clamps and copies: the error is the f32 rounding of the box (0.1, 0.2, 0.3, 0.05; 3 and 10 are
    exact).  The largest figures are inputs that end free inside a box 0.1 wide from a reference up to |a_j| ~ 35 outside it:
    u = r + lam a / 2 cancels there, whatever the order of operations.  No class is more than 1e3 times its f32/f64 error (the
    largest ratio is 400, KB act/lo/free: 2.4e-5 against 5.9e-8)."""
    c = Q.f32_cases(key)
    u, w, st, h = launch(c, "f32", "f32")
    eu, ew, eh = scaled_errors(c, u, w, h)
    report(f"{key} f32/f32", c, eu, ew, eh)
    e = np.maximum(eu, ew)
    print("  measured:", {k: float(f"{v:.1e}") for k, v in per_class(c, e).items()})
    assert np.array_equal(st, c["status"]), np.flatnonzero(st != c["status"])
    for k, v in per_class(c, e).items():
        assert v <= F32_BOUND[key][k], (k, v, F32_BOUND[key][k])


@pytest.mark.parametrize("key", (Q.DU, Q.DPCBF))
def test_missing_obstacle(key):
    """has_obs = None is has_obs = 1 everywhere, bit for bit; a row with has_obs = 0 returns clamp(u_ref), the reference omegas, h = 0
    and 'optimal', and its obstacle row is not read: NaN there changes nothing."""
    c = Q.cases(key)
    B = len(c["X"])
    ones = launch(c, "f64", "f64")
    none = launch(c, "f64", "f64", has_obs="none")
    for a, b in zip(ones, none):
        assert np.array_equal(a, b, equal_nan=True)
    has = np.ones(B, dtype=np.int32)
    has[::5] = 0
    obs = c["obs"].copy()
    obs[::10] = np.nan                                        # half of the rows without an obstacle hold NaN
    u, w, st, h = launch(c, "f64", "f64", obs=obs, has_obs=has)
    off = has == 0
    lo, hi = Q.OD.input_bounds(c["model"], c["ospec"])
    assert np.array_equal(u[off], np.clip(c["u_ref"][off], lo, hi)) and (w[off] == 1.0).all() and (h[off] == 0.0).all() and (st[off] == 0).all()
    on = ~off
    for a, b in zip((u, w, st, h), ones):
        assert np.array_equal(a[on], b[on])


@pytest.mark.parametrize("key", (Q.DU, Q.C3BF, Q.DPCBF))
def test_non_finite_inputs_stay_in_their_lane(key):
    """NaN or Inf in one agent's X, u_ref or obstacle row: that agent is 'infeasible' with NaN u and omega, every other agent's outputs
    are bitwise what they were.  One launch per (value, array): the struck agents are 28 lanes apart, each with another entry struck.

    Struck are the entries the row depends on: the whole state, both references, the obstacle's centre and radius, and its velocity
    where the barrier reads it.  One exemption: an INFINITE radius under the rel-degree-1 bicycles.  Their barriers clamp
    |p|^2 - ego^2 at eps from below, so ego = +-inf gives a finite row -- in the reference and in the oracle as well -- and the QP is
    solved.  A NaN radius is struck: the reference's max(., eps) hands it on, and so must the kernel."""
    c = Q.cases(key)
    B = len(c["X"])
    base = launch(c, "f64", "f64")
    for val in (np.nan, np.inf, -np.inf):
        obs_cols = (0, 1, 2) if key == Q.DU else ((0, 1, 2, 3, 4) if np.isnan(val) else (0, 1, 3, 4))
        for name, cols in (("X", (0, 1, 2, 3)), ("u_ref", (0, 1)), ("obs", obs_cols)):
            arr = c[name].copy()
            struck = np.arange(3, B, 28)[:len(cols) * 2]
            assert len(struck) == len(cols) * 2
            for n, i in enumerate(struck):
                arr[i, cols[n % len(cols)]] = val
            u, w, st, h = launch(c, "f64", "f64", **{name: arr})
            assert (st[struck] == INFEASIBLE).all(), (val, name, st[struck])
            assert np.isnan(u[struck]).all() and np.isnan(w[struck]).all()
            rest = np.setdiff1d(np.arange(B), struck)
            for a, b in zip((u, w, st, h), base):
                assert np.array_equal(a[rest], b[rest]), (val, name)


@pytest.mark.parametrize("key", (Q.C3BF, Q.DPCBF))
def test_infinite_radius_is_solved_like_the_oracle_solves_it(key):
    """The exemption above, held to the oracle rather than left alone: with an infinite obstacle radius the rel-degree-1 barriers are
    finite, and kernel and oracle agree on status, u, omega and h."""
    c = Q.cases(key)
    idx = np.arange(5, 5 + 16)
    obs = c["obs"][idx].copy()
    obs[::2, 2], obs[1::2, 2] = np.inf, -np.inf
    ref = Q.resolve(c, c["X"][idx], c["u_ref"][idx], obs)
    u, w, st, h = launch(c, "f64", "f64", X=c["X"][idx], u_ref=c["u_ref"][idx], obs=obs)
    assert np.array_equal(st, ref["status"]) and (st == 0).all()
    eu, ew, eh = scaled_errors(ref, u, w, h)
    assert max(eu.max(), ew.max(), eh.max()) <= TOL["f64"], (eu.max(), ew.max(), eh.max())


def test_bad_obstacle_flag():
    """DynamicUnicycle2D: a flag that is neither 0 nor 1 gives SC_STATUS_BAD_OBSTACLE and NaN outputs, for that agent alone."""
    c = Q.cases(Q.DU)
    B = len(c["X"])
    base = launch(c, "f64", "f64")
    obs = c["obs"].copy()
    struck = np.array([1, 64, 255, 256, B - 1, 100])
    obs[struck, 6] = [2.0, 0.5, np.nan, 2.0, 0.5, np.nan]
    u, w, st, h = launch(c, "f64", "f64", obs=obs)
    assert (st[struck] == BAD_OBSTACLE).all()
    assert np.isnan(u[struck]).all() and np.isnan(w[struck]).all()
    rest = np.setdiff1d(np.arange(B), struck)
    for a, b in zip((u, w, st, h), base):
        assert np.array_equal(a[rest], b[rest])
    ref = Q.resolve(c, obs=obs)
    assert np.array_equal(st, ref["status"])


@pytest.mark.parametrize("key", (Q.DU, Q.DPCBF))
def test_outputs_do_not_depend_on_the_position_in_the_batch(key):
    """The batch reversed, and cut to B = 1, 255, 256 and 257 (around the 256-lane block): every agent's outputs are bitwise those of
    its row in the full launch."""
    c = Q.cases(key)
    B = len(c["X"])
    assert B > 257
    base = launch(c, "f64", "f64")
    rev = launch(c, "f64", "f64", idx=np.arange(B)[::-1])
    for a, b in zip(rev, base):
        assert np.array_equal(a[::-1], b)
    for n in (1, 255, 256, 257):
        cut = launch(c, "f64", "f64", idx=np.arange(n))
        for a, b in zip(cut, base):
            assert a.shape[0] == n and np.array_equal(a, b[:n]), n
