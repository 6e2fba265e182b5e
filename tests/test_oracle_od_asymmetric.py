"""CPU: the optimal-decay oracles at UNEQUAL decay parameters.  Every other oracle test runs at the defaults, where the two decay
variables of a pair are interchangeable (omega1 = omega2 = 1, p_sb1 = p_sb2, alpha1 = alpha2): an oracle that mixed up the two, or
that wrote a reference of 1 into a derivative, would pass them -- and would make tests/test_od_asymmetric_gpu.py worthless.  Here, at
two unequal sets per family (one with both references away from 1):

  (a) grad, J and the Lagrangian Hessian W against central differences at a random point with rho away from the references, at the
      tolerances the default-parameter tests of each family use;
  (b) the cost and the CBF rows against a restatement written out from the oracle headers:
      f = stage cost + R u^2 + p_sb1 (rho1 - omega1)^2 + p_sb2 (rho2 - omega2)^2, row = dd_h + (a1 rho1 + a2 rho2) d_h + a1 a2 rho1 rho2 h;
  (c) the Schur and the dense Newton step reaching the same point, whose KKT residual, recomputed here from the problem functions, is
      within the solver's tol;
  (d) oracle/od_cbf_qp.py against scipy SLSQP with penalties of order 1 - 100, so that the decay variables move; the inert omega2 of
      the relative-degree-1 models reported at its reference."""
import numpy as np
import pytest
from scipy.optimize import minimize

from oracle import mpc_cbf as M, mpc_gn as G, mpc_lin as L, ms_ipopt as MS
from oracle import od_cbf_qp as OD, od_mpc_cbf as O, od_mpc_gn as OG, od_mpc_rd1 as O1, od_mpc_vtol as OV, robots as R
from safe_control_amd import workloads as W

# two variables per stage: (gains, references, penalties) all unequal; B has both references on the other side of 1 and the order of every pair reversed
SETS2 = {"A": dict(omega1=0.8, omega2=1.25, p_sb1=3.0, p_sb2=40.0), "B": dict(omega1=1.4, omega2=0.6, p_sb1=25.0, p_sb2=2.0)}
GAINS = {"A": (1.6, 0.5), "B": (0.7, 1.3)}                               # alpha1, alpha2 as multiples of the family's default
SETS1 = {"A": dict(omega1=0.8, p_sb1=3.0), "B": dict(omega1=1.4, p_sb1=25.0)}


def set2(which, a_default):
    return dict(SETS2[which], alpha1=GAINS[which][0] * a_default, alpha2=GAINS[which][1] * a_default)


def fd(fun, x, h=1e-6):
    return np.array([(fun(x + h * e) - fun(x - h * e)) / (2 * h) for e in np.eye(len(x))])


def check_derivatives(ev, nvar, m, rng, tg, tj, tw, rel_grad_floor=0.0):
    """ev(zz, lam, level) -> dict; central differences of f, g and of the Lagrangian gradient."""
    zz, lam = rng
    e2 = ev(zz, lam, 2)
    gfd = fd(lambda v: ev(v, None, 0)["f"], zz)
    Jfd = fd(lambda v: ev(v, None, 0)["g"], zz).T
    assert np.abs(gfd - e2["grad"]).max() <= tg * max(rel_grad_floor, np.abs(gfd).max())
    assert np.abs(Jfd - e2["J"]).max() <= tj * max(1.0, np.abs(Jfd).max())

    def gL(v):
        e = ev(v, None, 1)
        return e["grad"] - e["J"].T @ lam
    Wfd = fd(gL, zz)
    assert np.abs(Wfd - e2["W"]).max() <= tw * max(1.0, np.abs(e2["W"]).max())
    assert np.abs(e2["W"] - e2["W"].T).max() <= 1e-9 * max(1.0, np.abs(e2["W"]).max())


def kkt_residual(ev1, info):
    """max(|sf grad - J' lam|, |g - s|, |s lam|) at the returned point, in the solver's scaling (oracle/od_mpc_cbf.py: solve)."""
    sf, lam, s = info["scale"], info["lam"] * info["scale"], info["s"]
    return max(np.abs(sf * ev1["grad"] - ev1["J"].T @ lam).max(), np.abs(ev1["g"] - s).max(), np.abs(s * lam).max())


# ---- oracle/od_mpc_cbf.py (DynamicUnicycle2D) --------------------------------------------------------------------------------------

def du_case(i, K=8):
    X, goal, _, obs = W.du_cbfqp_batch(16, K, seed=1)
    return X[i], goal[i], obs[i]


@pytest.mark.parametrize("which", ["A", "B"])
def test_du_derivatives_cost_and_rows(which):
    P = dict(O.DEFAULTS, **set2(which, 0.0125))
    x0, goal, obs = du_case(1)
    rng = np.random.default_rng(3)
    zz = np.concatenate([rng.uniform(-0.4, 0.4, 20), rng.uniform(-1.0, 3.0, 20)])
    lam = rng.uniform(0, 2, 140)
    check_derivatives(lambda v, l, lev: O.evaluate(x0, v, goal, obs, P, l, level=lev), 40, 140, (zz, lam), 1e-5, 1e-6, 1e-5)
    # (b) the cost and the rows, written out (oracle/od_mpc_cbf.py header)
    z, rho = zz[:20], zz[20:].reshape(10, 2)
    ev = O.evaluate(x0, zz, goal, obs, P, level=0)
    X, pe = M.rollout(x0, z, P)
    pos = np.vstack([X[:, :2], pe[None]])
    Q, Rw = np.asarray(P["Q"]), np.asarray(P["R"])
    f = 0.0
    for k in range(1, 11):
        f += Q[0] * (pos[k, 0] - goal[0]) ** 2 + Q[1] * (pos[k, 1] - goal[1]) ** 2 + Q[2] * X[k, 2] ** 2 + Q[3] * X[k, 3] ** 2
    f += sum(Rw[i] * z[2 * k + i] ** 2 for k in range(10) for i in range(2))
    f += sum(P["p_sb1"] * (rho[k, 0] - P["omega1"]) ** 2 + P["p_sb2"] * (rho[k, 1] - P["omega2"]) ** 2 for k in range(10))
    assert abs(ev["f"] - f) <= 1e-12 * abs(f)
    a1, a2 = P["alpha1"], P["alpha2"]
    for k in range(10):
        for j in range(8):
            h0, h1, h2 = (M.barrier(pos[k + s], obs[j], P)[0] for s in range(3))
            row = (h2 - 2 * h1 + h0) + (a1 * rho[k, 0] + a2 * rho[k, 1]) * (h1 - h0) + a1 * a2 * rho[k, 0] * rho[k, 1] * h0
            assert abs(ev["g"][k * 8 + j] - row) <= 1e-12 * max(1.0, abs(row))


@pytest.mark.parametrize("which", ["A", "B"])
def test_du_schur_dense_and_kkt(which):
    over = dict(set2(which, 0.0125))
    P = dict(O.DEFAULTS, **over)
    n_moved = 0
    for i in (0, 3, 5):
        x0, goal, obs = du_case(i)
        a = O.solve(x0, np.zeros(2), goal, obs, params=over, return_info=True)
        b = O.solve(x0, np.zeros(2), goal, obs, params=over, return_info=True, linear_algebra="dense")
        assert a[2] == b[2] == O.STATUS_OPTIMAL and abs(a[3] - b[3]) <= 2
        assert np.abs(a[4]["zz"] - b[4]["zz"]).max() < 1e-6
        assert kkt_residual(O.evaluate(x0, a[4]["zz"], goal, a[4]["obs"], P, level=1), a[4]) <= P["tol"]
        n_moved += int(np.abs(a[4]["zz"][20:].reshape(10, 2) - [P["omega1"], P["omega2"]]).max() > 1e-2)
    assert n_moved >= 2


# ---- oracle/od_mpc_gn.py (KinematicBicycle2D, Quad2D) and oracle/od_mpc_vtol.py ------------------------------------------------------

def gn_problem(fam, which, N):
    if fam == "vtol":
        P = OV.params(N=N, **set2(which, 0.35))
        X, up, goal, obs = W.mpc_family_batch("vtol", 8, 4, 0)
        i = 2
        o = obs[i].copy(); o[0, :3] = [X[i, 0] + 6.0, X[i, 1] + 0.4, 1.2]
        return P, P["model"], X[i], up[i], goal[i], o
    mdl = {"kb": OG.kb_model, "quad2d": OG.quad2d_model}[fam]()
    P = OG.params(mdl, N, **set2(which, mdl["alpha1"]))
    X, up, goal, obs = W.mpc_family_batch(fam, 8, 8, 0)
    return P, mdl, X[3], up[3], goal[3], obs[3]


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("fam", ["kb", "quad2d", "vtol"])
def test_gn_derivatives_cost_and_rows(fam, which):
    N = 5 if fam == "vtol" else 10
    P, mdl, x0, up, goal, obs = gn_problem(fam, which, N)
    nu = int(P.get("nu", 2))
    n = nu * N
    rng = np.random.default_rng(4)
    z = rng.uniform(mdl["u_lo"], mdl["u_hi"], (N, nu)).reshape(-1)
    rho = rng.uniform(-0.5, 2.5, (N, 2))
    zz = np.concatenate([z, rho.reshape(-1)])
    ev0 = OG.evaluate(x0, zz, up, goal, obs, P, None, 0)
    lam = rng.uniform(0, 2, ev0["g"].shape[0])
    tol = (1e-6, 1e-6, 2e-6) if fam == "vtol" else (1e-6, 1e-6, 1e-6)
    check_derivatives(lambda v, l, lev: OG.evaluate(x0, v, up, goal, obs, P, l, lev), n + 2 * N, len(lam), (zz, lam), *tol)
    # (b) the decay penalty on top of the model's own cost (R u^2: rterm = "u"), and the rows from the barrier values at the three points
    # of a stage (oracle/mpc_gn.py: hv, pinned on the reference's agent_barrier_dt by the MPCCBF tests)
    base = G.evaluate(x0, z, up, goal, obs, dict(P, stage_w=np.ones((N, 3))), None, 0)
    pen = sum(P["p_sb1"] * (rho[k, 0] - P["omega1"]) ** 2 + P["p_sb2"] * (rho[k, 1] - P["omega2"]) ** 2 for k in range(N))
    assert abs(ev0["f"] - (base["f"] + pen)) <= 1e-12 * abs(ev0["f"])
    hv, K = base["hv"], obs.shape[0]
    a1, a2 = P["alpha1"], P["alpha2"]
    for k in range(N):
        ha, hb, hc = hv[k]
        row = (hc - 2 * hb + ha) + (a1 * rho[k, 0] + a2 * rho[k, 1]) * (hb - ha) + a1 * a2 * rho[k, 0] * rho[k, 1] * ha
        assert np.abs(ev0["g"][k * K:(k + 1) * K] - row).max() <= 1e-12 * max(1.0, np.abs(row).max())


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("fam", ["kb", "quad2d"])
def test_gn_schur_dense_and_kkt(fam, which):
    mdl = {"kb": OG.kb_model, "quad2d": OG.quad2d_model}[fam]()
    mult = {"A": (1.25, 0.8), "B": (0.8, 1.25)}[which] if fam == "kb" else GAINS[which]      # (the bicycle crawls at gains far from its default)
    over = dict(SETS2[which], alpha1=mult[0] * mdl["alpha1"], alpha2=mult[1] * mdl["alpha2"])
    P = OG.params(mdl, 10, **over)
    X, up, goal, obs = W.mpc_family_batch(fam, 8, 8, seed=18)
    n_opt = 0
    for i in (1, 2, 4):
        a = OG.solve(mdl, X[i], up[i], goal[i], obs[i], params_over=over, return_info=True)
        b = OG.solve(mdl, X[i], up[i], goal[i], obs[i], params_over=over, return_info=True, linear_algebra="dense")
        assert a[2] == b[2] and abs(a[3] - b[3]) <= 2
        if a[2] != 0 or a[4]["err"] > P["tol"]:
            continue
        n_opt += 1
        assert np.abs(a[0] - b[0]).max() <= 1e-6 and np.abs(a[1] - b[1]).max() <= 1e-6
        assert kkt_residual(OG.evaluate(X[i], a[4]["zz"], up[i], goal[i], a[4]["obs"], P, None, 1), a[4]) <= P["tol"]
    assert n_opt >= 2


@pytest.mark.parametrize("which", ["A", "B"])
def test_vtol_schur_dense_and_kkt(which):
    N = 10
    over = set2(which, 0.35)
    x0 = np.array([0.0, 10.0, 0.0, 12.0, 0.0, 0.0]); goal = np.array([100.0, 10.0])
    obs = np.zeros((2, 7)); obs[0, :3] = [9.5 if which == "A" else 12.0, 10.3, 1.5]; obs[1, :3] = [500.0, 10.0, 1.0]     # (set B leaves no feasible point at 9.5 m)
    a = OV.solve(x0, np.zeros(4), goal, obs, N=N, params_over=over, return_info=True)
    b = OV.solve(x0, np.zeros(4), goal, obs, N=N, params_over=over, return_info=True, linear_algebra="dense")
    assert a[2] == b[2] == 0 and abs(a[3] - b[3]) <= 2
    assert np.abs(a[0] - b[0]).max() <= 1e-6 and np.abs(a[4]["zz"] - b[4]["zz"]).max() <= 1e-5
    P = OV.params(N=N, **over)
    assert kkt_residual(OG.evaluate(x0, a[4]["zz"], np.zeros(4), goal, a[4]["obs"], P, None, 1), a[4]) <= P["tol"]
    assert np.abs(a[4]["zz"][4 * N:].reshape(N, 2) - [P["omega1"], P["omega2"]]).max() > 1e-2


# ---- oracle/od_mpc_rd1.py (Unicycle2D, Quad3D: one decay variable) -------------------------------------------------------------------

def rd1_case(kind, which, seed=1):
    from test_oracle_od_rd1 import quad_case, uni_case
    if kind == "uni":
        x0, goal, obs, _ = uni_case(seed)
        return x0, goal, obs, O1.uni_params(N=6, alpha=(0.08 if which == "A" else 0.035), **SETS1[which])
    x0, goal, obs, _ = quad_case(seed)
    return x0, goal, obs, O1.lin_params(dict(L.quad3d_model(), circles_only=False), N=5, alpha=(0.24 if which == "A" else 0.1), **SETS1[which])


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("kind", ["uni", "quad3d"])
def test_rd1_derivatives_cost_and_rows(kind, which):
    x0, goal, obs, P = rd1_case(kind, which)
    N, nu = P["N"], P.get("nu", 2)
    n = N * nu
    rng = np.random.default_rng(5)
    lo = P["u_lo"] if "u_lo" in P else -np.array([P["a_max"], P["w_max"]])
    hi = P["u_hi"] if "u_hi" in P else np.array([P["a_max"], P["w_max"]])
    z = rng.uniform(np.tile(lo, N) * 0.3, np.tile(hi, N) * 0.3)
    rho = rng.uniform(-0.5, 2.5, N)
    zz = np.concatenate([z, rho])
    ev0 = O1.evaluate(x0, zz, goal, obs, P, level=0)
    lam = rng.uniform(0, 2, ev0["g"].shape[0])
    check_derivatives(lambda v, l, lev: O1.evaluate(x0, v, goal, obs, P, l, level=lev), n + N, len(lam), (zz, lam), 1e-5, 1e-5, 2e-5, rel_grad_floor=1.0)
    # (b) f = the model's cost with R u^2 + p_sb1 sum (rho_k - omega1)^2; row = d_h + alpha rho_k h_k: the rows at rho = 0 are d_h alone
    free = O1.evaluate(x0, np.concatenate([z, np.zeros(N)]), goal, obs, dict(P, p_sb1=0.0), level=1)
    assert abs(ev0["f"] - (free["f"] + P["p_sb1"] * np.sum((rho - P["omega1"]) ** 2))) <= 1e-12 * abs(ev0["f"])
    K = obs.shape[0]
    for k in range(N):
        row = free["g"][k * K:(k + 1) * K] + P["alpha"] * rho[k] * free["ha"][k]
        assert np.abs(ev0["g"][k * K:(k + 1) * K] - row).max() <= 1e-12 * max(1.0, np.abs(row).max())


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("kind", ["uni", "quad3d"])
def test_rd1_schur_dense_and_kkt(kind, which):
    n_opt = 0
    for seed in (10, 11, 12):
        x0, goal, obs, P = rd1_case(kind, which, seed)
        up = np.zeros(P.get("nu", 2))
        a = O1.solve(x0, up, goal, obs, P, return_info=True)
        b = O1.solve(x0, up, goal, obs, P, return_info=True, linear_algebra="dense")
        assert a[2] == b[2]
        if a[2] != 0 or a[4]["err"] > P["tol"]:
            continue
        n_opt += 1
        assert np.abs(a[4]["zz"] - b[4]["zz"]).max() <= 1e-7
        assert kkt_residual(O1.evaluate(x0, a[4]["zz"], goal, a[4]["obs"], P, level=1), a[4]) <= P["tol"]
    assert n_opt >= 2


# ---- oracle/ms_ipopt.py: vtol_od_model ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["A", "B"])
def test_ms_vtol_od_model_derivatives_and_cost(which):
    p = set2(which, 0.35)
    mdl = MS.vtol_od_model()
    mdl.update(alpha1=p["alpha1"], alpha2=p["alpha2"], od=dict(omega_ref=np.array([p["omega1"], p["omega2"]]), p_sb=np.array([p["p_sb1"], p["p_sb2"]])))
    N = 3
    x0 = np.array([0.0, 10.0, 0.02, 12.0, 0.1, 0.0]); goal = np.array([100.0, 10.0])
    obs = np.zeros((2, 7)); obs[0, :3] = [9.5, 10.3, 1.5]; obs[1, :3] = [20.0, 9.0, 1.0]
    nlp = MS.StageNLP(mdl, x0, np.zeros(4), goal, obs, N=N)
    rng = np.random.default_rng(6)
    w = nlp.initial_guess() + rng.uniform(-0.05, 0.05, nlp.n)
    w[nlp.iu[:, 4:]] = rng.uniform(-0.5, 2.5, (N, 2))
    ev = nlp.evaluate(w, 2)
    gfd = fd(lambda v: nlp.evaluate(v, 0)["f"], w)
    Jc = fd(lambda v: nlp.evaluate(v, 0)["c"], w).T
    Jd = fd(lambda v: nlp.evaluate(v, 0)["d"], w).T
    assert np.abs(gfd - ev["grad"]).max() <= 1e-5 * np.abs(gfd).max()
    assert np.abs(Jc - ev["Jc"]).max() <= 1e-6 * max(1.0, np.abs(Jc).max()) and np.abs(Jd - ev["Jd"]).max() <= 1e-6 * max(1.0, np.abs(Jd).max())
    yc, yd = rng.uniform(-1, 1, nlp.m_c), rng.uniform(0, 2, nlp.m_d)

    def gL(v):
        e = nlp.evaluate(v, 2)
        return e["grad"] + e["Jc"].T @ yc + e["Jd"].T @ yd
    Wfd = fd(gL, w)
    Wh = ev["hess"](1.0, yc, yd)
    assert np.abs(Wfd - Wh).max() <= 1e-5 * max(1.0, np.abs(Wh).max())
    # the cost: the plain model's state term + R u^2 + the decay penalties; the rows: the plain model's with the stage's gains
    X, U = nlp.split(w)
    e = X - nlp.xg
    f = np.sum(mdl["Q"] * e * e) + np.sum(mdl["R"][:4] * U[:, :4] ** 2) + np.sum(p["p_sb1"] * (U[:, 4] - p["omega1"]) ** 2 + p["p_sb2"] * (U[:, 5] - p["omega2"]) ** 2)
    assert abs(ev["f"] - f) <= 1e-12 * abs(f)
    d = nlp.evaluate(w, 0)["d"].reshape(N, 2)
    for k in range(N):
        plain = dict(MS.vtol_model(), alpha1=p["alpha1"] * U[k, 4], alpha2=p["alpha2"] * U[k, 5])     # a1 rho1 + a2 rho2 and a1 a2 rho1 rho2 as fixed gains
        q = MS.StageNLP(plain, x0, np.zeros(4), goal, obs, N=N)
        wq = np.zeros(q.n); wq[q.ix] = X; wq[q.iu] = U[:, :4]
        assert np.abs(q.evaluate(wq, 0)["d"].reshape(N, 2)[k] - d[k]).max() <= 1e-12 * max(1.0, np.abs(d[k]).max())


@pytest.mark.parametrize("which", ["A", "B"])
def test_ms_vtol_od_model_solve_agrees_with_the_condensed_oracle(which):
    """Part (c) for the multiple-shooting statement: at unequal parameters oracle/ms_ipopt.py (states as variables, IPOPT's filter method)
    and oracle/od_mpc_vtol.py (condensed, the merit-function method pinned above by its KKT residual) are two statements and two
    algorithms for ONE problem: same status, same cost, same inputs.  Bars: the condensed solve ends at a KKT residual
    of tol = 1e-6 in a cost scaled by sf (info["scale"], gradients of 100), that is a gradient residual of tol / sf in the cost as
    stated; a variable whose own curvature is c = 2 R_i or 2 p_sb_i is then determined to tol / (sf c), which is the bar on the plan
    (the multiple-shooting solve ends at 1e-8 and adds nothing to it); the cost to 1e-7 relative."""
    N = 10
    p = set2(which, 0.35)
    x0 = np.array([0.0, 10.0, 0.0, 12.0, 0.0, 0.0]); goal = np.array([100.0, 10.0])
    obs = np.zeros((2, 7)); obs[0, :3] = [12.0, 10.3, 1.5]; obs[1, :3] = [500.0, 10.0, 1.0]
    mdl = MS.vtol_od_model()
    mdl.update(alpha1=p["alpha1"], alpha2=p["alpha2"], od=dict(omega_ref=np.array([p["omega1"], p["omega2"]]), p_sb=np.array([p["p_sb1"], p["p_sb2"]])))
    um, sm, im, info = MS.solve(mdl, x0, np.zeros(4), goal, obs, N=N, return_info=True, opts=dict(MS.KERNEL_PROFILE))
    uc, rc, sc, ic, ic_info = OV.solve(x0, np.zeros(4), goal, obs, N=N, params_over=p, return_info=True)
    assert sm == sc == 0
    f0 = float(np.sum(mdl["Q"] * (x0 - np.concatenate([goal, np.zeros(4)])) ** 2))      # the cost of stage 0, a constant the condensed statement leaves out
    assert abs(info["f"] - f0 - ic_info["f"]) <= 1e-7 * abs(ic_info["f"])
    bar = 1e-6 / (ic_info["scale"] * 2.0 * min(0.5, p["p_sb1"], p["p_sb2"]))
    print(f"ms against condensed, set {which}: bar {bar:.2e}, inputs {np.abs(info['U'][:, :4].reshape(-1) - ic_info['zz'][: 4 * N]).max():.2e}, "
          f"decay rates {np.abs(info['U'][:, 4:].reshape(-1) - ic_info['zz'][4 * N:]).max():.2e}")
    assert np.abs(info["U"][:, :4].reshape(-1) - ic_info["zz"][: 4 * N]).max() <= bar
    # (the decay rates are printed, not held: on a stage with an active row the cross term -a1 a2 lam h takes the curvature of one
    # combination of the two rates far below 2 p_sb, so the bar above does not apply to them -- set B: 2.1e-4 on one stage at costs
    # equal to 2e-11 relative)
    assert np.abs(info["U"][:, 4:] - [p["omega1"], p["omega2"]]).max() > 1e-2


# ---- oracle/od_cbf_qp.py -----------------------------------------------------------------------------------------------------------

QP2 = [dict(alpha1=0.8, alpha2=0.3, omega1=0.8, omega2=1.25, p_sb1=3.0, p_sb2=40.0), dict(alpha1=0.2, alpha2=0.9, omega1=1.4, omega2=0.6, p_sb1=80.0, p_sb2=1.5)]
QP1 = [dict(alpha=0.8, omega1=0.8, p_sb1=3.0, omega2=1.25), dict(alpha=0.9, omega1=1.4, p_sb1=1.5, omega2=0.6)]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("model", [R.MODEL_DU, R.MODEL_KB_C3BF, R.MODEL_QUAD2D])
def test_od_cbf_qp_enumerator_agrees_with_slsqp(model, which):
    """tests/test_oracle_od.py::test_enumerator_agrees_with_slsqp at unequal alpha, omega and p_sb."""
    from oracle.cbf_qp import input_bounds
    n = 48
    if model == R.MODEL_DU:
        X, goal, ur, obs = W.du_cbfqp_batch(n, 2, seed=2)
        spec = R.default_spec(model); spec.update(a_max=1.0, w_max=0.5)
    elif model == R.MODEL_QUAD2D:
        Xd, goal, _, obs = W.du_cbfqp_batch(n, 2, seed=2)
        rng = np.random.default_rng(9)
        X = np.zeros((n, 6)); X[:, :2] = Xd[:, :2]; X[:, 2] = rng.uniform(-0.4, 0.4, n); X[:, 3:5] = rng.uniform(-1.5, 1.5, (n, 2))
        ur = rng.uniform(2.0, 11.0, (n, 2))
        spec = R.default_spec(model)
    else:
        X, goal, ur, obs = W.kb_c3bf_batch(n, 2, seed=2)
        spec = R.default_spec(model)
    rel2 = model in R.REL_DEG2
    p = (QP2 if rel2 else QP1)[which]
    lo, hi = input_bounds(model, spec)
    worst, n_skip, n_moved = 0.0, 0, 0
    for i in range(n):
        uref = ur[i] * (3.0 if i % 3 == 0 else 1.0)
        r = OD.solve(model, X[i], uref, obs[i, 0], spec, param=p)
        assert r["status"] == 0
        fx, gx = R.f(model, X[i], spec), R.g(model, X[i], spec)
        if rel2:
            h, hdot, d = R.agent_barrier(model, X[i], obs[i, 0], spec["radius"])
            A, b = d @ gx, d @ fx
            rr = np.array([uref[0], uref[1], p["omega1"], p["omega2"]]); D = np.array([1, 1, p["p_sb1"], p["p_sb2"]])
            con = lambda x: np.array([A @ x[:2] + b + (p["alpha1"] + p["alpha2"]) * hdot * x[2] + p["alpha1"] * p["alpha2"] * h * x[3],     # noqa: E731
                                      x[0] - lo[0], hi[0] - x[0], x[1] - lo[1], hi[1] - x[1]])
        else:
            h, d = R.agent_barrier(model, X[i], obs[i, 0], spec["radius"])
            A, b = d @ gx, d @ fx
            rr = np.array([uref[0], uref[1], p["omega1"]]); D = np.array([1, 1, p["p_sb1"]])
            con = lambda x: np.array([A @ x[:2] + b + p["alpha"] * h * x[2], x[0] - lo[0], hi[0] - x[0], x[1] - lo[1], hi[1] - x[1]])     # noqa: E731
            assert r["omega"][1] == p["omega2"]                 # the inert variable: at its reference
        s = minimize(lambda x: np.sum(D * (x - rr) ** 2), rr.copy(), constraints=[{"type": "ineq", "fun": con}],
                     method="SLSQP", options={"ftol": 1e-15, "maxiter": 500})
        if con(s.x).min() < -1e-9:                              # SLSQP gave up at an infeasible point (1e-9, not the 1e-7 of test_oracle_od.py: with
            # references three times the box |grad f| is of order 50, and a violation of 1e-7 would buy more cost than the 1e-7 of the bar below)
            n_skip += 1
            continue
        got = np.concatenate([r["u"], r["omega"]])[: len(D)]
        worst = max(worst, np.abs(s.x - got).max())
        assert np.sum(D * (got - rr) ** 2) <= s.fun + 1e-7
        n_moved += int(np.abs(got[2:] - rr[2:]).max() > 1e-2)
    assert worst < 5e-6 and n_skip <= 6
    assert n_moved >= 4, "with penalties of order 1 - 100 the decay variables must move where the row is active"


def test_od_cbf_qp_inert_omega2_is_reported_at_its_reference():
    X, goal, ur, obs = W.kb_c3bf_batch(4, 1, seed=2)
    spec = R.default_spec(R.MODEL_KB_C3BF)
    for i in range(4):
        assert OD.solve(R.MODEL_KB_C3BF, X[i], ur[i], obs[i, 0], spec, param=dict(omega2=0.7))["omega"][1] == 0.7
        assert OD.solve(R.MODEL_KB_C3BF, X[i], ur[i], obs[i, 0], spec)["omega"][1] == 1.0
    assert OD.solve(R.MODEL_KB_C3BF, X[0], ur[0], None, spec, param=dict(omega1=0.8, omega2=0.7))["omega"].tolist() == [0.8, 0.7]
