"""Runs the numpy MPC oracle over a whole batch on the host cores: plain child processes (``python tests/_oracle_pool.py
in.npz out.npz``), one slice of the batch each, so nothing depends on fork/spawn semantics of a parent that may hold a HIP
context.  At most MAX_WORKERS of them at a time.  Test infrastructure only."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_WORKERS = 16                    # worker processes per batch, by default and at most
TRACE_ROWS = 16                     # iterate-trace rows kept per multiple-shooting solve


# ---- oracle/ms_ipopt.py (kernels 12 and 13) -----------------------------------------------------------------------------------
MS_FAMILIES = {"du": "DynamicUnicycle2D", "uni": "Unicycle2D", "di": "DoubleIntegrator2D", "si": "SingleIntegrator2D",
               "kb": "KinematicBicycle2D", "vtol": "VTOL2D", "vtol_od": "VTOL2D"}


def ms_model(family, spec=None, od=None, alpha1=None, alpha2=None):
    """The oracle model of `family` built from the completed robot_spec the kernel gets (safe_control_amd.robots.spec), not from the
    model's own defaults: every limit and radius is the host class's.  `od` = dict(omega_ref=(w1, w2), p_sb=(p1, p2)) and the two gains
    replace those of the optimal-decay model ("vtol_od")."""
    from oracle import ms_ipopt as MS
    from safe_control_amd.robots.spec import complete_robot_spec
    mk = {"du": MS.du_model, "uni": MS.uni_model, "di": MS.di_model, "si": MS.si_model, "kb": MS.kb_model,
          "vtol": MS.vtol_model, "vtol_od": MS.vtol_od_model}[family]
    sp = complete_robot_spec(dict(spec or {}, model=MS_FAMILIES[family]))
    keys = mk()["spec"].keys()
    mdl = mk({k: v for k, v in sp.items() if k in keys})
    if od is not None:
        mdl["od"] = dict(omega_ref=np.asarray(od["omega_ref"], dtype=np.float64), p_sb=np.asarray(od["p_sb"], dtype=np.float64))
    if alpha1 is not None:
        mdl["alpha1"] = float(alpha1)
    if alpha2 is not None:
        mdl["alpha2"] = float(alpha2)
    return mdl


def _worker_ms(d, outp):
    """kind = "ms:<family>": oracle.ms_ipopt.solve with params dict(opts=<profile>, N=<horizon or None>, spec=<robot_spec>, od=<decay
    references and penalties or None>, alpha1, alpha2); per row
    u, st, it, plan (X then U, flattened), exit (index into ms_ipopt.EXITS), filter_peak, resto (restoration phases entered),
    resto_iters, f, and the first TRACE_ROWS rows of the iterate trace [E0, dinf, pinf, comp, mu, theta, delta_w, alpha] (NaN past
    the end; ntr rows in all; the restoration's rows carry -alpha and resto_row = 1)."""
    from oracle import ms_ipopt as MS
    fam = str(d["kind"])[3:]
    X, up, goal, obs = d["X"], d["up"], d["goal"], d["obs"]
    prm = d["params"].item() if "params" in d.files else {}
    prm = dict(prm or {})
    mdl = ms_model(fam, prm.get("spec"), prm.get("od"), prm.get("alpha1"), prm.get("alpha2"))
    opts, N = dict(prm.get("opts") or MS.KERNEL_PROFILE), prm.get("N")
    B = X.shape[0]
    out = {k: [] for k in ("u", "st", "it", "plan", "exit", "filter_peak", "resto", "resto_iters", "f", "trace", "resto_row", "ntr")}
    for i in range(B):
        tr = []
        u, st, it, info = MS.solve(mdl, X[i], up[i], goal[i], obs[i] if obs.ndim == 3 else obs, N=N, return_info=True, opts=opts, trace=tr)
        T = np.full((TRACE_ROWS, 8), np.nan)
        rr = np.zeros(TRACE_ROWS, dtype=np.int64)
        for j, q in enumerate(tr[:TRACE_ROWS]):
            T[j] = [q["E0"], q["dinf"], q["pinf"], q["comp"], q["mu"], q["theta"], q["delta"], -q["alpha"] if q["resto"] else q["alpha"]]
            rr[j] = int(q["resto"])
        for k, v in (("u", u), ("st", st), ("it", it), ("plan", np.concatenate([info["X"].reshape(-1), info["U"].reshape(-1)])),
                     ("exit", MS.EXITS.index(info["exit"])), ("filter_peak", info["filter_peak"]), ("resto", info["n_resto"]),
                     ("resto_iters", info["resto_iters"]), ("f", info["f"]), ("trace", T), ("resto_row", rr), ("ntr", len(tr))):
            out[k].append(v)
    np.savez(outp, **{k: np.array(v) for k, v in out.items()})


def ms_solve_many(family, X, up, goal, obs, opts=None, N=None, spec=None, workers=None, timeout=1800, od=None, alpha1=None, alpha2=None):
    """oracle.ms_ipopt.solve with the model of `family` (ms_model) on every row (obs [B,K,7] or one shared [K,7] table); dict of
    arrays, see _worker_ms; exit as the names of ms_ipopt.EXITS."""
    from oracle import ms_ipopt as MS
    B = X.shape[0]
    ob = obs if obs.ndim == 3 else np.broadcast_to(obs, (B,) + obs.shape)
    r = _run(dict(kind=np.array("ms:" + family)), X, up, goal, np.ascontiguousarray(ob),
             dict(opts=opts, N=N, spec=spec, od=od, alpha1=alpha1, alpha2=alpha2), workers, timeout)
    r["exit"] = np.array(MS.EXITS)[r["exit"]]
    return r


_CACHE = {}


def _key(family, tag, opts, N, spec):
    from oracle import ms_ipopt as MS
    mdl = ms_model(family, spec)                                  # (the model's numbers: two ways of writing one robot_spec share a run)
    return (family, json.dumps(tag, sort_keys=True), json.dumps(dict(opts or MS.KERNEL_PROFILE), sort_keys=True), N,
            json.dumps(mdl["spec"], sort_keys=True, default=repr))


def ms_cached(family, tag, X, up, goal, obs, opts=None, N=None, spec=None):
    """ms_solve_many, solved once per test session for each (family, tag, options): `tag` names the inputs (the generator, its seed
    and batch size), so that every test that reads the same problems reads one oracle run."""
    k = _key(family, tag, opts, N, spec)
    if k not in _CACHE:
        _CACHE[k] = ms_solve_many(family, X, up, goal, obs, opts=opts, N=N, spec=spec)
    return _CACHE[k]


def ms_batch(family, seed=0, B=4096, K=8, opts=None, N=None, spec=None):
    """workloads.mpc_family_batch(family, B, K, seed) and the oracle's solve of every problem of it (cached per session):
    ((X, up, goal, obs), dict of arrays)."""
    from safe_control_amd import workloads as W
    X, up, goal, obs = W.mpc_family_batch(family, B, K, seed=seed)
    return (X, up, goal, obs), ms_cached(family, ("mpc_family_batch", seed, B, K), X, up, goal, obs, opts=opts, N=N, spec=spec)


def mixed_scene(fam, n, seed=3):
    """The first n problems of the seed-0 bench batch of `fam` with ~60 % of their obstacle rows replaced by superellipsoids."""
    from safe_control_amd import workloads as W
    X, up, goal, obs = (a[:n].copy() for a in W.mpc_family_batch(fam, 4096, 8, seed=0))
    se = W.superellipsoid_obstacles(X[:, :2], 8, seed=seed, radius=0.25, rho_max=2.5)
    mix = np.random.default_rng(1).random((n, 8)) < 0.6
    obs[mix] = se[mix]
    return X, up, goal, obs


def take(res, idx):
    """Rows `idx` of a result dict."""
    return {k: v[idx] for k, v in res.items()}


def _worker_od_rd1(d, outp):
    """kind = "od_uni" | "od_quad3d": oracle.od_mpc_rd1.solve (the config-5 extension)."""
    from oracle import mpc_lin as L, od_mpc_rd1 as O
    X, up, goal, obs = d["X"], d["up"], d["goal"], d["obs"]
    over = d["params"].item() if "params" in d.files else {}
    N = over.get("N", 10)
    if str(d["kind"]) == "od_uni":
        P = O.uni_params(**over)
        nu = 2
    else:
        over = dict(over); over.pop("N", None)
        P = O.lin_params(dict(L.quad3d_model(), circles_only=False), N=N, **over)
        nu = 4
    B = X.shape[0]
    u = np.zeros((B, nu)); st = np.zeros(B, dtype=np.int64); it = np.zeros(B, dtype=np.int64)
    z = np.zeros((B, nu * N)); rho = np.zeros((B, N)); f = np.zeros(B)
    for i in range(B):
        u[i], _, st[i], it[i], info = O.solve(X[i], up[i], goal[i], obs[i], P, return_info=True)
        z[i], rho[i], f[i] = info["z"], info["rho"], info["f"]
    np.savez(outp, u=u, st=st, it=it, z=z, rho=rho, f=f)


def _worker_od_du(d, outp):
    """kind = "od_du": oracle.od_mpc_cbf.solve (DynamicUnicycle2D); params = overrides of its DEFAULTS (N, alpha1, .., p_sb2)."""
    from oracle import od_mpc_cbf as O
    X, up, goal, obs = d["X"], d["up"], d["goal"], d["obs"]
    over = dict((d["params"].item() if "params" in d.files else {}) or {})
    N = over.get("N", O.DEFAULTS["N"])
    B = X.shape[0]
    u = np.zeros((B, 2)); st = np.zeros(B, dtype=np.int64); it = np.zeros(B, dtype=np.int64)
    z = np.zeros((B, 2 * N)); rho = np.zeros((B, 2 * N)); f = np.zeros(B); err = np.zeros(B)
    for i in range(B):
        u[i], _, st[i], it[i], info = O.solve(X[i], up[i], goal[i], obs[i], params=over, return_info=True)
        z[i], rho[i], f[i], err[i] = info["zz"][: 2 * N], info["zz"][2 * N:], info["f"], info["err"]
    np.savez(outp, u=u, st=st, it=it, z=z, rho=rho, f=f, err=err)


def _worker_od_gn(d, outp):
    """kind = "od_gn:kb" | "od_gn:quad2d": oracle.od_mpc_gn.solve; params = N and overrides of od_mpc_gn.params (alpha1, .., p_sb2)."""
    from oracle import od_mpc_gn as OG
    mdl = {"kb": OG.kb_model, "quad2d": OG.quad2d_model}[str(d["kind"])[6:]]()
    X, up, goal, obs = d["X"], d["up"], d["goal"], d["obs"]
    over = dict((d["params"].item() if "params" in d.files else {}) or {})
    N = over.pop("N", 10)
    B = X.shape[0]
    u = np.zeros((B, 2)); st = np.zeros(B, dtype=np.int64); it = np.zeros(B, dtype=np.int64)
    z = np.zeros((B, 2 * N)); rho = np.zeros((B, 2 * N)); f = np.zeros(B); err = np.zeros(B)
    for i in range(B):
        u[i], _, st[i], it[i], info = OG.solve(mdl, X[i], up[i], goal[i], obs[i], N=N, params_over=over, return_info=True)
        z[i], rho[i], f[i], err[i] = info["zz"][: 2 * N], info["zz"][2 * N:], info["f"], info["err"]
    np.savez(outp, u=u, st=st, it=it, z=z, rho=rho, f=f, err=err)


def od_du_solve_many(X, up, goal, obs, params=None, workers=None, timeout=1800):
    """oracle.od_mpc_cbf.solve on every row; dict(u, st, it, z, rho (omega1_k, omega2_k per stage), f, err)."""
    return _run(dict(kind=np.array("od_du")), X, up, goal, obs, params, workers, timeout)


def od_gn_solve_many(family, X, up, goal, obs, params=None, workers=None, timeout=1800):
    """oracle.od_mpc_gn.solve with the model of `family` ("kb" | "quad2d") on every row; dict(u, st, it, z, rho, f, err)."""
    return _run(dict(kind=np.array("od_gn:" + family)), X, up, goal, obs, params, workers, timeout)


def _worker_od_vtol(d, outp):
    """kind = "odvtol": oracle.od_mpc_vtol.solve (optimal-decay MPC-CBF of VTOL2D); zz = [u (4 N) | rho (2 N)]."""
    from oracle import od_mpc_vtol as OV
    X, up, goal, obs = d["X"], d["up"], d["goal"], d["obs"]
    over = d["params"].item() if "params" in d.files else {}
    over = dict(over or {})
    N = over.pop("N", 30)
    B = X.shape[0]
    u = np.zeros((B, 4)); st = np.zeros(B, dtype=np.int64); it = np.zeros(B, dtype=np.int64)
    z = np.zeros((B, 4 * N)); rho = np.zeros((B, 2 * N)); f = np.zeros(B); gmin = np.zeros(B); err = np.zeros(B); lam = np.zeros(B)
    for i in range(B):
        u[i], _, st[i], it[i], info = OV.solve(X[i], up[i], goal[i], obs[i], N=N, params_over=over, return_info=True)
        z[i], rho[i], f[i], gmin[i], err[i], lam[i] = info["zz"][: 4 * N], info["zz"][4 * N:], info["f"], info["g"].min(), info["err"], info["lam"].max()
    np.savez(outp, u=u, st=st, it=it, z=z, rho=rho, f=f, gmin=gmin, err=err, lam=lam)


def od_vtol_solve_many(X, up, goal, obs, params=None, workers=None, timeout=1800):
    """oracle.od_mpc_vtol.solve on every row; dict(u, st, it, z, rho, f, gmin, err, lam)."""
    return _run(dict(kind=np.array("odvtol")), X, up, goal, obs, params, workers, timeout)


def family_problem(family, N=10, over=None):
    """(params, evaluate function) of one model family of workloads.MPC_FAMILIES for oracle.mpc_cbf.solve."""
    from oracle import mpc_cbf as M, mpc_gn as G, mpc_kb_state as S, mpc_lin as L
    over = dict(over or {})
    if family == "du":
        P = dict(M.DEFAULTS, N=N); P.update(over); return P, M.evaluate
    if family in ("kb", "di", "quad2d"):
        mdl = {"kb": G.kb_model, "di": G.di_model, "quad2d": G.quad2d_model}[family]()
        return G.params(mdl, N, **over), G.evaluate
    if family == "vtol":
        from oracle import mpc_vtol as V
        return V.params(N=30 if N == 10 else N, **over), G.evaluate      # the reference's VTOL2D horizon is 30
    if family in ("c3bf", "dpcbf"):
        mdl = S.c3bf_model() if family == "c3bf" else S.dpcbf_model()
        P = S.params(mdl, N, **over); P["model"] = dict(mdl, circles_only=True); return P, S.evaluate
    mdl = L.quad3d_model() if family == "quad3d" else L.si_model()
    return L.params(mdl, N, **over), L.evaluate


def _worker_family(d, outp):
    """kind = "fam:<family>": the shared solver with that family's problem functions; also records the l1 violation of the CBF
    rows at the returned point and how often the restoration was entered."""
    from oracle import mpc_cbf as M
    fam = str(d["kind"])[4:]
    X, up, goal, obs = d["X"], d["up"], d["goal"], d["obs"]
    over = d["params"].item() if "params" in d.files else {}
    N = over.pop("N", 30 if fam == "vtol" else 10) if isinstance(over, dict) else 10
    B = X.shape[0]
    nu = up.shape[1]
    u = np.zeros((B, nu)); st = np.zeros(B, dtype=np.int64); it = np.zeros(B, dtype=np.int64); z = np.zeros((B, nu * N))
    theta = np.zeros(B); nr = np.zeros(B, dtype=np.int64); err = np.zeros(B); stalled = np.zeros(B, dtype=np.int64)
    for i in range(B):
        P, ev = family_problem(fam, N, over)
        u[i], st[i], it[i], info = M.solve(X[i], up[i], goal[i], obs[i], params=P, return_info=True, evaluate_fn=ev)
        z[i], theta[i], nr[i], err[i], stalled[i] = info["z"], info["theta"], info["n_resto"], info["err"], info.get("stalled", 0)
    np.savez(outp, u=u, st=st, it=it, z=z, theta=theta, n_resto=nr, err=err, stalled=stalled)


def _worker_phase1(d, outp):
    """kind = "p1:<family>": an independent feasibility search (tests/test_oracle_mpc_resto.py: phase_one) from the plan `z` a solver
    returned: best min_i g_i over the CBF rows it reaches."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_oracle_mpc_resto import phase_one
    fam = str(d["kind"])[3:]
    X, up, goal, obs, Z = d["X"], d["up"], d["goal"], d["obs"], d["z"]
    over = d["params"].item() if "params" in d.files else {}
    starts = int((over or {}).get("starts", 8))
    best = np.zeros(X.shape[0])
    for i in range(X.shape[0]):
        P, ev = family_problem(fam, 10, {})
        info = dict(z=Z[i], obs=obs[i])
        best[i] = phase_one(X[i], up[i], goal[i], P, ev, info, starts=starts)
    np.savez(outp, best=best)


def phase_one_many(family, X, up, goal, obs, z, starts=8, workers=None, timeout=3000):
    """phase_one on every row, from the plans `z`; returns best min g per row."""
    return _run(dict(kind=np.array("p1:" + family), z=z), X, up, goal, obs, dict(starts=starts), workers, timeout)["best"]


def family_solve_many(family, X, up, goal, obs, params=None, workers=None, timeout=1800):
    """oracle.mpc_cbf.solve with the problem functions of `family` on every row; dict(u, st, it, z, theta, n_resto, err, stalled)."""
    return _run(dict(kind=np.array("fam:" + family)), X, up, goal, obs, params, workers, timeout)


def _worker(inp, outp):
    sys.path.insert(0, ROOT)
    from oracle import mpc_cbf as M
    d = np.load(inp, allow_pickle=True)
    if "kind" in d.files and str(d["kind"]) == "odvtol":
        return _worker_od_vtol(d, outp)
    if "kind" in d.files and str(d["kind"]) == "od_du":
        return _worker_od_du(d, outp)
    if "kind" in d.files and str(d["kind"]).startswith("od_gn:"):
        return _worker_od_gn(d, outp)
    if "kind" in d.files and str(d["kind"]) in ("od_uni", "od_quad3d"):
        return _worker_od_rd1(d, outp)
    if "kind" in d.files and str(d["kind"]).startswith("od_"):
        raise ValueError(f"unknown optimal-decay oracle kind {d['kind']}")
    if "kind" in d.files and str(d["kind"]).startswith("p1:"):
        return _worker_phase1(d, outp)
    if "kind" in d.files and str(d["kind"]).startswith("fam:"):
        return _worker_family(d, outp)
    if "kind" in d.files and str(d["kind"]).startswith("ms:"):
        return _worker_ms(d, outp)
    X, up, goal, obs = d["X"], d["up"], d["goal"], d["obs"]
    params = d["params"].item() if "params" in d.files else None
    B = X.shape[0]
    N = (params or {}).get("N", M.DEFAULTS["N"])
    u = np.zeros((B, 2)); st = np.zeros(B, dtype=np.int64); it = np.zeros(B, dtype=np.int64); z = np.zeros((B, 2 * N)); f = np.zeros(B)
    for i in range(B):
        u[i], st[i], it[i], info = M.solve(X[i], up[i], goal[i], obs[i], params=params, return_info=True)
        z[i], f[i] = info["z"], info["f"]
    np.savez(outp, u=u, st=st, it=it, z=z, f=f)


def od_rd1_solve_many(kind, X, up, goal, obs, params=None, workers=None, timeout=1800):
    """oracle.od_mpc_rd1.solve on every row (kind "od_uni" | "od_quad3d"); returns dict(u, st, it, z, rho, f)."""
    return _run(dict(kind=np.array(kind)), X, up, goal, obs, params, workers, timeout)


def mpc_cbf_solve_many(X, up, goal, obs, params=None, workers=None, timeout=900):
    """oracle.mpc_cbf.solve on every row; returns (u0[B,2], status[B], iters[B], z[B,n], f[B])."""
    r = _run({}, X, up, goal, obs, params, workers, timeout)
    return r["u"], r["st"], r["it"], r["z"], r["f"]


def concurrently(jobs):
    """Several *_solve_many calls at once, MAX_WORKERS child processes between them: jobs = [(function, args, kwargs), ...]; their
    results in that order.  (One oracle run per parameter set of a batch: the runs are short and a batch of 32 fills few workers.)  The cap
    of MAX_WORKERS processes holds as long as no two calls of this function overlap: call it from one thread only."""
    from concurrent.futures import ThreadPoolExecutor
    w = max(1, MAX_WORKERS // len(jobs))
    with ThreadPoolExecutor(len(jobs)) as ex:
        futs = [ex.submit(fn, *a, **dict(kw, workers=w)) for fn, a, kw in jobs]
        return [f.result() for f in futs]


def _run(extra, X, up, goal, obs, params, workers, timeout):
    B = X.shape[0]
    workers = max(1, min(workers or MAX_WORKERS, MAX_WORKERS, os.cpu_count() or 2, B))
    edges = np.linspace(0, B, workers + 1).astype(int)
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for w in range(workers):
            a, b = edges[w], edges[w + 1]
            inp, outp = os.path.join(tmp, f"in{w}.npz"), os.path.join(tmp, f"out{w}.npz")
            per_row = {k: (v[a:b] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B else v) for k, v in extra.items()}
            kw = dict(per_row, X=X[a:b], up=up[a:b], goal=goal[a:b], obs=obs[a:b])
            if params is not None:
                kw["params"] = np.array(params, dtype=object)
            np.savez(inp, **kw)
            env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
            procs.append((subprocess.Popen([sys.executable, os.path.abspath(__file__), inp, outp], env=env), outp))
        parts = []
        for p, outp in procs:
            rc = p.wait(timeout=timeout)
            assert rc == 0, f"oracle worker failed with {rc}"
            parts.append(dict(np.load(outp)))
    return {k: np.concatenate([q[k] for q in parts]) for k in parts[0]}


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2])
