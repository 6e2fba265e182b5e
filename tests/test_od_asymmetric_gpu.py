"""GPU: every optimal-decay kernel against its oracle at UNEQUAL decay parameters (gain, reference and penalty differ between the two
decay variables, references away from 1).  With the default parameters the two variables of a pair are interchangeable -- rho1_k and
rho2_k of the oracle come out equal to the last bit -- so the parity tests at the defaults cannot see a kernel that swaps p_sb1 / p_sb2,
omega1 / omega2 or alpha1 / alpha2 at one of its index sites, hard-codes a reference of 1, or drops the a1 a2 h cross term of a decay
block.  Here the controller gets ``cbf_param=`` the unequal set and the oracle the same numbers through its own parameter route
(tests/test_oracle_od_asymmetric.py pins the oracles at these sets first).

Bars: each family's existing ones, restated from its test -- same status; on the optimal problems |u0| 1e-6, |z| 2e-5, rho 1e-4
(DynamicUnicycle2D, relative degree 1), 1e-5 (bicycle, Quad2D), 2e-5 (VTOL2D), iterations within 2; the bicycle's crawler rule of
test_odmpcgn_gpu.py, Quad3D's acceptable-point rule of test_od_rd1_gpu.py, the multiple-shooting bars of test_mpcvtol_ms_gpu.py;
OD-CBF-QP 1e-7 (f64 storage) / 3e-6 (f32 storage) scaled by max(1, |.|).

Conditions on the inputs, checked from the ORACLE's results alone before any kernel output is looked at (check_inputs): >= 3/4 of a
batch optimal, >= 3/4 done in under 40 iterations, on >= 1/2 of the optimal problems some rho more than 1e-2 from its reference,
and on >= 1/2 of them u0 or rho moves by more than 100 x the comparison tolerance when the oracle is re-solved with the parameters of
the two variables exchanged (omega and p_sb; separately the gains) -- for the one-variable families with omega1 = 1, separately
p_sb1 = 10, in place of the given value.  That last condition is what makes a swap or a hard-coded default fail these tests.  The
counts are printed.  All inputs are rounded to f32 first, so that one oracle run serves the f64 launch and the f32-storage case.

Two families cannot meet the shares as the MPC batches do, for reasons of their inputs, and have their own, written down where they
are checked: the CBF-QP batches of test_odcbfqp_gpu.setup (one obstacle, the row is active on about a sixth of the problems: shares
of 1/8 of the batch) and the multiple-shooting VTOL2D solves (IPOPT's algorithm takes 50 - 400 iterations on these scenes by design;
there is no crawler excuse in its bars, so the 40-iteration condition does not apply).

Parameter sets.  DynamicUnicycle2D: alpha 0.02 / 0.005, omega 0.8 / 1.25, p_sb 3 / 40.  Quad2D: alpha 1.6 x / 0.5 x its default 0.15,
omega 0.8 / 1.25, p_sb 3 / 40.  KinematicBicycle2D: see KB_SET.  VTOL2D: see VTOL_SET.  Relative degree 1: see UNI_SET, QUAD3D_SET."""
import functools
import os
import sys
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import _oracle_pool as OP  # noqa: E402
from oracle import od_cbf_qp as OD, robots as R  # noqa: E402
from safe_control_amd import workloads as W  # noqa: E402
from test_od_rd1_gpu import UNI_SPEC, quad_scene, uni_scene  # noqa: E402
from test_od_vtol_gpu import hard_batch  # noqa: E402
from test_odcbfqp_gpu import NAMES, setup as qp_setup  # noqa: E402
from test_odmpccbf_gpu import SPEC as DU_SPEC  # noqa: E402

DEV = "cuda:0"

DU_SET = dict(alpha1=0.02, alpha2=0.005, omega1=0.8, omega2=1.25, p_sb1=3.0, p_sb2=40.0)
QUAD2D_SET = dict(alpha1=0.24, alpha2=0.075, omega1=0.8, omega2=1.25, p_sb1=3.0, p_sb2=40.0)
# KinematicBicycle2D (default alpha 0.05, p_sb 10): alpha x 1.6 / x 0.5 with p_sb 3 / 40 makes the oracle crawl (8 problems of seed 18:
# up to 122 iterations), so the gains and penalties stay nearer the defaults: alpha x 1.25 / x 0.8, p_sb 5 / 20.  The draws are those of
# seed 1: on seed 18 the oracle ends only 19 of 32 solves in under 40 iterations at the DEFAULT parameters already (and at every milder
# unequal set tried), so no parameter choice meets the iteration condition there; of seeds 0 - 7 at KB_SET, seed 1 has the fewest crawlers.
KB_SET = dict(alpha1=0.0625, alpha2=0.04, omega1=0.8, omega2=1.25, p_sb1=5.0, p_sb2=20.0)
VTOL_SET = dict(alpha1=0.6, alpha2=0.15, omega1=0.8, omega2=1.25, p_sb1=3.0, p_sb2=40.0)
# one decay variable per stage: gain, reference and penalty of that variable away from the defaults (0.05 | 0.15, 1, 10); omega2 / p_sb2
# belong to the inert second variable of the Unicycle2D extension, which must come back AT omega2
UNI_SET = dict(alpha=0.08, omega1=0.8, p_sb1=3.0, omega2=1.25, p_sb2=40.0)
QUAD3D_SET = dict(alpha=0.06, omega1=0.8, p_sb1=3.0)
QP_SET2 = dict(alpha1=0.8, alpha2=0.3, omega1=0.8, omega2=1.25, p_sb1=3.0, p_sb2=40.0)
QP_SET1 = dict(alpha=0.8, omega1=0.8, p_sb1=3.0, omega2=1.25)


def r32(a):
    """The array rounded to f32, as f64: what an f32-storage launch reads."""
    return np.ascontiguousarray(a).astype(np.float32).astype(np.float64)


def t(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def exchanged(p):
    """(omega and p_sb exchanged between the two variables, gains exchanged) -- or, with one variable, (omega1 = 1, p_sb1 = 10)."""
    if "alpha1" in p:
        return (("omega, p_sb exchanged", dict(p, omega1=p["omega2"], omega2=p["omega1"], p_sb1=p["p_sb2"], p_sb2=p["p_sb1"])),
                ("alpha exchanged", dict(p, alpha1=p["alpha2"], alpha2=p["alpha1"])))
    return (("omega1 = 1", dict(p, omega1=1.0)), ("p_sb1 = 10", dict(p, p_sb1=10.0)))


# ---- the batches and their oracle runs ---------------------------------------------------------------------------------------------

def _du(N, K):
    X, goal, _, obs = W.du_cbfqp_batch(32, K, seed=1)
    return (r32(X), np.zeros((32, 2)), r32(goal), r32(obs)), DU_SET, lambda a, p: (OP.od_du_solve_many, a, dict(params=dict(p, N=N)))


def _uni(N):
    X, goal, obs = uni_scene(32, 8, seed=N * 10 + 8)
    a = (r32(X), np.zeros((32, 2)), r32(goal), r32(obs))
    keys = ("alpha", "omega1", "p_sb1")
    return a, UNI_SET, lambda a_, p: (OP.od_rd1_solve_many, ("od_uni", a_[0][:, :3]) + a_[1:], dict(params=dict({k: p[k] for k in keys}, N=N)))


def _gn(fam, N=10, K=8):
    X, up, goal, obs = W.mpc_family_batch(fam, 32, K, seed={"kb": 1, "quad2d": 18}[fam])
    return (r32(X), r32(up), r32(goal), r32(obs)), {"kb": KB_SET, "quad2d": QUAD2D_SET}[fam], \
        lambda a, p: (OP.od_gn_solve_many, (fam,) + a, dict(params=dict(p, N=N)))


def _quad3d(N):
    X, goal, obs = quad_scene(32, 8, seed=N * 10 + 8)
    a = (r32(X), np.zeros((32, 4)), r32(goal), r32(obs))
    return a, QUAD3D_SET, lambda a_, p: (OP.od_rd1_solve_many, ("od_quad3d",) + a_, dict(params=dict(p, N=N)))


VTOL_N = 12


def _vtol_scene():
    """The problems of hard_batch that have a disc on the flight path (its even ones): without one no row is active and the decay
    variables sit on their references whatever the parameters."""
    return tuple(r32(a[::2]) for a in hard_batch(2 * VTOL_N))


def _vtol_wave():
    return _vtol_scene(), VTOL_SET, lambda a, p: (OP.od_vtol_solve_many, a, dict(params=dict(p), timeout=3000))


def _vtol_ms():
    from oracle import ms_ipopt as MS

    def job(a, p):
        return (OP.ms_solve_many, ("vtol_od",) + a, dict(opts=dict(MS.KERNEL_PROFILE), od=dict(omega_ref=(p["omega1"], p["omega2"]), p_sb=(p["p_sb1"], p["p_sb2"])),
                                                        alpha1=p["alpha1"], alpha2=p["alpha2"]))
    return _vtol_scene(), VTOL_SET, job


CASES = {"du-10-8": lambda: _du(10, 8), "du-6-3": lambda: _du(6, 3), "uni": lambda: _uni(10), "kb": lambda: _gn("kb"), "quad2d": lambda: _gn("quad2d"),
         "quad3d-10": lambda: _quad3d(10), "quad3d-20": lambda: _quad3d(20), "vtol-wave": _vtol_wave, "vtol-ms": _vtol_ms}
# (u0, rho) comparison tolerances of the family: the exchange condition asks for 100 x these
TOLS = {"du": (1e-6, 1e-4), "uni": (1e-6, 1e-4), "kb": (1e-6, 1e-5), "quad2d": (1e-6, 1e-5), "quad3d": (1e-6, 1e-4), "vtol": (1e-6, 2e-5)}


def _ms_fields(r, N=30):
    """u0 (the four physical inputs) and the decay rates of the plan of a multiple-shooting oracle run."""
    U = r["plan"][:, (N + 1) * 6:].reshape(len(r["u"]), N, -1)
    return dict(r, u=r["u"][:, :4], rho=U[:, :, 4:].reshape(len(r["u"]), -1))


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, parameter set, oracle run at the set, [(label, oracle run at an exchanged set), ..]) -- solved once per session."""
    args, pset, job = CASES[name]()
    t0 = time.time()
    runs = OP.concurrently([job(args, pset)] + [job(args, q) for _, q in exchanged(pset)])
    if name == "vtol-ms":
        runs = [_ms_fields(r) for r in runs]
    print(f"[{name}] oracle: {len(runs)} runs of {len(args[0])} problems in {time.time() - t0:.1f} s")
    return args, pset, runs[0], [(lab, r) for (lab, _), r in zip(exchanged(pset), runs[1:])]


def check_inputs(name, iteration_share=0.75):
    """The conditions of the module docstring, from the oracle alone; returns the case."""
    args, pset, o, alts = case(name)
    fam = name.split("-")[0]
    tu, tr = TOLS[fam]
    B = len(o["st"])
    ok = o["st"] == 0
    ref = np.array([pset["omega1"], pset["omega2"]] if "alpha1" in pset else [pset["omega1"]])
    rho = o["rho"].reshape(B, -1, len(ref))
    moved = np.abs(rho - ref).max(axis=(1, 2)) > 1e-2
    hist = np.bincount(np.minimum(o["it"] // 10, 10), minlength=11)
    print(f"[{name}] oracle at {pset}: optimal {int(ok.sum())}/{B}, under 40 iterations {int((o['it'] < 40).sum())}/{B} (by tens, last = 100+: {hist.tolist()}), "
          f"rho more than 1e-2 off its reference on {int((moved & ok).sum())}/{int(ok.sum())}; rho1 in [{rho[ok][..., 0].min():.3f}, {rho[ok][..., 0].max():.3f}]"
          + (f", rho2 in [{rho[ok][..., 1].min():.3f}, {rho[ok][..., 1].max():.3f}]" if len(ref) == 2 else ""))
    assert ok.sum() >= 0.75 * B, f"{name}: inputs: too few optimal"
    if iteration_share:
        assert (o["it"] < 40).sum() >= iteration_share * B, f"{name}: inputs: the oracle crawls"
    assert (moved & ok).sum() >= 0.5 * ok.sum(), f"{name}: inputs: the decay variables do not move"
    for lab, a in alts:
        both = ok & (a["st"] == 0)
        ch = (np.abs(a["u"] - o["u"]).max(axis=1) > 100 * tu) | (np.abs(a["rho"] - o["rho"]).max(axis=1) > 100 * tr)
        print(f"[{name}] {lab}: oracle's u0 or rho changes by more than 100 x tol on {int((ch & both).sum())}/{int(ok.sum())}; "
              f"max |du0| {np.abs(a['u'] - o['u'])[both].max():.3g}, max |drho| {np.abs(a['rho'] - o['rho'])[both].max():.3g}")
        assert (ch & both).sum() >= 0.5 * ok.sum(), f"{name}: inputs: '{lab}' does not change the answers"
    return args, pset, o


def report(name, **dev):
    print(f"[{name}] kernel against oracle: " + ", ".join(f"max |{k}| {v:.3g}" for k, v in dev.items()))


def launch(ctl, args, io="f64", **kw):
    td = torch.float64 if io == "f64" else torch.float32
    out = ctl.solve(*[t(a, td) for a in args], **kw)
    torch.cuda.synchronize()
    return out


def f32_storage_is_the_f64_launch_rounded(make, args, outs=2, **kw):
    """io_dtype = "f32" on f32 inputs against io_dtype = "f64" on the same numbers: same status and iterations, the f32 outputs the f64
    ones rounded to nearest.  Returns the f64 launch's outputs."""
    r64 = launch(make("f64"), args, "f64", **kw)
    rf = launch(make("f32"), args, "f32", **kw)
    assert torch.equal(r64[outs], rf[outs]) and torch.equal(r64[outs + 1], rf[outs + 1]), "status / iterations differ between f32 and f64 storage"
    for a, b in zip(r64[:outs], rf[:outs]):
        keep = ~torch.isnan(a).any(dim=1)
        assert torch.equal(a[keep].float(), b[keep]), float((a[keep].float() - b[keep]).abs().max())
    return r64


def strict_compare(name, o, u, rho, st, it, z, tol_rho, z_scale=False):
    """The bars of test_odmpccbf_gpu.py / test_od_rd1_gpu.py (Unicycle2D) / test_od_vtol_gpu.py."""
    assert np.array_equal(st, o["st"]), np.flatnonzero(st != o["st"])
    ok = o["st"] == 0
    du, dz, dr = np.abs(u - o["u"])[ok].max(), np.abs(z - o["z"])[ok].max(), np.abs(rho - o["rho"])[ok].max()
    report(name, du0=du, dz=dz, drho=dr, diters=np.abs(it - o["it"])[ok].max())
    assert du <= 1e-6 and dz <= 2e-5 and dr <= tol_rho
    return ok


# ---- csrc/od_cbf_qp.hip ------------------------------------------------------------------------------------------------------------

QP_B = 200


def qp_exchanged(p):
    """The QP's relative-degree-2 row, A u + b + (a1 + a2) omega1 h_dot + a1 a2 omega2 h, is symmetric in the two GAINS: exchanging them
    is no change of the problem (the oracle's answers stay put to the last bit), so the penalties and the references are exchanged
    separately here instead."""
    if "alpha1" in p:
        return (("p_sb exchanged", dict(p, p_sb1=p["p_sb2"], p_sb2=p["p_sb1"])), ("omega exchanged", dict(p, omega1=p["omega2"], omega2=p["omega1"])))
    return exchanged(p)


@functools.lru_cache(maxsize=None)
def qp_case(model, io):
    """Inputs of test_odcbfqp_gpu.setup as the launch reads them (rounded for f32 storage) and the oracle at the unequal set and at its
    exchanged sets."""
    X, ur, obs, spec, ospec = qp_setup(model, QP_B, seed=11)
    if io == "f32":
        X, ur, obs = r32(X), r32(ur), r32(obs)
    has = np.ones(QP_B, dtype=np.int32); has[::17] = 0
    pset = QP_SET2 if model in R.REL_DEG2 else QP_SET1
    runs = [[OD.solve(model, X[i], ur[i], obs[i] if has[i] else None, ospec, param=q) for i in range(QP_B)] for q in [pset] + [q for _, q in qp_exchanged(pset)]]
    return (X, ur, obs, has, spec), pset, runs


@pytest.mark.parametrize("model", [R.MODEL_DU, R.MODEL_KB, R.MODEL_QUAD2D, R.MODEL_KB_C3BF, R.MODEL_KB_DPCBF])
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_od_cbf_qp(model, io):
    """Input shares for this family: the batches of test_odcbfqp_gpu.setup hold ONE obstacle per problem and the row is active on about a
    sixth of them (measured on the oracle: DynamicUnicycle2D, 300 problems of seed 11: 49 active); elsewhere the decay variables sit on
    their references and u on the clipped reference whatever the parameters.  So the shares of 1/2 are taken over the problems whose ROW
    IS ACTIVE in the oracle (its answer is not the clipped reference with the decay variables on their references), of which there must
    be 25 or more: on at least half of those a decay variable is more than 1e-2 off its reference, and on at least half of those each
    exchange moves the oracle's answer by more than 100 x the tolerance."""
    import safe_control_amd as sca
    (X, ur, obs, has, spec), pset, (base, *alts) = qp_case(model, io)
    name = f"qp-{NAMES[model]}-{io}"
    tol = 1e-7 if io == "f64" else 3e-6
    ok = np.array([r["status"] == 0 for r in base])
    refw = np.array([pset["omega1"], pset["omega2"]])
    vec = lambda rs: np.array([np.concatenate([r["u"], r["omega"]]) if r["status"] == 0 else np.full(4, np.nan) for r in rs])   # noqa: E731
    vb = vec(base)
    moved = np.abs(vb[:, 2:] - refw).max(axis=1) > 1e-2
    lo, hi = (np.array(b) for b in __import__("oracle.cbf_qp", fromlist=["input_bounds"]).input_bounds(model, R.default_spec(model) | {k: v for k, v in spec.items() if k != "model"}))
    free = np.concatenate([np.clip(ur, lo, hi), np.tile(refw, (QP_B, 1))], axis=1)              # the answer where no row binds
    active = ok & (np.abs(vb - free).max(axis=1) > 1e-9)
    print(f"[{name}] oracle at {pset}: optimal {int(ok.sum())}/{QP_B}, row active on {int(active.sum())}, a decay variable more than 1e-2 off its reference on {int((moved & active).sum())} of those; "
          f"omega1 in [{np.nanmin(vb[:, 2]):.3f}, {np.nanmax(vb[:, 2]):.3f}], omega2 in [{np.nanmin(vb[:, 3]):.3f}, {np.nanmax(vb[:, 3]):.3f}]")
    assert ok.sum() >= 0.75 * QP_B and active.sum() >= QP_B // 8 and (moved & active).sum() >= 0.5 * active.sum()
    for (lab, _), rs in zip(qp_exchanged(pset), alts):
        ch = np.abs(vec(rs) - vb).max(axis=1) > 100 * tol * np.maximum(1.0, np.abs(vb).max(axis=1))
        print(f"[{name}] {lab}: oracle's u or omega changes by more than 100 x tol on {int((ch & active).sum())} of the {int(active.sum())} with an active row")
        assert (ch & active).sum() >= 0.5 * active.sum(), lab
    ctl = sca.BatchedOptimalDecayCBFQP(dict(spec), io_dtype=io, compute_dtype="f64", cbf_param=dict(pset))
    td = ctl.torch_dtype
    u, w, st, h = ctl.solve(t(X, td), t(ur, td), t(obs, td), torch.tensor(has, device=DEV))
    u, w, st, h = u.double().cpu().numpy(), w.double().cpu().numpy(), st.cpu().numpy(), h.double().cpu().numpy()
    worst = np.zeros(3)
    for i, r in enumerate(base):
        assert st[i] == r["status"], i
        if r["status"] != 0:
            continue
        e = (np.abs(u[i] - r["u"]).max() / max(1.0, float(np.abs(r["u"]).max())), np.abs(w[i] - r["omega"]).max() / max(1.0, float(np.abs(r["omega"]).max())),
             abs(h[i] - (r["h"] if has[i] else 0.0)) / max(1.0, abs(r["h"])))
        worst = np.maximum(worst, e)
        assert max(e) <= tol, (i, e, u[i], r["u"], w[i], r["omega"])
    report(name, du=worst[0], domega=worst[1], dh=worst[2])
    if model not in R.REL_DEG2:                                # the inert second variable: AT its reference on every problem, not at 1
        assert np.all(w[:, 1] == pset["omega2"])                # (1.25: the same number in f32)


# ---- csrc/mpc_cbf.hip, optimal decay -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K", [(10, 8), (6, 3)])
def test_dynamic_unicycle(N, K):
    import safe_control_amd as sca
    name = f"du-{N}-{K}"
    args, pset, o = check_inputs(name)
    make = lambda io: sca.BatchedOptimalDecayMPCCBF(dict(DU_SPEC), io_dtype=io, horizon=N, cbf_param=dict(pset))     # noqa: E731
    if N == 10:
        u, rho, st, it, z = f32_storage_is_the_f64_launch_rounded(make, args, want_z=True)
    else:
        u, rho, st, it, z = launch(make("f64"), args, want_z=True)
    u, rho, st, it, z = (a.cpu().numpy() for a in (u, rho, st, it, z))
    ok = strict_compare(name, o, u, rho, st, it, z, 1e-4)
    assert np.abs(it - o["it"])[ok].max() <= 2


def test_unicycle2d_extension():
    import safe_control_amd as sca
    args, pset, o = check_inputs("uni")
    make = lambda io: sca.BatchedOptimalDecayMPCCBF(dict(UNI_SPEC), io_dtype=io, horizon=10, extension=True, cbf_param=dict(pset))     # noqa: E731
    u, rho, st, it, z = (a.cpu().numpy() for a in f32_storage_is_the_f64_launch_rounded(make, args, want_z=True))
    ok = strict_compare("uni", o, u, rho[:, 0::2], st, it, z, 1e-4)
    assert np.abs(it - o["it"])[ok].max() <= 2
    assert np.all(rho[:, 1::2] == pset["omega2"])              # the inert omega2_k: at the GIVEN reference on every stage of every problem


# ---- csrc/mpc_gn.hip, optimal decay ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", ["kb", "quad2d"])
def test_step_barrier_models(fam):
    """The rule of test_odmpcgn_gpu.py: a status may differ only where one side crawls for 40+ iterations (at most B / 8 such problems);
    a solve that left through the acceptable-point rule (err > 1e-6) has the wider bars of that test; iterations within 2 unless both
    sides crawl for 60+.

    KinematicBicycle2D, parameters chosen (KB_SET): alpha 0.0625 / 0.04 (x 1.25 / x 0.8), omega 0.8 / 1.25, p_sb 5 / 20, on the draws of
    seed 1.  Oracle there: 27 of 32 optimal, 29 under 40 iterations; iterations by tens (0-9, 10-19, .., 100+):
    [0, 8, 11, 10, 1, 0, 1, 0, 0, 0, 1].  Seed 18, the draws of test_odmpcgn_gpu.py: [0, 7, 9, 3, 2, 3, 1, 1, 0, 2, 4] at this set
    and [0, 7, 7, 5, 2, 3, 1, 0, 0, 2, 5] at the defaults -- 19 of 32 under 40 either way."""
    import safe_control_amd as sca
    args, pset, o = check_inputs(fam)
    N, B = 10, len(args[0])
    name = {"kb": "KinematicBicycle2D", "quad2d": "Quad2D"}[fam]
    make = lambda io: sca.BatchedOptimalDecayGnMPCCBF({"model": name}, io_dtype=io, horizon=N, cbf_param=dict(pset))     # noqa: E731
    u, rho, st, it, z = (a.cpu().numpy() for a in f32_storage_is_the_f64_launch_rounded(make, args, want_z=True))
    n_opt = n_parted = 0
    worst = np.zeros(3)
    for i in range(B):
        so, ito = int(o["st"][i]), int(o["it"][i])
        if st[i] != so:
            assert max(int(it[i]), ito) >= 40, f"status differs at problem {i}: {st[i]} vs {so} after {it[i]} / {ito} iterations"
            n_parted += 1
            continue
        if so != 0:
            continue
        tol = (1e-6, 1e-5, 2e-5) if o["err"][i] <= 1e-6 else (1e-4, 1e-3, 1e-3)
        e = (np.abs(u[i] - o["u"][i]).max() / max(1.0, np.abs(o["u"][i]).max()), np.abs(rho[i] - o["rho"][i]).max(),
             np.abs(z[i] - o["z"][i]).max() / max(1.0, np.abs(o["z"][i]).max()))
        assert e[0] <= tol[0] and e[1] <= tol[1] and e[2] <= tol[2], (i, e, tol)
        assert abs(int(it[i]) - ito) <= 2 or min(int(it[i]), ito) >= 60, i
        if o["err"][i] <= 1e-6:
            worst = np.maximum(worst, e)
        n_opt += 1
    report(fam, du0=worst[0], drho=worst[1], dz=worst[2])
    print(f"[{fam}] compared {n_opt}, parted {n_parted}")
    assert n_opt >= B // 2 and n_parted <= B // 8


# ---- csrc/mpc_lin.hip, optimal decay (Quad3D) --------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [10, 20])
def test_quad3d(N):
    """N = 10: the lean layout; N = 20: the four-wave layout.  The rule of test_od_rd1_gpu.py: problems whose iteration counts differ by
    more than 2 left through the acceptable-point rule where rounding says (at most 15 % of the optimal ones), held to 1e-4 on u0."""
    import safe_control_amd as sca
    name = f"quad3d-{N}"
    args, pset, o = check_inputs(name)
    make = lambda io: sca.BatchedOptimalDecayLinearMPCCBF({"model": "Quad3D"}, io_dtype=io, horizon=N, cbf_param=dict(pset))     # noqa: E731
    u, rho, st, it, z = (a.cpu().numpy() for a in f32_storage_is_the_f64_launch_rounded(make, args, want_z=True))
    assert np.array_equal(st, o["st"]), np.flatnonzero(st != o["st"])
    ok = o["st"] == 0
    tight = ok & (np.abs(it - o["it"]) <= 2)
    assert tight.sum() >= 0.85 * ok.sum()
    du, dz, dr = np.abs(u - o["u"])[tight].max(), np.abs(z - o["z"])[tight].max(), np.abs(rho - o["rho"])[tight].max()
    report(name, du0=du, dz=dz, drho=dr)
    assert du <= 1e-6 and dz <= 2e-5 and dr <= 1e-4
    loose = ok & ~tight
    if loose.any():
        assert np.abs(u[loose] - o["u"][loose]).max() <= 1e-4 * max(1.0, np.abs(o["u"][loose]).max())


# ---- csrc/mpc_vtol_wave.hip and csrc/mpc_vtol_ms.hip, optimal decay ----------------------------------------------------------------

def test_vtol_condensed():
    """f32 storage: on the problems that end optimal the f32 outputs are the f64 launch's rounded to nearest (the existing f32 case of
    test_od_vtol_gpu.py holds them to 1e-6 only)."""
    import safe_control_amd as sca
    args, pset, o = check_inputs("vtol-wave")
    u, rho, st, it, z = (a.cpu().numpy() for a in launch(sca.BatchedOptimalDecayVtolMPCCBF(io_dtype="f64", cbf_param=dict(pset)), args, want_z=True))
    strict_compare("vtol-wave", o, u, rho, st, it, z, 2e-5)
    u32, rho32, s32, i32 = launch(sca.BatchedOptimalDecayVtolMPCCBF(io_dtype="f32", cbf_param=dict(pset)), args, "f32")
    assert np.array_equal(s32.cpu().numpy(), st) and np.array_equal(i32.cpu().numpy(), it)
    opt = torch.tensor(st == 0, device=DEV)
    assert torch.equal(t(u).float()[opt], u32[opt]) and torch.equal(t(rho).float()[opt], rho32[opt])


def test_vtol_multiple_shooting():
    """The bars of test_mpcvtol_ms_gpu.py::test_optimal_decay_instantiation_against_the_oracle: same status on every problem; the same
    optimum (u0 to 1e-6, decay rates to 1e-5) on >= 97 % of the problems both call optimal; iteration counts equal on >= 85 % and within
    30 % + 10 on all.  No 40-iteration condition on the inputs: IPOPT's algorithm takes 50 - 400 iterations on these scenes and the
    bars excuse no crawler."""
    import safe_control_amd as sca
    args, pset, o = check_inputs("vtol-ms", iteration_share=0)
    ctl = sca.BatchedOptimalDecayVtolMSMPCCBF(io_dtype="f64", cbf_param=dict(pset), fallback=False)
    u, rho, st, it = (a.cpu().numpy() for a in launch(ctl, args))
    assert np.array_equal(st, o["st"]), np.flatnonzero(st != o["st"])
    both = o["st"] == 0
    du, dr = np.abs(u - o["u"]).max(axis=1), np.abs(rho - o["rho"]).max(axis=1)
    report("vtol-ms", du0=du[both].max(), drho=dr[both].max(), diters=np.abs(it - o["it"])[both].max())
    same = (du <= 1e-6) & (dr <= 1e-5)
    assert same[both].mean() >= 0.97, (np.flatnonzero(both & ~same), du[both].max(), dr[both].max())
    assert np.mean(it[both] == o["it"][both]) >= 0.85 and (np.abs(it[both] - o["it"][both]) <= 0.3 * o["it"][both] + 10).all()


# ---- the drop-in classes: cbf_param mutated in place between two calls ("online adaptive CBF") -------------------------------------
# Each class solves once at its defaults, has ctl.cbf_param updated IN PLACE to the unequal set, and solves again from the same u_prev:
# the second answer is the oracle's at the new parameters (a parameter block cached at construction, or omega2 / p_sb2 written to the
# wrong slot, fails here) and differs from the first by more than 1e-4.  The scenes are the ones of each draw on which the oracle's
# answers at the two parameter sets differ (a row is active); bars as in each class's own drop-in test.

TRACK = "track"


def test_dropin_od_cbf_qp():
    import safe_control_amd as sca
    X, ur, obs, spec, ospec = qp_setup(R.MODEL_DU, 20, seed=3)
    robot = sca.RobotHandle(X[0], dict(spec), dt=0.05)
    for i in (3, 7, 18):
        ctl = sca.OptimalDecayCBFQP(robot, dict(spec))
        robot.X = X[i].reshape(-1, 1)
        u1 = ctl.solve_control_problem(robot.X, {"u_ref": ur[i].reshape(2, 1)}, obs[i]).reshape(-1)
        ctl.cbf_param.update(QP_SET2)
        u2 = ctl.solve_control_problem(robot.X, {"u_ref": ur[i].reshape(2, 1)}, obs[i]).reshape(-1)
        r = OD.solve(R.MODEL_DU, X[i], ur[i], obs[i], ospec, param=QP_SET2)
        assert ctl.status == "optimal" and r["status"] == 0
        np.testing.assert_allclose(u2, r["u"], atol=1e-7)
        np.testing.assert_allclose(ctl.omega, r["omega"], atol=1e-7)
        assert np.abs(u2 - u1).max() > 1e-4 and np.abs(r["omega"] - [QP_SET2["omega1"], QP_SET2["omega2"]]).max() > 1e-2, i


def test_dropin_od_mpc_cbf_dynamic_unicycle():
    import safe_control_amd as sca
    from oracle import od_mpc_cbf as O
    Xn, goal, _, on = W.du_cbfqp_batch(8, 5, seed=3)
    for i in (0, 1, 5):
        ctl = sca.OptimalDecayMPCCBF(sca.RobotHandle(Xn[i], dict(DU_SPEC), dt=0.05), dict(DU_SPEC), num_obs=5)
        ref = {"state_machine": TRACK, "u_ref": np.zeros((2, 1)), "goal": goal[i]}
        u1 = ctl.solve_control_problem(Xn[i].reshape(-1, 1), ref, on[i]).reshape(-1)
        ctl.cbf_param.update(DU_SET)
        ctl.u_prev = np.zeros(2)
        u2 = ctl.solve_control_problem(Xn[i].reshape(-1, 1), ref, on[i]).reshape(-1)
        uo, ro, so, ito, info = O.solve(Xn[i], np.zeros(2), goal[i], on[i], params=dict(DU_SET), return_info=True)
        assert so == 0 and ctl.solver_status == "optimal" and abs(ctl.iterations - ito) <= 2
        assert np.abs(u2 - uo).max() <= 1e-6 and abs(ctl.omega1 - ro[0]) <= 1e-4 and abs(ctl.omega2 - ro[1]) <= 1e-4
        assert np.abs(ctl.rho - info["zz"][20:]).max() <= 1e-4
        assert np.abs(u2 - u1).max() > 1e-4, i


def test_dropin_od_mpc_cbf_quad2d():
    import safe_control_amd as sca
    from oracle import od_mpc_gn as OG
    X, up, goal, obs = W.mpc_family_batch("quad2d", 8, 5, seed=2)
    mdl = OG.quad2d_model()
    for i in (2, 3, 4):
        ctl = sca.OptimalDecayMPCCBF(sca.RobotHandle(X[i], {"model": "Quad2D"}), {"model": "Quad2D"}, num_obs=5)
        assert type(ctl).__name__ == "OptimalDecayGnMPCCBF"
        ref = {"state_machine": TRACK, "u_ref": np.zeros((2, 1)), "goal": goal[i]}
        ctl.u_prev = up[i].copy()
        u1 = ctl.solve_control_problem(X[i].reshape(-1, 1), ref, obs[i]).reshape(-1)
        ctl.cbf_param.update(QUAD2D_SET)
        ctl.u_prev = up[i].copy()
        u2 = ctl.solve_control_problem(X[i].reshape(-1, 1), ref, obs[i]).reshape(-1)
        uo, ro, so, ito, info = OG.solve(mdl, X[i], up[i], goal[i], obs[i], N=10, params_over=dict(QUAD2D_SET), return_info=True)
        assert so == 0 and info["err"] <= 1e-6 and ctl.solver_status == "optimal" and abs(ctl.iterations - ito) <= 2
        assert np.abs(u2 - uo).max() <= 1e-6 * max(1.0, np.abs(uo).max())
        assert abs(ctl.omega1 - ro[0]) <= 1e-5 and abs(ctl.omega2 - ro[1]) <= 1e-5 and np.abs(ctl.rho - info["zz"][20:]).max() <= 1e-5
        assert np.abs(u2 - u1).max() > 1e-4, i


def test_dropin_od_mpc_cbf_quad3d_as_routed():
    """Quad3D is routed to the PLAIN row with R u^2 (test_od_quad3d_gpu.py): of cbf_param only the gain ``alpha`` reaches the kernel;
    omega1 / omega2 are the inert decay inputs and are reported at their references -- the GIVEN ones."""
    import safe_control_amd as sca
    from oracle import mpc_lin as L

    class Robot:
        dt, robot_radius = 0.05, 0.25
    X, G, Ob = quad_scene(8, 5, seed=5, superell=False)
    mdl = L.quad3d_model()
    new = dict(alpha=0.04, omega1=0.8, omega2=1.25, p_sb1=3.0, p_sb2=40.0)
    for i in (3, 6):
        ctl = sca.OptimalDecayMPCCBF(Robot(), {"model": "Quad3D"})
        assert type(ctl).__name__ == "OptimalDecayLinearMPCCBF"
        ref = {"state_machine": TRACK, "u_ref": np.zeros((4, 1)), "goal": G[i]}
        u1 = ctl.solve_control_problem(X[i].reshape(-1, 1), ref, Ob[i][:, :3]).reshape(-1)
        ctl.cbf_param.update(new)
        ctl.u_prev = np.zeros(4)
        u2 = ctl.solve_control_problem(X[i].reshape(-1, 1), ref, Ob[i][:, :3]).reshape(-1)
        uo, so, ito, info = L.solve(mdl, X[i], np.zeros(4), G[i], Ob[i], N=10, params_over={"rterm": "u2", "alpha": new["alpha"]}, return_info=True)
        assert so == 0 and info["err"] <= 1e-6 and ctl.solver_status == "optimal" and abs(ctl.iterations - ito) <= 2
        assert np.abs(u2 - uo).max() <= 1e-6
        assert ctl.omega1 == 0.8 and ctl.omega2 == 1.25
        assert np.abs(u2 - u1).max() > 1e-4, i


def test_dropin_od_mpc_cbf_vtol():
    """Bars of the multiple-shooting kernel (test_mpcvtol_ms_gpu.py): u0 to 1e-6, decay rates to 1e-5, iterations within 30 % + 10."""
    import safe_control_amd as sca
    from oracle import mpc_cbf as M, ms_ipopt as MS
    x0 = np.array([0.0, 10.0, 0.0, 12.0, 0.0, 0.0])
    ref = {"state_machine": TRACK, "goal": np.array([100.0, 10.0]), "u_ref": np.zeros((4, 1))}
    p = VTOL_SET
    for ox in (22.0, 16.0):
        obsl = np.array([[ox, 10.5, 1.5]])
        robot = sca.RobotHandle(x0.reshape(-1, 1), {"model": "VTOL2D"}, dt=0.05)
        ctl = sca.OptimalDecayMPCCBF(robot, {"model": "VTOL2D"}, num_obs=2)
        assert type(ctl).__name__ == "OptimalDecayVtolMPCCBF"
        u1 = ctl.solve_control_problem(robot.X, ref, obsl).reshape(-1)
        ctl.cbf_param.update(p)
        ctl.u_prev = np.zeros(4)
        u2 = ctl.solve_control_problem(robot.X, ref, obsl).reshape(-1)
        mdl = MS.vtol_od_model(dict(radius=robot.robot_radius))
        mdl.update(alpha1=p["alpha1"], alpha2=p["alpha2"], od=dict(omega_ref=np.array([p["omega1"], p["omega2"]]), p_sb=np.array([p["p_sb1"], p["p_sb2"]])))
        uo, so, ito, info = MS.solve(mdl, x0, np.zeros(4), ref["goal"], M.pad_obstacles(obsl, 2), return_info=True, opts=dict(MS.KERNEL_PROFILE))
        rho_o = info["U"][:, 4:].reshape(-1)
        assert so == 0 and ctl.solver_status == "optimal" and abs(ctl.iterations - ito) <= 0.3 * ito + 10, (ctl.iterations, ito)
        assert np.abs(u2 - uo[:4]).max() <= 1e-6 and np.abs(ctl.rho - rho_o).max() <= 1e-5
        assert abs(ctl.omega1 - rho_o[0]) <= 1e-5 and abs(ctl.omega2 - rho_o[1]) <= 1e-5
        assert np.abs(rho_o.reshape(-1, 2) - [p["omega1"], p["omega2"]]).max() > 1e-2 and np.abs(u2 - u1).max() > 1e-4, ox
