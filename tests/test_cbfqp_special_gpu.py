"""The specialised cooperative CBF-QP kernel (cbfqp_coop8_du_kernel, csrc/cbf_qp_kernel.hpp) against the generic one.

The dispatcher sends a launch to the specialised kernel when it is DynamicUnicycle2D with f64 arithmetic, K = 8, per-agent
obstacles, no n_obs and a batch in the cooperative regime; SC_CBFQP_GENERIC=1 sends every launch to the generic kernel.  The
switch is read once per process, so each setting runs every case in ONE fresh child process (the two children run side by side,
each under its own time limit), and the outputs are compared as bits: u (NaN included), status and h.

Cases: B = 8 (one full wave), 200 (full waves only: FULL), 203 (a ragged last wave), 1; f32 and f64 storage; h_out present and
absent; hard mode on and off.  The batch is workloads.du_cbfqp_batch with single rows overwritten: an all-zero obstacle row, a
constraint row that is exactly (0, 0) (robot at rest, obstacle abeam), a NaN row, a duplicated row, one agent with no violated
row among agents that have some, |theta| >= 1e5 (the library branch of the sincos), a superellipsoid and an invalid flag.

The launches that must NOT take the new path (n_obs given, a shared table, K = 5, K = 16, B above SC_COOP_MAX_AGENTS) are held
to the C oracle by test_cbfqp_gpu.compare, with its tolerances, as tests/test_cbfqp_args_gpu.py does.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_cbfqp_gpu as T  # noqa: E402  (compare and its tolerances: the yardstick, used as it is)
from oracle import robots as R  # noqa: E402
from safe_control_amd import workloads as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (8, 200, 203, 1)
VARIANTS = [(io, want_h, mode) for io in ("f32", "f64") for want_h in (True, False) for mode in ("cbf", "hard")]


def batch(B):
    """du_cbfqp_batch(B, 8) with the degenerate rows written over single agents (B = 1 stays as drawn)."""
    X, _, u_ref, obs = W.du_cbfqp_batch(B, 8, seed=40 + B)
    X, u_ref, obs = X.copy(), u_ref.copy(), obs.copy()
    if B >= 8:
        at = (lambda j: j) if B == 8 else (lambda j: 10 * j + 3)      # B = 200 / 203: spread over the waves, odd group positions
        obs[at(0), 2] = 0.0                                            # an all-zero obstacle row
        obs[at(1), 5] = obs[at(1), 1]                                  # a duplicated row
        obs[at(2), 3, 0:6] = np.nan                                    # a NaN row (the flag stays a circle's)
        obs[at(3), :, 0:2] = X[at(3), None, 0:2] + 100.0               # no violated row: every obstacle far away
        X[at(4), 2] = 1.0e5 + 0.75                                     # the library branch of the sincos
        X[at(5), 2:4] = 0.0                                            # at rest, heading along x, obstacle abeam: the row is exactly (0, 0)
        obs[at(5), 4, 0:2] = [X[at(5), 0], X[at(5), 1] + 3.0]
        r = obs[at(6), 6, 2]
        obs[at(6), 6, 2:7] = [r + 0.3, 0.6 * r + 0.2, 4.0, 0.3, 1.0]   # a superellipsoid among the circles
        obs[at(7), 0, 6] = 2.0                                         # an invalid flag: status 3 for that agent
    if B == 203:
        X[202, 2] = -2.0e5                                             # the library branch in the ragged wave as well
        obs[201, 7] = obs[201, 0]
    return X, u_ref, obs


CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import safe_control_amd as sca
d = np.load(sys.argv[2])
out = {}
for B in (8, 200, 203, 1):
    for io in ("f32", "f64"):
        for mode in ("cbf", "hard"):
            ctl = sca.BatchedCBFQP({"model": "DynamicUnicycle2D", "a_max": 1.0, "w_max": 0.5, "radius": 0.25, "cbf_mode": mode},
                                   dt=0.05, io_dtype=io, compute_dtype="f64")
            t = lambda a: torch.tensor(a, dtype=ctl.torch_dtype, device="cuda:0")
            tX, tu, to = t(d[f"X{B}"]), t(d[f"u{B}"]), t(d[f"o{B}"])
            for want_h in (True, False):
                u, st, h = ctl.solve(tX, tu, to, None, want_h=want_h)
                torch.cuda.synchronize()
                key = f"{B}.{io}.{int(want_h)}.{mode}"
                bits = torch.int32 if io == "f32" else torch.int64
                out[key + ".u"] = u.view(bits).cpu().numpy()
                out[key + ".st"] = st.cpu().numpy()
                if want_h:
                    out[key + ".h"] = h.view(bits).cpu().numpy()
np.savez(sys.argv[3], **out)
"""


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """Every case under both settings of the switch: {setting: npz}.  One child per setting, started together."""
    tmp = tmp_path_factory.mktemp("special")
    inp = {}
    for B in BATCHES:
        inp[f"X{B}"], inp[f"u{B}"], inp[f"o{B}"] = batch(B)
    np.savez(tmp / "in.npz", **inp)
    env = {k: v for k, v in os.environ.items() if k != "SC_CBFQP_GENERIC"}
    procs = {}
    for name, extra in (("special", {}), ("generic", {"SC_CBFQP_GENERIC": "1"})):
        procs[name] = subprocess.Popen([sys.executable, "-c", CHILD, ROOT, str(tmp / "in.npz"), str(tmp / f"{name}.npz")],
                                       env=dict(env, **extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    res = {}
    try:
        for name, p in procs.items():
            _, err = p.communicate(timeout=300)
            assert p.returncode == 0, f"{name}: exit {p.returncode}\n{err[-2000:]}"
            res[name] = np.load(tmp / f"{name}.npz")
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
                p.wait()
    return res


def test_inputs_exercise_the_solve_and_its_edges():
    """By the C oracle the B = 203 batch holds agents moved off clamp(u_ref), infeasible ones and the invalid flag."""
    X, u_ref, obs = batch(203)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).astype(np.float64)
    spec = T.oracle_spec(R.MODEL_DU, T.du_spec())
    u, st, _ = T.c_oracle.cbfqp_batch(R.MODEL_DU, f32(X), f32(u_ref), f32(obs), spec, T.ocbf.default_cbf_param(R.MODEL_DU), 0.05, "cbf", None)
    box = np.clip(f32(u_ref), [-1.0, -0.5], [1.0, 0.5])
    moved = (st == 0) & (np.abs(u - box).max(axis=1) > 1e-9)
    print(f"oracle: {int(moved.sum())} moved, {int((st == 1).sum())} infeasible, {int((st == 3).sum())} bad obstacle, of {len(st)}")
    assert moved.sum() >= 30 and (st == 1).sum() >= 3 and (st == 3).sum() == 1
    assert st[33] == 0 and not moved[33]                               # the agent whose obstacles are far away


@pytest.mark.parametrize("io,want_h,mode", VARIANTS, ids=[f"{io}-{'h' if h else 'noh'}-{m}" for io, h, m in VARIANTS])
@pytest.mark.parametrize("B", BATCHES)
def test_special_equals_generic_bit_for_bit(both, B, io, want_h, mode):
    key = f"{B}.{io}.{int(want_h)}.{mode}"
    for name in ("u", "st") + (("h",) if want_h else ()):
        a, b = both["special"][f"{key}.{name}"], both["generic"][f"{key}.{name}"]
        assert a.shape == b.shape and a.dtype == b.dtype
        print(f"{key}.{name}: {int((a != b).sum())} of {a.size} entries differ")
        assert np.array_equal(a, b), f"{key}.{name}: differs at {np.argwhere(a != b)[:8].tolist()}"
    st = both["special"][f"{key}.st"]
    if B >= 8:
        assert (st == 3).sum() == 1 and (st == 0).any()


def test_statuses_are_not_all_alike(both):
    """The comparison above would hold for two kernels that return nothing: the 203-agent batch has all three statuses."""
    st = both["special"]["203.f32.1.cbf.st"]
    assert (st == 0).sum() >= 100 and (st == 1).sum() >= 3 and (st == 3).sum() == 1
    u = both["special"]["203.f32.1.cbf.u"].view(np.float32)
    assert np.isfinite(u[st == 0]).all() and np.isnan(u[st != 0]).all()


NOT_SPECIAL = ["n_obs", "shared", "K5", "K16", "above_coop_max"]


@pytest.mark.parametrize("case", NOT_SPECIAL)
def test_launches_that_keep_the_generic_path_hold_the_oracle(case):
    K = {"K5": 5, "K16": 16}.get(case, 8)
    B = 32776 if case == "above_coop_max" else 203
    X, _, u_ref, obs = W.du_cbfqp_batch(B, K, seed=900 + K + B)
    n_obs = None
    if case == "n_obs":
        n_obs = np.random.default_rng(9).integers(0, K + 1, B).astype(np.int32)
        n_obs[:8] = K                                                   # a whole group with every row used
        for i in range(B):
            obs[i, n_obs[i]:] = 1e30                                    # what lies beyond n_obs must be ignored
    if case == "shared":
        obs = obs[5].copy()
    T.compare(R.MODEL_DU, T.du_spec(), X, u_ref, obs, "f32", "f64", n_obs=n_obs)
