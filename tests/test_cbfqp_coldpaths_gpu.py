"""The cold blocks of the specialised cooperative CBF-QP kernel (cbfqp_coop8_du_kernel, csrc/cbf_qp_kernel.hpp, sc_group.hpp).

The kernel keeps three rare cases out of the path every wave executes, each under one wave-uniform branch: a flat direction of the
box clip (a component of a unit normal that is exactly 0.0), a partner row parallel to a candidate's line, and a bad obstacle flag.
The benchmark batch takes none of them, so nothing else runs them.  Here the inputs are built so that they run in waves whose other
lanes are ordinary, and so that one wave (agents 8..15 of the 24-agent batch) takes none:

  * an agent with two obstacles at the same centre and different radii -- identical normals, different offsets, exactly parallel
    rows -- once with both rows violated at clamp(u_ref) (the inner row's candidate line violates the outer row: a dead candidate)
    and once with neither violated;
  * an agent with v = 0 exactly: the second component of every row is exactly 0.0, before and after f32 storage;
  * one bad obstacle row (flag 2) in one group of a wave;
  * a duplicated obstacle;
  * ordinary agents as workloads.du_cbfqp_batch draws them.

B = 8 (one full wave), 13 (a ragged second wave: the !FULL instantiation) and 24 (three waves); K = 8; f32 and f64 storage; with
and without h_out; soft and hard mode.  Expected values: the same launches with SC_CBFQP_GENERIC=1 in a fresh child process, bit for
bit (the pattern of tests/test_cbfqp_special_gpu.py), and oracle.c_oracle.cbfqp_batch with the tolerances of
test_cbfqp_gpu.compare: |u - u_oracle| <= 1e-7 (f64 storage) / 2e-6 (f32 storage), h likewise relative to max(1, |h|) with 1e-9 /
2e-6, status equal.  Every constructed agent is compared and its status must be the oracle's; an ordinary agent may differ in status
only within 1e-6 of the feasibility margin, as in compare.  The CPU test checks with the numpy oracle that the inputs produce
each condition and that the numpy and the C oracle agree on every agent.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle, cbf_qp as ocbf, robots as R
from safe_control_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import count_coop8_branches as CB  # noqa: E402  (the rows as the kernel groups them; also what DESIGN.md 1b's counts come from)

BATCHES = (8, 13, 24)
VARIANTS = [(io, want_h, mode) for io in ("f32", "f64") for want_h in (True, False) for mode in ("cbf", "hard")]
PAR_BOTH, PAR_NONE, AT_REST, BAD_ROW, DUPLICATE = 1, 2, 3, 4, 5          # positions inside a wave of 8 agents


def spec():
    s = R.default_spec(R.MODEL_DU)
    s.update(a_max=1.0, w_max=0.5, radius=0.25)
    return s


def constructed(B):
    """{agent: kind} of a batch: wave 0 holds one of each; the ragged wave of B = 13 an agent at rest; wave 2 of B = 24 a second set."""
    c = {p: p for p in (PAR_BOTH, PAR_NONE, AT_REST, BAD_ROW, DUPLICATE)}
    if B == 13:
        c[12] = AT_REST
    if B == 24:
        c.update({16 + p: p for p in (PAR_BOTH, PAR_NONE, AT_REST, BAD_ROW, DUPLICATE)})
    return c


def batch(B):
    """du_cbfqp_batch(B, 8) with the constructed agents written over it."""
    X, _, u_ref, obs = W.du_cbfqp_batch(B, 8, seed=70 + B)
    X, u_ref, obs = X.copy(), u_ref.copy(), obs.copy()

    def pair(i, rows, bearing, rho, radii):
        """Two obstacles at one centre, `rho` away at `bearing` from the heading."""
        th = X[i, 2] + bearing
        for r, rad in zip(rows, radii):
            obs[i, r, 0:3] = [X[i, 0] + rho * np.cos(th), X[i, 1] + rho * np.sin(th), rad]

    for i, kind in constructed(B).items():
        second = i >= 16                                               # other rows, so other xor-partners, in the second set
        if kind == PAR_BOTH:                                           # closing on the pair, asked to accelerate: braking satisfies both
            X[i, 2:4] = [0.3, 0.5]
            pair(i, (2, 5) if second else (0, 1), 0.4, 1.25, (0.5, 0.7))
            u_ref[i] = [0.5, 0.1]
        elif kind == PAR_NONE:                                         # the pair lies behind: no input of the box violates it
            X[i, 2:4] = [-1.1, 0.8]
            pair(i, (1, 5) if second else (3, 4), np.pi - 0.4, 2.5, (0.4, 0.9))
        elif kind == AT_REST:                                          # v = 0: every row is (a, 0); one obstacle close ahead
            X[i, 2:4] = [0.3, 0.0]
            pair(i, (6,) if second else (2,), 0.2, 0.9, (0.5,))
            u_ref[i] = [1.0, 0.1]
        elif kind == BAD_ROW:
            obs[i, 7 if second else 4, 6] = 2.0
        elif kind == DUPLICATE:
            obs[i, 3] = obs[i, 1]
    return X, u_ref, obs


def stored(a, io):
    """What the kernel sees of an input array: rounded to the storage type."""
    return np.ascontiguousarray(a, dtype=np.float32 if io == "f32" else np.float64).astype(np.float64)


@pytest.fixture(scope="module")
def oracle():
    """C-oracle results of every batch, storage type and mode: {(B, io, mode): (u, status, h)}.  Computed once, read only."""
    out = {}
    for B in BATCHES:
        X, u_ref, obs = batch(B)
        for io in ("f32", "f64"):
            for mode in ("cbf", "hard"):
                res = c_oracle.cbfqp_batch(R.MODEL_DU, stored(X, io), stored(u_ref, io), stored(obs, io), spec(),
                                           ocbf.default_cbf_param(R.MODEL_DU), 0.05, mode, None)
                for a in res:
                    a.setflags(write=False)
                out[B, io, mode] = res
    return out


@pytest.mark.parametrize("io", ("f32", "f64"))
@pytest.mark.parametrize("B", BATCHES)
def test_inputs_produce_each_condition(oracle, B, io):
    """By the numpy oracle: the parallel pairs, the exactly zero component, the bad row, two violated rows; numpy and C oracle agree."""
    X, u_ref, obs = (stored(a, io) for a in batch(B))
    sp = spec()
    c = CB.conditions(X, u_ref, obs, sp)
    nviol = c["viol"].sum(axis=1)
    kinds = constructed(B)
    for i, kind in kinds.items():
        pairs = np.argwhere(np.triu(c["par"][i]))
        if kind == PAR_BOTH:
            assert len(pairs) == 1 and c["viol"][i, pairs[0]].all(), f"agent {i}: one parallel pair, both rows violated at u_box"
        elif kind == PAR_NONE:
            assert len(pairs) == 1 and not c["viol"][i, pairs[0]].any(), f"agent {i}: one parallel pair, neither row violated"
        elif kind == AT_REST:
            assert c["flat"][i].all() and c["viol"][i].any(), f"agent {i}: every row flat, one of them violated"
        elif kind == BAD_ROW:
            assert c["bad"][i].sum() == 1
        elif kind == DUPLICATE:
            assert c["par"][i, 1, 3] and np.array_equal(obs[i, 1], obs[i, 3])
    print(f"B={B} {io}: violated rows per agent {nviol.tolist()}")
    assert (nviol >= 2).any()
    ordinary = [i for i in range(B) if i not in kinds]
    assert not c["flat"][ordinary].any() and not c["par"][ordinary].any() and not c["bad"][ordinary].any()
    if B == 24:                                                        # the wave that takes none of the cold blocks, but enters the solve
        assert all(i in ordinary for i in range(8, 16)) and c["viol"][8:16].any()
    # the numpy oracle (per agent, so that the bad row's ValueError stays with its agent) against the C oracle
    for mode in ("cbf", "hard"):
        uo, so, ho = oracle[B, io, mode]
        for i in range(B):
            if kinds.get(i) == BAD_ROW:
                with pytest.raises(ValueError):
                    ocbf.solve(R.MODEL_DU, X[i], u_ref[i], list(obs[i]), sp, num_obs=8, dt=0.05, cbf_mode=mode)
                assert so[i] == 3 and np.isnan(uo[i]).all()
                continue
            r = ocbf.solve(R.MODEL_DU, X[i], u_ref[i], list(obs[i]), sp, num_obs=8, dt=0.05, cbf_mode=mode)
            assert r["status"] == so[i], f"agent {i} ({mode}): numpy oracle status {r['status']}, C oracle {so[i]}"
            if so[i] == 0:
                assert np.abs(r["u"] - uo[i]).max() <= 1e-7
            assert (np.abs(r["h"] - ho[i]) <= 1e-9 * np.maximum(1.0, np.abs(ho[i]))).all()
        print(f"B={B} {io} {mode}: status {so.tolist()}")
        assert all(so[i] == 0 for i, kind in kinds.items() if kind != BAD_ROW), "a constructed agent is infeasible: nothing to compare"


# ---------------------------------------------------------------------------------------------------------------- GPU
CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import safe_control_amd as sca
d = np.load(sys.argv[2])
out = {}
for B in (8, 13, 24):
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
    """Every case on the specialised and on the generic kernel: {setting: npz}.  One fresh child per setting, started together."""
    pytest.importorskip("torch")
    tmp = tmp_path_factory.mktemp("coldpaths")
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


IDS = [f"{io}-{'h' if h else 'noh'}-{m}" for io, h, m in VARIANTS]


@pytest.mark.gpu
@pytest.mark.parametrize("io,want_h,mode", VARIANTS, ids=IDS)
@pytest.mark.parametrize("B", BATCHES)
def test_special_equals_generic_bit_for_bit(both, B, io, want_h, mode):
    key = f"{B}.{io}.{int(want_h)}.{mode}"
    for name in ("u", "st") + (("h",) if want_h else ()):
        a, b = both["special"][f"{key}.{name}"], both["generic"][f"{key}.{name}"]
        assert a.shape == b.shape and a.dtype == b.dtype
        print(f"{key}.{name}: {int((a != b).sum())} of {a.size} entries differ")
        assert np.array_equal(a, b), f"{key}.{name}: differs at {np.argwhere(a != b)[:8].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("io,want_h,mode", VARIANTS, ids=IDS)
@pytest.mark.parametrize("B", BATCHES)
def test_special_holds_the_oracle(both, oracle, B, io, want_h, mode):
    """u, status and h of the specialised kernel against the C oracle, with the tolerances of test_cbfqp_gpu.compare."""
    import test_cbfqp_gpu as T                                         # margins(): the yardstick's own feasibility margin
    key = f"{B}.{io}.{int(want_h)}.{mode}"
    ft = np.float32 if io == "f32" else np.float64
    ug = both["special"][f"{key}.u"].view(ft).astype(np.float64)
    sg = both["special"][f"{key}.st"]
    uo, so, ho = oracle[B, io, mode]
    kinds = constructed(B)
    diff = np.nonzero(sg != so)[0]
    print(f"{key}: status gpu {sg.tolist()} oracle {so.tolist()}")
    assert not any(i in kinds for i in diff), f"status of a constructed agent differs from the oracle: {diff.tolist()}"
    if len(diff):
        X, _, obs = (stored(a, io) for a in batch(B))
        mg = T.margins(R.MODEL_DU, X[diff], obs[diff], spec(), ocbf.default_cbf_param(R.MODEL_DU), None, mode)
        assert np.all(np.abs(mg) < 1e-6), f"status mismatch away from the margin: {diff.tolist()}, margins {mg.tolist()}"
    assert len(diff) <= 2
    assert np.all(np.isnan(ug[sg != 0]))
    assert all(sg[i] == (3 if kind == BAD_ROW else 0) for i, kind in kinds.items())
    ok = (sg == 0) & (so == 0)
    err = np.abs(ug[ok] - uo[ok]).max(axis=1)
    tol_u = 1e-7 if io == "f64" else 2e-6                              # times max(1, largest bound) = 1
    print(f"{key}: max |u - u_oracle| {err.max():.3e} (tolerance {tol_u:g}) over {int(ok.sum())} agents")
    assert (err <= tol_u).all(), f"u: worst {err.max()} at agent {np.nonzero(ok)[0][err.argmax()]}"
    if want_h:
        hg = both["special"][f"{key}.h"].view(ft).astype(np.float64)
        herr = np.abs(hg - ho) / np.maximum(1.0, np.abs(ho))
        tol_h = 1e-9 if io == "f64" else 2e-6
        print(f"{key}: max relative |h - h_oracle| {herr.max():.3e} (tolerance {tol_h:g})")
        assert (herr <= tol_h).all(), f"h: worst {herr.max()}"
