"""The branches that the scalar-path change of the specialised cooperative CBF-QP kernel added or moved (cbfqp_coop8_du_kernel,
csrc/cbf_qp_kernel.hpp; "cold paths of the specialised solve" in csrc/sc_group.hpp).

That change takes the literals of the solve from the argument block, keeps the smallest |a| of the seven partner clips instead of
a flag per partner (one compare against eps_par = 1e-12 after the loop decides whether the parallel-partner block runs), puts the
`nn > 0` guard of the row normalisation under a wave-uniform branch, and makes `hard` a template argument (soft and hard mode
are two instantiations).  The benchmark batch takes none of the cold sides, so nothing else runs them.  Here agents are written
over workloads.du_cbfqp_batch draws so that each of them runs in a wave whose other lanes are ordinary:

  * mixed-flag waves: waves with exactly one superellipsoid row (wave 0 of every batch), a wave whose 64 rows are all
    superellipsoids (wave 2 of B = 24), and an invalid flag in a wave that also holds a superellipsoid (wave 0 of B = 24);
  * degenerate rows (wave 0 of B = 24): an all-zero row (an agent at rest heading along x, the obstacle exactly abeam), a row
    whose normal is (2e-170, 0), so that its sum of squares underflows to nn == 0 (f64 storage; f32 storage rounds the offset to 0
    and the row is all-zero as well), and a NaN obstacle (wave 0 of every batch).  An all-zero or underflowed row is itself a
    parallel partner of every other row of its agent (a == 0 or about 1e-170), and so is the row the kernel zeroes for an invalid
    flag: those agents set the parallel-partner flag of their wave too, which is why they share no wave with the pairs below;
  * parallel-partner pairs, both rows violated at clamp(u_ref), each the ONLY agent of its wave that can set the flag, so that
    the pair alone decides whether the cold block runs: |n_i x n_j| = 0.6e-12 in the one wave of B = 8 (the block runs), 1.7e-12
    in wave 0 of B = 13 (no agent of the wave is parallel: the block must not run), on either side of eps_par and within a factor
    of two of it (f64 storage; f32 storage cannot hold a 1e-12 angle: the two centres round to bearings about 1e-7 apart and
    neither pair is parallel, so no wave of B = 8 takes the block), and one exactly parallel pair (one centre, two radii) in the
    ragged wave of B = 13.  Ratios reached, by count_coop8_branches.conditions on the f64 inputs: 0.600 and 1.700 of eps_par
    (printed by the CPU test, asserted to lie in [0.5, 1) and (1, 2]).  The CPU test asserts, per storage type and wave, which
    agents set the flag.

B = 8 (one full wave), 13 (ragged: the !FULL instantiations) and 24 (three waves, the middle one ordinary); K = 8; f32 and f64
storage; with and without h_out; soft and hard mode.  Expected values: the same launches with SC_CBFQP_GENERIC=1 in a fresh child
process, bit for bit, and oracle.c_oracle.cbfqp_batch with the tolerances of test_cbfqp_gpu.compare: |u - u_oracle| <= 1e-7 (f64
storage) / 2e-6 (f32 storage), h likewise relative to max(1, |h|) with 1e-9 / 2e-6, status equal.  Every constructed agent is
compared and its status must be the oracle's; an ordinary agent may differ in status only within 1e-6 of the feasibility margin, as
in compare.  The CPU test checks with the numpy oracle that the inputs produce each condition, per storage type, and that the
numpy and the C oracle agree on every agent.
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
SUPER_ONE, ZERO_ROW, UNDERFLOW, NAN_ROW, PAR_BELOW, PAR_ABOVE, PAR_EXACT, SUPER_ALL, BAD_AND_SUPER = range(1, 10)
EPS_PAR = 1e-12
BELOW, ABOVE = 0.6e-12, 1.7e-12                           # |n_i x n_j| aimed at
PAIR_ROWS = (2, 5)                                        # rows of the near-parallel and the exactly parallel pairs
# {batch: {agent: kind}}.  No wave holds two agents that can set the parallel-partner flag except wave 0 of B = 24, where the
# degenerate rows and the invalid flag live; agent 0 of every batch stays ordinary (the idle lanes of a ragged wave compute on it).
LAYOUT = {
    8: {1: SUPER_ONE, 4: NAN_ROW, 5: PAR_BELOW},
    13: {1: SUPER_ONE, 4: NAN_ROW, 6: PAR_ABOVE, 10: PAR_EXACT},
    24: {1: BAD_AND_SUPER, 2: ZERO_ROW, 3: UNDERFLOW, 4: NAN_ROW, **{i: SUPER_ALL for i in range(16, 24)}},
}
# agents that set the parallel-partner flag, per batch and storage type: {(B, io): {wave: [agents]}}; every other wave: none
PAR_TRIGGERS = {(8, "f64"): {0: [5]}, (8, "f32"): {}, (13, "f64"): {1: [10]}, (13, "f32"): {1: [10]},
                (24, "f64"): {0: [1, 2, 3]}, (24, "f32"): {0: [1, 2, 3]}}


def spec():
    s = R.default_spec(R.MODEL_DU)
    s.update(a_max=1.0, w_max=0.5, radius=0.25)
    return s


def constructed(B):
    """{agent: kind} of a batch."""
    return dict(LAYOUT[B])


def superellipsoid(obs, i, r):
    """The circle of row r of agent i made a superellipsoid on the same centre (as tests/test_cbfqp_special_gpu.py does)."""
    rad = obs[i, r, 2]
    obs[i, r, 2:7] = [rad + 0.3, 0.6 * rad + 0.2, 4.0, 0.3, 1.0]


def cross_of(X, obs, i, rows):
    c = CB.conditions(X[i:i + 1], np.zeros((1, 2)), obs[i:i + 1], spec())
    return c["cross"][0, rows[0], rows[1]]


def batch(B):
    """du_cbfqp_batch(B, 8) with the constructed agents written over it."""
    X, _, u_ref, obs = W.du_cbfqp_batch(B, 8, seed=80 + B)
    X, u_ref, obs = X.copy(), u_ref.copy(), obs.copy()
    for i, kind in constructed(B).items():
        if kind == SUPER_ONE:
            superellipsoid(obs, i, 3)
        elif kind == SUPER_ALL:
            for r in range(8):
                superellipsoid(obs, i, r)
        elif kind == BAD_AND_SUPER:
            superellipsoid(obs, i, 6)
            obs[i, 1, 6] = 2.0
        elif kind == ZERO_ROW:                                         # at rest, heading along x, obstacle abeam: the row is exactly (0, 0)
            X[i, 2:4] = 0.0
            obs[i, 4, 0:2] = [X[i, 0], X[i, 1] + 3.0]
        elif kind == UNDERFLOW:                                        # the same with the obstacle 1e-170 behind abeam: the row is (2e-170, 0)
            X[i, 0] = 0.0
            X[i, 2:4] = 0.0
            obs[i, :, 0] -= obs[i, :, 0].min() - 1.5                   # the other obstacles keep their distance from the moved agent
            obs[i, 4, 0:2] = [-1e-170, X[i, 1] + 3.0]
        elif kind == NAN_ROW:
            obs[i, 3, 0:6] = np.nan                                    # the flag stays a circle's
        elif kind in (PAR_BELOW, PAR_ABOVE):                           # two centres on bearings delta apart, delta by the linear rule
            X[i, 2:4] = [0.3, 0.5]
            want = BELOW if kind == PAR_BELOW else ABOVE
            delta = 1e-9
            for _ in range(3):
                for r, rho, rad, d in zip(PAIR_ROWS, (1.25, 1.3), (0.5, 0.7), (0.0, delta)):
                    th = X[i, 2] + 0.4 + d
                    obs[i, r, 0:3] = [X[i, 0] + rho * np.cos(th), X[i, 1] + rho * np.sin(th), rad]
                delta *= want / cross_of(X, obs, i, PAIR_ROWS)
            u_ref[i] = [0.5, 0.1]                                      # closing on the pair, asked to accelerate: both rows violated at u_box
        elif kind == PAR_EXACT:                                        # one centre, two radii: identical normals, both rows violated
            X[i, 2:4] = [0.3, 0.5]
            th = X[i, 2] + 0.4
            for r, rad in zip(PAIR_ROWS, (0.5, 0.7)):
                obs[i, r, 0:3] = [X[i, 0] + 1.25 * np.cos(th), X[i, 1] + 1.25 * np.sin(th), rad]
            u_ref[i] = [0.5, 0.1]
    return X, u_ref, obs


def stored(a, io):
    """What the kernel sees of an input array: rounded to the storage type."""
    with np.errstate(under="ignore"):
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
    """By the numpy oracle, per storage type: what each constructed agent is; numpy and C oracle agree on every agent."""
    X, u_ref, obs = (stored(a, io) for a in batch(B))
    sp = spec()
    c = CB.conditions(X, u_ref, obs, sp)
    kinds = constructed(B)
    r0, r1 = PAIR_ROWS
    for i, kind in kinds.items():
        npar = int(np.triu(c["par"][i]).sum())
        if kind == SUPER_ONE:
            assert c["noncircle"][i].sum() == 1 and not c["bad"][i].any()
        elif kind == SUPER_ALL:
            assert c["noncircle"][i].all() and not c["bad"][i].any()
        elif kind == BAD_AND_SUPER:
            assert c["bad"][i].sum() == 1 and c["noncircle"][i].sum() == 2
        elif kind in (ZERO_ROW, UNDERFLOW):
            n4 = CB.unit_rows(X[i:i + 1], obs[i:i + 1], sp)[0][0, 4]
            print(f"B={B} {io} agent {i}: row 4 = {n4.tolist()}")
            assert c["degenerate"][i, 4] and c["degenerate"][i].sum() == 1
            if kind == UNDERFLOW and io == "f64":
                assert n4[0] != 0.0 and n4[1] == 0.0, "a nonzero normal whose squares underflow"
            else:
                assert n4[0] == 0.0 and n4[1] == 0.0, "an all-zero row"
        elif kind == NAN_ROW:
            assert c["degenerate"][i, 3] and c["degenerate"][i].sum() == 1
        elif kind in (PAR_BELOW, PAR_ABOVE):
            x = c["cross"][i, r0, r1]
            print(f"B={B} {io} agent {i}: |n_i x n_j| = {x:.4e} = {x / EPS_PAR:.3f} eps_par, violated rows {np.nonzero(c['viol'][i])[0].tolist()}")
            assert c["viol"][i, [r0, r1]].all(), "both rows of the pair are candidates"
            if io == "f64":
                if kind == PAR_BELOW:
                    assert 0.5 * EPS_PAR <= x < EPS_PAR and c["par"][i, r0, r1] and npar == 1
                else:
                    assert EPS_PAR < x <= 2.0 * EPS_PAR and npar == 0
            else:                                                      # the 1e-12 angle does not survive f32 storage
                assert x > 1e3 * EPS_PAR and npar == 0
        elif kind == PAR_EXACT:
            assert c["cross"][i, r0, r1] <= EPS_PAR and npar == 1 and c["viol"][i, [r0, r1]].all()
        if kind in (ZERO_ROW, UNDERFLOW):                              # a == 0 (or 1e-170) against every other row of the agent
            assert c["par"][i, 4, [r for r in range(8) if r != 4]].all()
    # the waves: exactly one superellipsoid row in wave 0; wave 1 of B = 24 takes no cold side and enters the solve
    assert (obs[:8, :, 6] == 1.0).sum() == 1
    ordinary = [i for i in range(B) if i not in kinds]
    for key in ("flat", "bad", "noncircle", "degenerate"):
        assert not c[key][ordinary].any(), key
    assert not c["par"][ordinary].any()
    if B == 24:
        assert all(i in ordinary for i in range(8, 16)) and c["viol"][8:16].any()
        assert c["noncircle"][16:24].all()
    # which agents set the parallel-partner flag of their wave: a pair with |n_i x n_j| <= eps_par, or a row the kernel zeroes
    # for its invalid flag (a == 0 against every partner).  Every wave enters the solve, so the flag is looked at in each.
    sets_flag = c["par"].any(axis=(1, 2)) | c["bad"].any(axis=1)
    got = {w: [i for i in range(8 * w, min(8 * w + 8, B)) if sets_flag[i]] for w in range((B + 7) // 8)}
    print(f"B={B} {io}: agents that set the parallel-partner flag, by wave: {got}")
    assert {w: a for w, a in got.items() if a} == PAR_TRIGGERS[B, io]
    for w in got:
        assert c["viol"][8 * w:8 * w + 8].any(), f"wave {w} enters the solve"
    # the numpy oracle (per agent, so that the bad row's ValueError stays with its agent) against the C oracle
    for mode in ("cbf", "hard"):
        uo, so, ho = oracle[B, io, mode]
        for i in range(B):
            if kinds.get(i) == BAD_AND_SUPER:
                with pytest.raises(ValueError):
                    ocbf.solve(R.MODEL_DU, X[i], u_ref[i], list(obs[i]), sp, num_obs=8, dt=0.05, cbf_mode=mode)
                assert so[i] == 3 and np.isnan(uo[i]).all()
                continue
            r = ocbf.solve(R.MODEL_DU, X[i], u_ref[i], list(obs[i]), sp, num_obs=8, dt=0.05, cbf_mode=mode)
            assert r["status"] == so[i], f"agent {i} ({mode}): numpy oracle status {r['status']}, C oracle {so[i]}"
            if so[i] == 0:
                assert np.abs(r["u"] - uo[i]).max() <= 1e-7
            hn, hc = np.asarray(r["h"], dtype=np.float64), ho[i]
            assert np.array_equal(np.isnan(hn), np.isnan(hc))
            ok = ~np.isnan(hc)
            assert (np.abs(hn[ok] - hc[ok]) <= 1e-9 * np.maximum(1.0, np.abs(hc[ok]))).all()
        print(f"B={B} {io} {mode}: status {so.tolist()}")
        assert (so == 0).sum() >= B // 2, "most agents are feasible: there is something to compare"


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
    tmp = tmp_path_factory.mktemp("scalarpath")
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
    assert all(sg[i] == 3 for i, kind in kinds.items() if kind == BAD_AND_SUPER)
    ok = (sg == 0) & (so == 0)
    err = np.abs(ug[ok] - uo[ok]).max(axis=1)
    tol_u = 1e-7 if io == "f64" else 2e-6                              # times max(1, largest bound) = 1
    print(f"{key}: max |u - u_oracle| {err.max():.3e} (tolerance {tol_u:g}) over {int(ok.sum())} agents")
    assert (err <= tol_u).all(), f"u: worst {err.max()} at agent {np.nonzero(ok)[0][err.argmax()]}"
    if want_h:
        hg = both["special"][f"{key}.h"].view(ft).astype(np.float64)
        assert np.array_equal(np.isnan(hg), np.isnan(ho)), "h is NaN exactly where the oracle's is (the NaN obstacle)"
        fin = ~np.isnan(ho)
        herr = np.abs(hg[fin] - ho[fin]) / np.maximum(1.0, np.abs(ho[fin]))
        tol_h = 1e-9 if io == "f64" else 2e-6
        print(f"{key}: max relative |h - h_oracle| {herr.max():.3e} (tolerance {tol_h:g})")
        assert (herr <= tol_h).all(), f"h: worst {herr.max()}"
