"""CPU: the constructed optimal-decay QPs of tests/_od_qp_cases.py.  Every active set of od_solve (csrc/od_qp.hpp) the GPU test
(tests/test_od_qp_cases_gpu.py) claims to reach has to be in the batch with its margin, the oracle has to solve every case (all are
feasible: an obstacle with h != 0, so the decay variable alone satisfies the row), and the certificate -- which enumerates nothing --
has to accept every answer of the oracle and to refuse a wrong one."""
import time

import numpy as np
import pytest

import _od_qp_cases as Q

# corner classes ('row active, both inputs at a bound') the generator leaves empty: none.  The rel-degree-1 bicycles reach all four
# because their close scenes have the obstacle come at the agent (small or negative h, large |b|)
EMPTY_CORNERS = {Q.C3BF: (), Q.DPCBF: ()}
CERT_TOL = 1e-10                                      # the oracle's own answers: f64 rounding, far below the 1e-7 the kernel is held to


def _x(c, i):
    n = len(c["qp"][i][0])
    return np.concatenate([c["u"][i], c["omega"][i]])[:n]


@pytest.mark.parametrize("key", Q.KEYS)
def test_every_class_is_in_the_batch(key):
    t0 = time.perf_counter()
    c = Q.cases.__wrapped__(key)                            # a fresh generation, timed: scenes, construction and the oracle
    dt = time.perf_counter() - t0
    B = len(c["X"])
    counts = Q.class_counts(c)
    print(f"\n{key}: B = {B}, generated in {dt:.2f} s")
    for k in Q.CLASSES:
        print(f"  {k:16s} {counts[k]:3d}")
    assert dt < 60.0                                          # about a second; the limit only catches a generator gone quadratic
    assert B > 256 and B % 256 != 0
    assert all(k is not None for k in c["cls"]) and sum(counts.values()) == B
    assert np.array_equal(c["X"], Q.cases(key)["X"])          # deterministic
    full = [k for k in Q.CLASSES if counts[k] >= Q.MIN_PER_CLASS]
    empty = [k for k in Q.CLASSES if counts[k] == 0]
    assert len(full) + len(empty) == 18, "a class that is not empty has at least 8 cases"
    forced = int((Q.best_corner(c) == c["cls"]).sum())
    print(f"  row active at the corner that maximises a.u (the decay is forced): {forced}")
    if key in (Q.DU, Q.KB, Q.QUAD2D):
        assert not empty
        assert forced >= Q.MIN_PER_CLASS
    elif key in EMPTY_CORNERS:
        assert set(empty) == set(EMPTY_CORNERS[key]) and set(empty) <= set(Q.CORNERS)
        assert forced >= 1
    else:                                                     # DU over superellipsoids: flag 1, layout [x, y, a, b, n, theta, 1]
        assert (c["obs"][:, 6] == 1.0).all() and set(c["obs"][:, 4]) == {4.0, 6.0, 10.0}
        assert all(counts[k] >= Q.MIN_PER_CLASS for k in Q.CLASSES if k.startswith("inact"))
        assert sum(counts[k] >= Q.MIN_PER_CLASS for k in Q.CLASSES if k.startswith("act")) >= 3
    # classes share waves: no run of 64 lanes is of one kind
    for w in range(B // 64):
        assert len(set(c["cls"][64 * w:64 * w + 64])) >= 12


@pytest.mark.parametrize("key", Q.KEYS)
def test_oracle_solves_every_case_and_the_certificate_accepts_it(key):
    c = Q.cases(key)
    n_inf = int((c["status"] != 0).sum())
    worst = {}
    for i, qp in enumerate(c["qp"]):
        x = _x(c, i)
        cert = Q.certificate(*qp, x)
        assert Q.accepts(cert, x, CERT_TOL), (i, c["cls"][i], cert)
        worst[c["cls"][i]] = max(worst.get(c["cls"][i], 0.0), cert["bound"] / max(1.0, np.abs(x).max()))
        assert Q.classify(*qp, x) == c["cls"][i]
    print(f"\n{key}: oracle 'infeasible' on constructed cases: {n_inf}; worst certified distance to the minimiser "
          f"{max(worst.values()):.1e} (scaled)")
    assert n_inf == 0
    assert (c["h"] != 0).all() and np.isfinite(c["h"]).all()


@pytest.mark.parametrize("key", Q.MODEL_NAMES)
def test_f32_rounding_keeps_the_classes(key):
    c, f = Q.cases(key), Q.f32_cases(key)
    dropped = int((~f["kept"]).sum())
    print(f"\n{key}: {dropped} of {len(c['X'])} cases change class under f32 rounding of the inputs ({100.0 * dropped / len(c['X']):.2f} %)")
    assert dropped <= 0.02 * len(c["X"])
    assert (f["status"] == 0).all() and np.array_equal(f["cls"], c["cls"][f["kept"]])
    assert len(f["X"]) == int(f["kept"].sum()) == len(f["qp"])
    for k in Q.CLASSES:                                       # the rounding empties no class
        assert (f["cls"] == k).sum() >= min(Q.MIN_PER_CLASS, (c["cls"] == k).sum())


@pytest.mark.parametrize("key", (Q.DU, Q.DPCBF))
def test_certificate_refuses_what_is_not_the_minimiser(key):
    """The certificate has teeth: a solution moved by 1e-5, the answer of a neighbouring active set and clamp(u_ref) where the row is
    active are all refused at the 1e-7 the kernel is held to, and its bound is a bound: never below the true distance."""
    c = Q.cases(key)
    rng = np.random.default_rng(1)
    for i, (D, r, G, cc) in enumerate(c["qp"]):
        x = _x(c, i)
        n = len(x)
        y = x + 1e-5 * rng.choice([-1.0, 1.0], n) * np.maximum(1.0, np.abs(x))
        y[:2] = np.clip(y[:2], [-cc[1], -cc[3]], [cc[2], cc[4]])
        for cand in (y, np.concatenate([np.clip(r[:2], [-cc[1], -cc[3]], [cc[2], cc[4]]), r[2:]])):
            dist = float(np.abs(cand - x).max())
            if dist <= 1e-9:                                  # the candidate is the minimiser (row inactive: clamp(u_ref) is)
                continue
            cert = Q.certificate(D, r, G, cc, cand)
            assert cert["bound"] >= 0.999 * dist, (i, c["cls"][i], cert["bound"], dist)
            if dist > 1e-6 * max(1.0, np.abs(cand).max()):
                assert not Q.accepts(cert, cand, 1e-7), (i, c["cls"][i], dist, cert)


def test_bad_flag_and_missing_obstacle():
    """resolve(): the statuses the edge tests on the GPU compare with."""
    c = Q.cases(Q.DU)
    obs = c["obs"][:6].copy()
    obs[0, 6], obs[1, 6], obs[2, 6] = 2.0, 0.5, np.nan
    has = np.array([1, 1, 1, 1, 0, 1])
    r = Q.resolve(dict(c), c["X"][:6], c["u_ref"][:6], obs, has)
    assert list(r["status"]) == [Q.STATUS_BAD_OBSTACLE] * 3 + [0, 0, 0]
    lo, hi = Q.OD.input_bounds(c["model"], c["ospec"])
    assert np.array_equal(r["u"][4], np.clip(c["u_ref"][4], lo, hi)) and np.array_equal(r["omega"][4], [1.0, 1.0]) and r["h"][4] == 0.0
    assert np.array_equal(r["u"][5], c["u"][5])
