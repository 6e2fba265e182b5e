"""No GPU: the Manipulator2D QP batches of tests/_manip_qp_cases.py reach what they are meant to reach, judged by the oracle
(classes, infeasible kinds, feasibility margins), by the certificate (the oracle's own solutions) and by the replay of the
kernel's loop (branch census).  tests/test_manip_qp_cases_gpu.py runs the kernel of csrc/manip_cbf_qp.hip on the same batches."""
import numpy as np
import pytest

import _manip_qp_cases as C
from oracle import qp as Q

NAMES = ("small", "large")


def test_every_class_has_cases_with_margin():
    """(rank of active CBF normals, active bounds), with margin, over both batches; the bound-heavy classes in the small batch
    alone (six obstacles leave too little of the box free for them)."""
    counts = {n: C.class_counts(n)[0] for n in NAMES}
    for n in NAMES:
        print(n, {f"{k[0]}/{k[1]}": v for k, v in sorted(counts[n].items(), key=str)})
    for cls in C.CLASSES:
        total = sum(counts[n].get((cls, "margin"), 0) for n in NAMES)
        assert total >= C.MIN_PER_CLASS, f"class {cls}: {total} cases with margin"
    for cls in C.BOUND_HEAVY:
        assert counts["small"].get((cls, "margin"), 0) >= C.MIN_PER_CLASS, f"class {cls} in the small batch"
    # an active bound with a zero multiplier (a reference clipped onto the bound) is kept, under its own label
    assert sum(v for n in NAMES for (cls, kind), v in counts[n].items() if kind == "degenerate") >= C.MIN_PER_CLASS
    assert sum(int(np.sum(C.batch(n)["label"] == "clipped")) for n in NAMES) >= C.MIN_PER_CLASS


def test_every_infeasible_kind_has_cases():
    counts = {n: C.class_counts(n)[0] for n in NAMES}
    for kind in C.INFEASIBLE_KINDS:
        total = sum(counts[n].get(("infeasible", kind), 0) for n in NAMES)
        assert total >= C.MIN_PER_CLASS, f"infeasible/{kind}: {total}"


def test_replay_census_reaches_every_branch():
    tots = {n: C.census(n)[0] for n in NAMES}
    for n in NAMES:
        print(n, tots[n])
    drops = {k: sum(tots[n]["drops"][k] for n in NAMES) for k in tots["small"]["drops"]}
    assert drops[(2, "dependent")] >= 8 and drops[(2, "partial")] >= 8
    assert drops[(3, "dependent")] + drops[(3, "partial")] >= 8
    assert drops[(1, "dependent")] + drops[(1, "partial")] == 0      # cannot occur: the most violated row is taken first
    assert sum(tots[n]["dep_infeasible"] for n in NAMES) >= 8
    assert sum(tots[n]["dead"] for n in NAMES) >= 8
    assert all(sum(tots[n]["adds"][q] for n in NAMES) >= 8 for q in (1, 2, 3))
    assert max(tots[n]["max_rounds"] for n in NAMES) >= 6
    assert min(tots[n]["min_budget_left"] for n in NAMES) > 0         # the budget is never reached


@pytest.mark.parametrize("name", NAMES)
def test_replay_agrees_with_the_oracle(name):
    """A guard on the census tool, not on the product: same status everywhere, same minimiser to 1e-12 (measured 2.9e-14)."""
    sols, (_, per) = C.solutions(name), C.census(name)
    worst = 0.0
    for s, r in zip(sols, per):
        assert s["status"] == r["status"]
        if s["status"] == Q.STATUS_OPTIMAL:
            worst = max(worst, float(np.abs(s["u"] - r["u"]).max()))
    print(name, "replay vs oracle", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_oracle_solutions_pass_the_certificate(name):
    bt, sols = C.batch(name), C.solutions(name)
    worst = 0.0
    for i, s in enumerate(sols):
        if s["status"] == Q.STATUS_OPTIMAL:
            ce = C.certificate(s["G"], s["c"], bt["u_ref"][i], s["u"])
            assert ce["viol"] <= 1e-9 and ce["bound"] <= 1e-9, f"case {i}: {ce}"
            worst = max(worst, ce["bound"])
    print(name, "certified distance of the oracle", worst)


def test_certificate_rejects_a_wrong_answer():
    """The certificate measures a displaced point: moved by 1e-6 off the minimiser it certifies no less than ~1e-6 / 2."""
    bt, sols = C.batch("small"), C.solutions("small")
    _, per = C.class_counts("small")
    n = 0
    for i, s in enumerate(sols):
        if per[i][1] != "margin" or per[i][0] == (0, 0):
            continue
        d = np.array([1e-6, -1e-6, 1e-6])
        ce = C.certificate(s["G"], s["c"], bt["u_ref"][i], s["u"] + d)
        assert ce["bound"] >= 4e-7 or ce["viol"] > 1e-9, f"case {i}: {ce}"
        n += 1
    assert n > 50


@pytest.mark.parametrize("name", NAMES)
def test_few_cases_sit_at_the_edge_of_feasibility(name):
    """The GPU tests may excuse a status difference only where |Chebyshev margin| < 1e-6: at most 1 % of a batch may be there."""
    sols = C.solutions(name)
    near = sum(abs(Q.feasibility_margin(s["G"], s["c"])) < 1e-6 for s in sols)
    print(name, "cases within 1e-6 of the edge:", near)
    assert near <= len(sols) // 100
