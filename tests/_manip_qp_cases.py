"""Batches of single Manipulator2D CBF-QPs that reach every active set and every branch of manip_qp (csrc/manip_cbf_qp.hip),
what oracle/manipulator.py makes of them, a certificate of optimality that does not enumerate, and a numpy restatement of the
kernel's loop that is used ONLY to count which of its branches a batch reaches.  Host only, seeded;
tests/test_manip_qp_cases.py checks the batches here, tests/test_manip_qp_cases_gpu.py holds the kernel to them.

The QP of one arm is  min |u - u_ref|^2  s.t.  G u + c >= 0  with G = [A; I; -I], c = [b; w_max 1]: the CBF rows of
oracle.manipulator.assemble_rows (one per link circle per obstacle, up to num_rows) and the box |u_i| <= w_max.

Batches (batch(name)): 'small' K = 2, num_rows = 50 (one row per lane), 'large' K = 6, num_rows = 150 (three rows per lane).
Scenes are drawn as tests/test_manipulator_gpu.py::random_batch draws them.  Half of the references are drawn uniformly in
+-1.5 w_max ('wide'), which fills the classes with active bounds; the rest come from nominal_input ('nominal'), and those that
nominal_input clips exactly onto a bound are kept under the label 'clipped': an active bound with a zero multiplier is this
controller's everyday degenerate case.  Constructed cases carry their own labels: 'bounds' (small batch: a wide reference redrawn
until its oracle solution has two or three active bounds), 'opposed' (two obstacles either side of link 0, or one beside it
with the reference driving into it: opposed parallel rows).

The class a case is filed under is read off the ORACLE's solution (classify), never taken from the intent.
"""
import functools
import math

import numpy as np

from oracle import manipulator as M
from oracle import qp as Q

W_MAX, KP, RADIUS = 2.0, 5.0, 0.25
SPEC = {"w_max": W_MAX, "Kp": KP, "radius": RADIUS}            # oracle spec; the controller's adds "model": "Manipulator2D"
BASE = (5.0, 3.5)
DT = 0.05
SEED = 11
BATCHES = {"small": dict(K=2, num_rows=50, B=320), "large": dict(K=6, num_rows=150, B=320)}
MIN_PER_CLASS = 8
MULT_MARGIN = 1e-3                                              # multipliers of the active (deduplicated) normals: at least this
SLACK_MARGIN = 1e-3                                             # normalised slack of an inactive row: at least this
FREE_MARGIN = 1e-3                                              # a free input: at least this times w_max inside the box
ACTIVE = 1e-7                                                   # a row / bound is read as active within this (normalised)
SNAP = 1e-9                                                     # certificate: a constraint is held within this, relative
CLASSES = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (3, 0))
BOUND_HEAVY = ((0, 2), (0, 3), (1, 2))
INFEASIBLE_KINDS = ("zero_normal", "opposed", "general")
# the kernel's thresholds (csrc/manip_cbf_qp.hip, sc_math.hpp num<double>::tol_feas)
K_TOL, K_ZZ, K_R, K_BUDGET = 1e-9, 1e-12, 1e-14, 512


# ---------------------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------------------
def _scene(rng, K, touching=0.15):
    obs = np.zeros((K, 7))
    for r in range(K):
        rho = rng.uniform(0.5 if rng.random() < touching else 1.2, 3.8)
        phi = rng.uniform(-np.pi, np.pi)
        obs[r, :3] = [BASE[0] + rho * np.cos(phi), BASE[1] + rho * np.sin(phi), rng.uniform(0.15, 0.5)]
    return obs


def _bounds_active(u):
    return int(np.sum(np.abs(np.abs(u) - W_MAX) <= ACTIVE * W_MAX)) if u is not None else -1


@functools.lru_cache(maxsize=None)
def batch(name):
    """dict(X [B,3], u_ref [B,3], obs [B,K,7], n_obs [B] (all K), label [B] str, K, num_rows, base, spec)."""
    cfg = BATCHES[name]
    K, num_rows, B = cfg["K"], cfg["num_rows"], cfg["B"]
    rng = np.random.default_rng([SEED, K, num_rows])
    X = rng.uniform(-np.pi, np.pi, (B, 3))
    ur = np.zeros((B, 3)); obs = np.zeros((B, K, 7)); label = []
    n_bounds = B // 8 if name == "small" else 0                  # constructed: two or three bounds active
    n_opp = B // 16
    for i in range(B):
        obs[i] = _scene(rng, K)
        goal = np.array(BASE) + rng.uniform(-3, 3, 2)
        if i < n_bounds:
            # redraw the reference until the oracle's solution sits on >= 2 bounds
            # (every third case: all three references outside the box, until all three bounds are active)
            want = 3 if i % 3 == 0 else 2
            for _ in range(40):
                ur[i] = rng.uniform(-1.5 * W_MAX, 1.5 * W_MAX, 3)
                if want == 3:
                    ur[i] = rng.choice([-1.0, 1.0], 3) * rng.uniform(1.05 * W_MAX, 1.5 * W_MAX, 3)
                r = M.solve(X[i], ur[i], list(obs[i]), SPEC, 1.0, num_rows, DT, "cbf", BASE)
                if r["status"] == Q.STATUS_OPTIMAL and _bounds_active(r["u"]) >= want:
                    break
            label.append("bounds")
        elif i < n_bounds + n_opp:
            # link 0 points along X[0]; circles beside it, one on each side (even i) or one with the reference driving into it
            a = X[i, 0]
            s = rng.uniform(0.5, 1.2)                            # distance along link 0 (length 4/3)
            ax, n_ = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])
            rad = rng.uniform(0.2, 0.4)
            off = (RADIUS + rad) * rng.uniform(0.75, 1.0)        # inside the inflated distance sqrt(1.3) (R + r): h < 0
            c0 = np.array(BASE) + s * ax
            obs[i, 0, :3] = [*(c0 + off * n_), rad]
            if i % 2 == 0:
                obs[i, 1, :3] = [*(c0 - off * n_), rad]
                ur[i] = rng.uniform(-1.0, 1.0, 3)
            else:
                obs[i, 1, :3] = [*(np.array(BASE) - 3.5 * ax), 0.2]     # far behind the base: constrains nothing
                ur[i] = rng.uniform(-1.0, 1.0, 3)
            label.append("opposed")
        elif i % 2 == 0:
            ur[i] = rng.uniform(-1.5 * W_MAX, 1.5 * W_MAX, 3)
            label.append("wide")
        else:
            ur[i] = M.nominal_input(X[i], goal, SPEC, BASE)
            label.append("clipped" if np.any(np.abs(ur[i]) == W_MAX) else "nominal")
    return dict(X=X, u_ref=ur, obs=obs, n_obs=np.full(B, K, dtype=np.int32), label=np.array(label), K=K, num_rows=num_rows,
                base=BASE, spec=dict(SPEC))


def full_rows(A, b, w_max=W_MAX):
    """(G, c) of the whole QP: the CBF rows, then u_i + w >= 0 and -u_i + w >= 0."""
    return np.vstack([A, np.eye(3), -np.eye(3)]), np.concatenate([b, np.full(6, float(w_max))])


def used_rows(num_rows, n_obs, circles=25):
    return min(num_rows, int(n_obs) * circles)


@functools.lru_cache(maxsize=None)
def solutions(name, alpha=1.0, mode="cbf", dt=DT, base=BASE):
    """The oracle on every case of a batch (obstacles moved with the base): list of dict(u, status, h, A, b, G, c, rows)."""
    bt = batch(name)
    shift = np.array(base, dtype=np.float64) - np.array(bt["base"])
    out = []
    for i in range(len(bt["X"])):
        ob = bt["obs"][i].copy(); ob[:, :2] += shift
        r = M.solve(bt["X"][i], bt["u_ref"][i], list(ob), bt["spec"], alpha, bt["num_rows"], dt, mode, tuple(base))
        rows = used_rows(bt["num_rows"], bt["n_obs"][i])
        r["rows"] = rows
        r["G"], r["c"] = full_rows(r["A"][:rows], r["b"][:rows], bt["spec"]["w_max"])
        out.append(r)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# classification, read off the oracle's solution
# ---------------------------------------------------------------------------------------------------------------------------------
def _normalised(G, c):
    nrm = np.sqrt(np.einsum("ij,ij->i", G, G))
    ok = nrm > 0
    N = np.zeros_like(G); cn = np.array(c, dtype=np.float64)
    N[ok] = G[ok] / nrm[ok, None]; cn[ok] = c[ok] / nrm[ok]
    return N, cn, ok


def _unique_directions(N, tol=1e-9):
    keep = []
    for i in range(len(N)):
        if not any(np.abs(N[i] - N[j]).max() <= tol for j in keep):
            keep.append(i)
    return keep


def classify(G, c, u_ref, u, status, w_max=W_MAX):
    """(class, kind).  Feasible: class = (rank of the active CBF normals, number of active bounds); kind 'margin' when the
    multipliers of the active normals (NNLS, parallel rows merged) are >= MULT_MARGIN, every inactive row's normalised slack is
    >= SLACK_MARGIN and every free input is >= FREE_MARGIN w_max inside the box; 'degenerate' when all that holds except that an
    active BOUND has a multiplier below the margin (a reference clipped onto the bound); 'marginless' otherwise.
    Infeasible: class = 'infeasible', kind one of INFEASIBLE_KINDS."""
    from scipy.optimize import nnls
    G = np.asarray(G, dtype=np.float64); c = np.asarray(c, dtype=np.float64)
    m = len(c) - 6
    N, cn, ok = _normalised(G, c)
    if status != Q.STATUS_OPTIMAL:
        if np.any(~ok & (c < 0)):
            return "infeasible", "zero_normal"
        idx = np.nonzero(ok)[0]
        Nn, cc = N[idx], cn[idx]
        dots = Nn @ Nn.T
        opp = (dots <= -1.0 + 1e-12) & (cc[:, None] + cc[None, :] < -1e-9)
        return "infeasible", ("opposed" if np.any(opp) else "general")
    sl = N @ u + cn
    cbf_act = [i for i in range(m) if ok[i] and abs(sl[i]) <= ACTIVE]
    cbf_between = [i for i in range(m) if ok[i] and ACTIVE < sl[i] < SLACK_MARGIN]
    bnd_act = [j for j in range(3) if abs(abs(u[j]) - w_max) <= ACTIVE * w_max]
    bnd_between = [j for j in range(3) if j not in bnd_act and abs(u[j]) > w_max * (1.0 - FREE_MARGIN)]
    uniq = [cbf_act[k] for k in _unique_directions(N[cbf_act])] if cbf_act else []
    rank = int(np.linalg.matrix_rank(N[uniq], tol=1e-9)) if uniq else 0
    cls = (rank, len(bnd_act))
    if cbf_between or bnd_between or rank != len(uniq) or rank + len(bnd_act) > 3:
        return cls, "marginless"
    Nb = np.array([(-1.0 if u[j] > 0 else 1.0) * np.eye(3)[j] for j in bnd_act]).reshape(-1, 3)
    Na = np.vstack([N[uniq].reshape(-1, 3), Nb])
    if len(Na) == 0:
        return cls, "margin"
    mu, res = nnls(Na.T, 2.0 * (u - u_ref))
    if res > 1e-6:
        return cls, "marginless"
    if np.all(mu >= MULT_MARGIN):
        return cls, "margin"
    if np.all(mu[: len(uniq)] >= MULT_MARGIN):
        return cls, "degenerate"
    return cls, "marginless"


# ---------------------------------------------------------------------------------------------------------------------------------
# the certificate
# ---------------------------------------------------------------------------------------------------------------------------------
L = np.longdouble


def _solve_ld(Amat, rhs):
    """Gaussian elimination with partial pivoting in long double (numpy.linalg stops at float64); None when singular."""
    A = np.array(Amat, dtype=L); b = np.array(rhs, dtype=L)
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if abs(A[p, k]) <= L(1e-14):
            return None
        if p != k:
            A[[k, p]] = A[[p, k]]; b[[k, p]] = b[[p, k]]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            A[i, k:] -= f * A[k, k:]; b[i] -= f * b[k]
    x = np.zeros(n, dtype=L)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def certificate(G, c, u_ref, u, snap=SNAP):
    """KKT check, in long double, of a candidate u for  min |u - u_ref|^2  s.t.  G u + c >= 0.  Nothing is enumerated.

      1. primal feasibility: viol = max_i max(0, -(G u + c)_i / scale_i), scale_i = max(1, |G_i|.|u| + |c_i|).
      2. the constraints u HOLDS are those with |(G u + c)_i| <= snap scale_i.  Their normals are normalised and rows parallel to
         an earlier one are dropped (the rows of link 0 are all +-e_0 and the joint circles of two links coincide).  NNLS on what
         is left picks the support S+ of the multipliers; further held rows are added to S while they stay independent (rank <= 3).
      3. u is moved ONTO S: ut = u - N_S^T (N_S N_S^T)^-1 (N_S u + c_S); shift = |u - ut|.  The multipliers mu >= 0 of S+ come from
         least squares on  N_S+^T mu = 2 (ut - u_ref); a negative one is replaced by zero, which leaves its amount in the residual
         rho = 2 (ut - u_ref) - N_S+^T mu; eps = |rho|.  ut meets the rows of S+ exactly, so complementarity is exact.

    The bound.  The Hessian is 2 I.  With u* the minimiser, mu* its multipliers and d = ut - u*:
        2 |d|^2 = (grad f(ut) - grad f(u*)).d = (N^T mu + rho - N^T mu*).d
                = mu.(N ut + c) - mu.(N u* + c) - mu*.(N ut + c) + mu*.(N u* + c) + rho.d  <=  rho.d  <=  eps |d|
    (first and last product zero by complementarity, the second and third non-negative: mu, mu* >= 0, both points feasible).
    Hence |ut - u*| <= eps / 2 and |u - u*| <= shift + eps / 2 =: bound.  `bound` is infinite when ut is not feasible to the
    relative tolerance `snap` (nothing is certified then).

    Returns dict(bound, viol, shift, eps, held, mu)."""
    from scipy.optimize import nnls
    G64 = np.asarray(G, dtype=np.float64); c64 = np.asarray(c, dtype=np.float64).reshape(-1)
    ur64 = np.asarray(u_ref, dtype=np.float64).reshape(3)
    bad = dict(bound=math.inf, viol=math.inf, shift=math.inf, eps=math.inf, held=[], mu=np.zeros(0))
    if u is None or not np.all(np.isfinite(np.asarray(u, dtype=np.float64))):
        return bad
    u64 = np.asarray(u, dtype=np.float64).reshape(3)
    Gl, cl, ul, rl = G64.astype(L), c64.astype(L), u64.astype(L), ur64.astype(L)
    scale = np.maximum(L(1), np.abs(Gl) @ np.abs(ul) + np.abs(cl))
    res = Gl @ ul + cl
    viol = float(max(L(0), np.max(-res / scale)))
    nrm = np.sqrt(np.einsum("ij,ij->i", Gl, Gl))
    held = [i for i in np.nonzero(np.abs(res) <= L(snap) * scale)[0] if nrm[i] > 0]
    Nh = np.array([Gl[i] / nrm[i] for i in held], dtype=L).reshape(-1, 3)
    ch = np.array([cl[i] / nrm[i] for i in held], dtype=L)
    keep = _unique_directions(Nh.astype(np.float64))
    held = [held[k] for k in keep]; Nh, ch = Nh[keep], ch[keep]
    g = 2.0 * (u64 - ur64)
    support = []
    if len(held):
        mu0, _ = nnls(Nh.astype(np.float64).T, g)
        support = [k for k in range(len(held)) if mu0[k] > 0][:3]
    S = list(support)
    for k in range(len(held)):
        if k not in S and len(S) < 3 and np.linalg.matrix_rank(Nh[S + [k]].astype(np.float64), tol=1e-9) == len(S) + 1:
            S.append(k)
    ut = ul.copy()
    if S:
        NS = Nh[S]
        y = _solve_ld(NS @ NS.T, NS @ ul + ch[S])
        if y is None:
            return dict(bad, viol=viol)
        ut = ul - NS.T @ y
    shift = float(np.sqrt(np.sum((ul - ut) ** 2)))
    gt = 2 * (ut - rl)
    mu = np.zeros(len(support), dtype=L)
    if support:
        Np = Nh[support]
        y = _solve_ld(Np @ Np.T, Np @ gt)
        if y is None:
            return dict(bad, viol=viol)
        mu = np.maximum(y, L(0))
        rho = gt - Np.T @ mu
    else:
        rho = gt
    eps = float(np.sqrt(np.sum(rho ** 2)))
    scale_t = np.maximum(L(1), np.abs(Gl) @ np.abs(ut) + np.abs(cl))
    viol_t = float(max(L(0), np.max(-(Gl @ ut + cl) / scale_t)))
    bound = shift + eps / 2 if viol_t <= snap else math.inf
    return dict(bound=bound, viol=viol, shift=shift, eps=eps, held=held, mu=np.asarray(mu, dtype=np.float64))


# ---------------------------------------------------------------------------------------------------------------------------------
# the census tool: the kernel's loop in numpy.  It never supplies an expected value.
# ---------------------------------------------------------------------------------------------------------------------------------
def replay(A, b, u_ref, w_max=W_MAX):
    """manip_qp's dual active-set loop (csrc/manip_cbf_qp.hip) on the rows A u + b >= 0 plus the box, with the same thresholds
    (feasibility tolerance K_TOL, zz <= K_ZZ, r > K_R, a budget of K_BUDGET inner steps) and the same tie rule of the arg-min
    (lowest lane, row r in lane r % 64).  Returns the census of one QP: dict(status, u, rounds, adds {q: n}, drops [(q, kind)],
    dep_infeasible, dead, budget_left).  status: 0 optimal, 1 infeasible, 2 budget exhausted."""
    A = np.asarray(A, dtype=np.float64).reshape(-1, 3); b = np.asarray(b, dtype=np.float64).reshape(-1)
    m = len(b)
    N = np.zeros((m + 6, 3)); cc = np.full(m + 6, np.inf)
    out = dict(status=-1, u=None, rounds=0, adds={1: 0, 2: 0, 3: 0}, drops=[], dep_infeasible=False, dead=False, budget_left=K_BUDGET)
    dead = not np.all(np.isfinite(u_ref))
    for r in range(m):
        nn = float(A[r] @ A[r])
        if not (np.isfinite(nn) and np.isfinite(b[r])):
            dead = True
        if nn > 0.0:
            N[r] = A[r] / math.sqrt(nn); cc[r] = b[r] / math.sqrt(nn)
        elif b[r] < -K_TOL * max(1.0, abs(b[r])):
            dead = True
    for k in range(6):
        N[m + k, k >> 1] = -1.0 if k & 1 else 1.0
        cc[m + k] = w_max
    if dead:
        out.update(status=1, dead=True)
        return out
    lane = np.arange(m + 6) % 64
    u = np.array(u_ref, dtype=np.float64)
    An, lam, idx = [], [], []
    budget = K_BUDGET
    while out["status"] < 0:
        mrg = N @ u + cc + K_TOL * np.maximum(1.0, np.abs(cc))
        mn = mrg.min()
        if not mn < 0.0:
            out["status"] = 0
            break
        cand = np.nonzero(mrg == mn)[0]
        pr = int(cand[np.lexsort((cand, lane[cand]))[0]])
        out["rounds"] += 1
        np_, cp = N[pr], cc[pr]
        sp = float(np_ @ u + cp)
        lam_p = 0.0
        while True:
            budget -= 1
            if budget < 0:
                out["status"] = 2
                break
            q = len(An)
            Qm = np.zeros((q, 3)); R = np.zeros((q, q))
            for j in range(q):
                v = An[j].copy()
                for i in range(j):
                    R[i, j] = Qm[i] @ An[j]
                    v = v - R[i, j] * Qm[i]
                R[j, j] = math.sqrt(v @ v)
                Qm[j] = v / R[j, j]
            d = Qm @ np_ if q else np.zeros(0)
            z = np_ - (Qm.T @ d if q else 0.0)
            rr = np.zeros(q)
            for i in range(q - 1, -1, -1):
                rr[i] = (d[i] - R[i, i + 1:] @ rr[i + 1:]) / R[i, i]
            zz = float(z @ z)
            dep = zz <= K_ZZ
            t1, l = math.inf, -1
            for j in range(q):
                if rr[j] > K_R:
                    tj = lam[j] / rr[j]
                    if tj < t1:
                        t1, l = tj, j
            t2 = math.inf if dep else -sp / zz
            if l < 0 and dep:
                out["status"] = 1; out["dep_infeasible"] = True
                break
            t = min(t1, t2)
            lam = [max(lam[j] - t * rr[j], 0.0) for j in range(q)]
            lam_p += t
            if not dep:
                u = u + t * z
                sp += t * zz
            if t2 <= t1:
                An.append(np_.copy()); lam.append(lam_p); idx.append(pr)
                out["adds"][len(An)] += 1
                break
            out["drops"].append((q, "dependent" if dep else "partial"))
            del An[l], lam[l], idx[l]
    out["budget_left"] = budget
    out["u"] = u if out["status"] == 0 else None
    return out


def census(name):
    """Totals of replay over a batch, plus the per-case list."""
    sols = solutions(name)
    bt = batch(name)
    per = [replay(s["A"][: s["rows"]], s["b"][: s["rows"]], bt["u_ref"][i], bt["spec"]["w_max"]) for i, s in enumerate(sols)]
    tot = dict(rounds=sum(p["rounds"] for p in per), max_rounds=max(p["rounds"] for p in per),
               adds={q: sum(p["adds"][q] for p in per) for q in (1, 2, 3)},
               drops={(q, kind): sum(1 for p in per for d in p["drops"] if d == (q, kind)) for q in (1, 2, 3) for kind in ("dependent", "partial")},
               dep_infeasible=sum(p["dep_infeasible"] for p in per), dead=sum(p["dead"] for p in per),
               min_budget_left=min(p["budget_left"] for p in per))
    return tot, per


def class_counts(name, **variant):
    """{(class, kind): count} and the per-case list of (class, kind) of a batch under the oracle."""
    bt = batch(name)
    per = [classify(s["G"], s["c"], bt["u_ref"][i], s["u"], s["status"], bt["spec"]["w_max"]) for i, s in enumerate(solutions(name, **variant))]
    counts = {}
    for k in per:
        counts[k] = counts.get(k, 0) + 1
    return counts, per


# ---------------------------------------------------------------------------------------------------------------------------------
# further scenes for the GPU tests: wave layouts and link geometry
# ---------------------------------------------------------------------------------------------------------------------------------
def active_rows(G, c, u, tol=ACTIVE):
    """Indices of the rows of (G, c) that u holds at equality (normalised slack within tol)."""
    N, cn, ok = _normalised(G, c)
    return [i for i in range(len(c)) if ok[i] and abs(N[i] @ u + cn[i]) <= tol]


@functools.lru_cache(maxsize=None)
def layout_batch(K, num_rows, B=64):
    """B arms with K obstacles each, about a third of them just at or inside the inflated distance of a point on the THIRD link
    (the rest out of reach), so that the rows of the last obstacles -- the last slot of the wave -- are active in some cases;
    references uniform in +-1.5 w_max, so that bounds are active too.  dict(X, u_ref, obs, sols): sols the oracle's solutions."""
    rng = np.random.default_rng([SEED, 7, K, num_rows])
    X = rng.uniform(-np.pi, np.pi, (B, 3))
    ur = rng.uniform(-1.5 * W_MAX, 1.5 * W_MAX, (B, 3))
    obs = np.zeros((B, K, 7))
    for i in range(B):
        P = M.joint_positions(X[i], BASE)
        for r in range(K):
            rad = rng.uniform(0.15, 0.4)
            if rng.random() < (0.35 if K > 2 else 0.7):
                pt = P[2] + rng.uniform(0.3, 1.0) * (P[3] - P[2])
                d = math.sqrt(M.BETA) * (RADIUS + rad) * rng.uniform(0.95, 1.5)
                phi = rng.uniform(-np.pi, np.pi)
                obs[i, r, :3] = [pt[0] + d * math.cos(phi), pt[1] + d * math.sin(phi), rad]
            else:
                rho, phi = rng.uniform(4.6, 6.0), rng.uniform(-np.pi, np.pi)
                obs[i, r, :3] = [BASE[0] + rho * math.cos(phi), BASE[1] + rho * math.sin(phi), rad]
    sols = []
    for i in range(B):
        r = M.solve(X[i], ur[i], list(obs[i]), SPEC, 1.0, num_rows, DT, "cbf", BASE)
        r["rows"] = used_rows(num_rows, K)
        r["G"], r["c"] = full_rows(r["A"][: r["rows"]], r["b"][: r["rows"]])
        sols.append(r)
    return dict(X=X, u_ref=ur, obs=obs, sols=sols)


ARMS = {"short": dict(link_lengths=(1.0, 0.5, 0.25), K=4, num_rows=150),      # steps (6, 3, 2): 14 circles, 56 rows
        "long": dict(link_lengths=(2.0, 1.5, 1.0), K=4, num_rows=100)}        # steps (12, 9, 6): 30 circles; the cap cuts obstacle 3 after
                                                                              # 10 of the 13 circles of its first link


@functools.lru_cache(maxsize=None)
def arm_batch(arm, B=64):
    """Scenes scaled to an arm with other link lengths; half the references wide, half from nominal_input of that arm."""
    cfg = ARMS[arm]
    LL, K, num_rows = cfg["link_lengths"], cfg["K"], cfg["num_rows"]
    reach = float(sum(LL))
    circles = sum(M.link_steps(LL)) + 3
    rng = np.random.default_rng([SEED, 9, int(10 * reach)])
    X = rng.uniform(-np.pi, np.pi, (B, 3))
    ur = np.zeros((B, 3)); obs = np.zeros((B, K, 7))
    for i in range(B):
        for r in range(K):
            rho, phi = rng.uniform(0.35, 1.15) * reach, rng.uniform(-np.pi, np.pi)
            obs[i, r, :3] = [BASE[0] + rho * math.cos(phi), BASE[1] + rho * math.sin(phi), rng.uniform(0.1, 0.35)]
        goal = np.array(BASE) + rng.uniform(-reach, reach, 2)
        ur[i] = rng.uniform(-1.5 * W_MAX, 1.5 * W_MAX, 3) if i % 2 == 0 else M.nominal_input(X[i], goal, SPEC, BASE, LL)
    sols = []
    for i in range(B):
        r = M.solve(X[i], ur[i], list(obs[i]), SPEC, 1.0, num_rows, DT, "cbf", BASE, LL)
        r["rows"] = used_rows(num_rows, K, circles)
        r["G"], r["c"] = full_rows(r["A"][: r["rows"]], r["b"][: r["rows"]])
        sols.append(r)
    return dict(X=X, u_ref=ur, obs=obs, sols=sols, circles=circles, **cfg)
