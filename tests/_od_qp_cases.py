"""Constructed optimal-decay CBF-QPs, one batch per model, that reach every active set of od_solve (csrc/od_qp.hpp), what
oracle/od_cbf_qp.py makes of them, and a certificate of optimality that does not enumerate.  Host only, seeded;
tests/test_od_qp_cases.py checks the batches here, tests/test_od_qp_cases_gpu.py holds the kernel of csrc/od_cbf_qp.hip to them.

The QP of one agent is  min |u - u_ref|^2 + p1 (w1 - wr1)^2 + p2 (w2 - wr2)^2  s.t.  a.u + e.w + b >= 0,  lo <= u <= hi.
Its solution falls in one of 18 classes: the row inactive or active, times each input free, at its lower or at its upper bound
(CLASSES, named 'inact/lo/free', 'act/hi/hi', ...).  A case counts for a class only with a margin (FREE_MARGIN, MULT_MARGIN,
ROW_MARGIN below), so that a difference of the size of a tolerance cannot move it to a neighbouring class.

Drawing scenes alone does not reach the classes with the row active and an input at a bound, so the reference input is constructed
for the wanted active set: with the row (a, b, e) of a drawn scene, the free inputs' references are drawn, lam = -2 s / den follows
from them (s the row value at the references / bounds, den = sum_free a_j^2 + e1^2/p1 + e2^2/p2), and each fixed input's reference is
put at  bound - lam a_j / 2 -+ an offset,  which makes its bound multiplier twice the offset -- or left at a plain draw around the
box where the row itself pushes that input against its bound.  References stay below UR_MAX in size, and N_FORCED cases per batch
are built at the corner of the box that maximises a.u: the inputs do all they can for the row and the decay variables must move,
the case the controller exists for.  The class a case is filed under is read off the ORACLE's solution afterwards (classify), never
taken from the intent.

Scenes: three in five have the obstacle close (rho = 1.06 .. 2.5 (r + R)) and the agent aimed roughly at it and fast; for the
rel-degree-1 bicycles the obstacle also comes at the agent, which is what fills their corner classes.  The input boxes are tight
(specs()).
"""
import functools
import math

import numpy as np

from oracle import od_cbf_qp as OD, robots as R

DU, KB, C3BF, DPCBF, QUAD2D = "DynamicUnicycle2D", "KinematicBicycle2D", "KinematicBicycle2D_C3BF", "KinematicBicycle2D_DPCBF", "Quad2D"
DU_SE = "DynamicUnicycle2D/superellipsoid"            # the DU batch over superellipsoids [x, y, a, b, n, theta, 1]
MODEL_NAMES = (DU, KB, C3BF, DPCBF, QUAD2D)
KEYS = MODEL_NAMES + (DU_SE,)
SEED = 5
N_PER_CLASS = 16                                       # what the generator aims at; MIN_PER_CLASS is what the tests require
MIN_PER_CLASS = 8
N_FORCED = 12                                          # cases wanted in which the inputs do all they can for the row and the decay must move:
                                                       # the row active at the corner of the box that maximises a.u
N_SCENES = 6000                                        # scene budget per batch
FREE_MARGIN = 0.02                                     # a free input: at least this share of the box width inside the box
MULT_MARGIN = 1e-2                                     # bound multipliers and lam of an active constraint: at least this
ROW_MARGIN = 1e-2                                      # 'row inactive': the row at clamp(u_ref) at least this times rowscale above zero
UR_MAX = 1e3                                           # constructed references stay below this: at 1e6 the tolerances of kernel and oracle (1e-9
                                                       # of the box) are below the rounding of r_j + lam a_j / 2 itself
SNAP = 1e-9                                            # a constraint is read as active within this relative distance
STATES = ("free", "lo", "hi")
CLASSES = tuple(f"{a}/{q0}/{q1}" for a in ("inact", "act") for q0 in STATES for q1 in STATES)
CORNERS = tuple(f"act/{q0}/{q1}" for q0 in ("lo", "hi") for q1 in ("lo", "hi"))
STATUS_BAD_OBSTACLE = 3                                # SC_STATUS_BAD_OBSTACLE: a DU obstacle flag that is neither 0 nor 1


def model_id(key):
    return R.MODEL_NAMES[key.split("/")[0]]


def specs(key):
    """(robot_spec for the batched controller, spec for the oracle): the tight input boxes under which the corners are reached."""
    name = key.split("/")[0]
    if name == DU:
        spec = {"model": name, "a_max": 0.2, "w_max": 0.1, "radius": 0.25}
    elif name == QUAD2D:
        spec = {"model": name, "f_min": 3.0, "f_max": 10.0, "radius": 0.25}
    else:
        spec = {"model": name, "a_max": 0.3, "beta_max": 0.05, "radius": 0.3}
    ospec = R.default_spec(R.MODEL_NAMES[name])
    ospec.update({k: v for k, v in spec.items() if k != "model"})
    return spec, ospec


# ---------------------------------------------------------------------------------------------------------------------------------
# the certificate
# ---------------------------------------------------------------------------------------------------------------------------------
def certificate(D, r, G, c, x, snap=SNAP):
    """KKT check of a candidate x = (u0, u1, w1[, w2]) of  min sum_i D_i (x_i - r_i)^2  s.t.  G x + c >= 0  (row 0 of G the barrier
    row, rows 1..4 the bounds u0 >= lo0, u0 <= hi0, u1 >= lo1, u1 <= hi1), in long double.  Nothing is enumerated: the active set is
    read off x (constraints within `snap`, relative, of zero), the multipliers are recovered for it, and what is left of
    stationarity is measured.

      1. primal feasibility: viol = max_i max(0, -(G x + c)_i / scale_i), scale_i = max(1, |G_i|.|x| + |c_i|).
      2. x is moved ONTO its active set: an input at a bound is set to the bound, then the free variables are moved along
         D^-1 g (g the barrier row) until the row is zero.  The moved point xt meets its active constraints exactly, so
         complementarity holds exactly: mu_i (G xt + c)_i = 0.  shift = |x - xt|_D.
      3. multipliers: lam of the row by least squares over the free variables, weighted by 1/D; mu of an active bound from
         stationarity of its input.  A negative multiplier is replaced by zero, which leaves its amount in the residual
         rho = 2 D (xt - r) - G^T mu.  eps = |rho|_{D^-1}.

    The bound.  The objective is strongly convex with Hessian 2 diag(1, 1, p1, p2).  Let x* be the minimiser with multipliers
    mu* >= 0.  With d = xt - x*, |d|_D^2 = sum D_i d_i^2:
        2 |d|_D^2 = (grad f(xt) - grad f(x*)).d = (G^T mu + rho - G^T mu*).d
                  = mu.(G xt + c) - mu.(G x* + c) - mu*.(G xt + c) + mu*.(G x* + c) + rho.d  <=  rho.d  <=  eps |d|_D
    (first and last product zero by complementarity, the second and third non-negative because mu, mu* >= 0 and both points are
    feasible).  Hence |xt - x*|_D <= eps / 2 and
        |x - x*|_2  <=  |x - x*|_D  <=  shift + eps / 2  =: bound       (every D_i >= 1 here; otherwise divide by sqrt(min D)).
    A zero residual therefore means x IS the minimiser; `bound` is infinite if xt leaves the feasible set (an inactive constraint
    violated), in which case nothing is certified.

    Returns dict(bound, viol, active [5] bool, mu [5] as recovered, before the clip at zero)."""
    L = np.longdouble
    D, r, G, c, x = (np.asarray(a, dtype=np.float64).astype(L) for a in (D, r, G, c, x))
    n = len(D)
    if not np.all(np.isfinite(x)):
        return dict(bound=math.inf, viol=math.inf, active=np.zeros(5, dtype=bool), mu=np.full(5, np.nan))
    scale = np.maximum(L(1), np.abs(G) @ np.abs(x) + np.abs(c))
    res = G @ x + c
    viol = float(max(L(0), np.max(-res / scale)))
    active = np.abs(res) <= L(snap) * scale
    xt = x.copy()
    fixed = []
    for i in range(1, 5):
        if active[i]:
            j = (i - 1) // 2
            xt[j] = -c[i] / G[i, j]
            fixed.append(j)
    free = [j for j in range(n) if j not in fixed]
    g = G[0]
    lam = L(0)
    gg = np.sum(g[free] ** 2 / D[free])
    if active[0] and gg > 0:
        xt[free] = xt[free] - (g @ xt + c[0]) * (g[free] / D[free]) / gg
        lam = np.sum(g[free] * 2 * (xt[free] - r[free])) / gg
    mu_raw = np.zeros(5, dtype=L)
    mu_raw[0] = lam
    grad = 2 * D * (xt - r) - max(lam, L(0)) * g
    for i in range(1, 5):
        if active[i]:
            j = (i - 1) // 2
            mu_raw[i] = grad[j] / G[i, j]
    mu = np.maximum(mu_raw, 0)
    rho = 2 * D * (xt - r) - G.T @ mu
    eps = np.sqrt(np.sum(rho ** 2 / D))
    shift = np.sqrt(np.sum(D * (x - xt) ** 2))
    rt = G @ xt + c
    ok = np.all(rt >= -L(1e-17) * scale)
    bound = float((shift + eps / 2) / np.sqrt(min(L(1), np.min(D)))) if ok else math.inf
    return dict(bound=bound, viol=viol, active=np.asarray(active), mu=mu_raw.astype(np.float64))


def accepts(cert, x, tol):
    """The candidate is feasible to the kernel's own relative tolerance (1e-9) and provably within tol * max(1, |x|max) of the
    minimiser."""
    return cert["viol"] <= 1e-9 and cert["bound"] <= tol * max(1.0, float(np.abs(x).max()))


def classify(D, r, G, c, x):
    """The class of a solution x with its margins, or None if a margin fails."""
    cert = certificate(D, r, G, c, x)
    act, mu = cert["active"], cert["mu"]
    if act[0]:
        row = "act" if mu[0] >= MULT_MARGIN else None
    else:
        cl = np.clip(r[:2], [-c[1], -c[3]], [c[2], c[4]])
        terms = np.concatenate([G[0, :2] * cl, G[0, 2:] * r[2:], c[:1]])
        row = "inact" if terms.sum() >= ROW_MARGIN * max(1.0, np.abs(terms).sum()) else None
    q = []
    for j in range(2):
        lo, hi = -c[1 + 2 * j], c[2 + 2 * j]
        w = hi - lo
        if lo + FREE_MARGIN * w <= x[j] <= hi - FREE_MARGIN * w:
            q.append("free")
        elif act[1 + 2 * j] and mu[1 + 2 * j] >= MULT_MARGIN:
            q.append("lo")
        elif act[2 + 2 * j] and mu[2 + 2 * j] >= MULT_MARGIN:
            q.append("hi")
        else:
            q.append(None)
    if row is None or None in q:
        return None
    return f"{row}/{q[0]}/{q[1]}"


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------
def _scene(key, rng, R_):
    """One agent and its obstacle.  Three in five are close and closing (rho = 1.06 .. 2.5 (r + R), aimed roughly at the obstacle,
    fast; for the rel-degree-1 bicycles the obstacle comes at the agent as well), the others are plain draws."""
    name = key.split("/")[0]
    close = rng.random() < 0.6
    pos = rng.uniform(0.0, 14.0, 2)
    phi = rng.uniform(-math.pi, math.pi)                       # bearing of the obstacle
    aim = phi + (rng.uniform(-0.7, 0.7) if close else rng.uniform(-math.pi, math.pi))
    obs = np.zeros(7)
    if key == DU_SE:
        a, b = rng.uniform(0.3, 1.2, 2)
        big = max(a, b) + R_
        rho = rng.uniform(1.1, 2.0) * big if close else rng.uniform(1.3, 3.0) * big
        obs[2:7] = [a, b, float(rng.choice([4, 6, 10])), rng.uniform(-math.pi, math.pi), 1.0]
    else:
        rad = rng.uniform(0.2, 0.6)
        rho = rng.uniform(1.06, 2.5) * (rad + R_) if close else rng.uniform(1.3, 8.0) * (rad + R_)
        obs[2] = rad
    obs[:2] = pos + rho * np.array([math.cos(phi), math.sin(phi)])
    if name == QUAD2D:
        X = np.zeros(6)
        X[:2], X[2], X[5] = pos, rng.uniform(-0.4, 0.4), rng.uniform(-1.0, 1.0)
        X[3:5] = rng.uniform(0.5, 3.0) * np.array([math.cos(aim), math.sin(aim)]) if close else rng.uniform(-1.5, 1.5, 2)
        return X, obs
    X = np.zeros(4)
    X[:2], X[2] = pos, R.angle_normalize(aim)
    if name == DU:
        X[3] = rng.uniform(0.3, 3.0) if close else rng.uniform(0.0, 1.0)
    else:
        X[3] = rng.uniform(0.2, 3.5)
        if name in (C3BF, DPCBF):                              # moving circles; the close ones come at the agent
            obs[3:5] = rng.uniform(-0.5, 0.5, 2)
            if close:
                obs[3:5] -= rng.uniform(0.0, 3.0) * np.array([math.cos(phi), math.sin(phi)])
    return X, obs


def _construct(rng, g, b, wr, p, lo, hi, target):
    """u_ref for the active set `target` = (row active?, state of u0, state of u1) under the row g = (a0, a1, e1[, e2]), or None."""
    act, q = target[0], target[1:]
    a, e = g[:2], g[2:]
    w = hi - lo
    ur = np.zeros(2)
    free = [j for j in range(2) if q[j] == "free"]
    for j in free:
        ur[j] = rng.uniform(lo[j] + 0.03 * w[j], hi[j] - 0.03 * w[j])
        if act and rng.random() < 0.5:
            # a large coefficient moves a free input by lam a_j / 2 >= MULT_MARGIN |a_j| / 2, more than a tight box is wide: the
            # input can end inside the box only if its reference starts outside
            ur[j] += rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-2.0, 0.0) * abs(a[j])
    off = rng.uniform(0.05, 1.0, 2) * w + 0.01                 # half the bound multiplier
    if not act:
        for j in range(2):
            if q[j] == "lo":
                ur[j] = lo[j] - off[j]
            elif q[j] == "hi":
                ur[j] = hi[j] + off[j]
        terms = np.concatenate([a * np.clip(ur, lo, hi), e * wr, [b]])
        return ur if terms.sum() >= 2 * ROW_MARGIN * max(1.0, np.abs(terms).sum()) else None
    x0 = np.array([ur[j] if q[j] == "free" else (lo[j] if q[j] == "lo" else hi[j]) for j in range(2)])
    s = a @ x0 + e @ wr + b
    den = sum(a[j] ** 2 for j in free) + np.sum(e ** 2 / p)
    if not den > 0:
        return None
    lam = -2.0 * s / den
    if not lam >= 2 * MULT_MARGIN:
        return None
    for j in range(2):
        if q[j] == "free":
            u = ur[j] + 0.5 * lam * a[j]
            if not lo[j] + 0.03 * w[j] <= u <= hi[j] - 0.03 * w[j]:
                return None
        else:
            # at lo the multiplier is 2 (lo - r_j) - lam a_j, at hi it is lam a_j - 2 (hi - r_j): a plain reference (around the box)
            # where the row itself pushes the input against its bound, else just past the threshold.  Half the multiplier is `m`:
            # relative to lam a_j as well, so that the rounding of the inputs to f32 does not eat it
            sgn = -1.0 if q[j] == "lo" else 1.0
            thr = (lo[j] if q[j] == "lo" else hi[j]) - 0.5 * lam * a[j]
            m = off[j] + 1e-3 * abs(lam * a[j])
            plain = rng.uniform(lo[j] - w[j], hi[j] + w[j])
            ur[j] = plain if sgn * (plain - thr) >= m else thr + sgn * m
            if abs(ur[j]) > UR_MAX:
                return None
    return ur


def _solve(key, X, ur, obs, ospec):
    """Oracle solution, status and class of one case: (x or None, status, h, class or None, (D, r, G, c))."""
    m = model_id(key)
    try:
        D, r, G, c, h, P = OD.qp_data(m, X, ur, obs, ospec)
    except ValueError:                                         # DU: an obstacle flag that is neither 0 nor 1
        return None, STATUS_BAD_OBSTACLE, 0.0, None, None
    x, st = OD.solve_diag_qp(D, r, G, c)
    if x is None:
        return None, st, h, None, (D, r, G, c)
    return x, st, h, classify(D, r, G, c, x), (D, r, G, c)


def _pack(key, rows):
    m = model_id(key)
    rel2 = m in R.REL_DEG2
    spec, ospec = specs(key)
    x = np.array([np.full(4, np.nan) if row["x"] is None else (row["x"] if rel2 else np.append(row["x"], 1.0)) for row in rows])
    return dict(key=key, model=m, spec=spec, ospec=ospec, X=np.array([row["X"] for row in rows]),
                u_ref=np.array([row["ur"] for row in rows]), obs=np.array([row["obs"] for row in rows]),
                cls=np.array([row["cls"] for row in rows], dtype=object), u=x[:, :2], omega=x[:, 2:4],
                status=np.array([row["status"] for row in rows], dtype=np.int32), h=np.array([row["h"] for row in rows]),
                qp=[row["qp"] for row in rows])


@functools.lru_cache(maxsize=None)
def cases(key, seed=SEED):
    """The batch of one model (KEYS), shuffled: dict of X [B,nx], u_ref [B,2], obs [B,7], spec (for the controller), ospec (for the
    oracle), model (oracle id); the oracle's u [B,2], omega [B,2] (the inert omega2 of the rel-degree-1 models at its reference 1),
    status [B], h [B]; cls [B], the class of every case (no case is without one); qp, the (D, r, G, c) of every case."""
    rng = np.random.default_rng([seed, KEYS.index(key)])
    m = model_id(key)
    spec, ospec = specs(key)
    lo, hi = OD.input_bounds(m, ospec)
    rows, count, n_forced = [], {k: 0 for k in CLASSES}, 0
    for _ in range(N_SCENES):
        need = sorted((k for k in CLASSES if count[k] < N_PER_CLASS), key=lambda k: (count[k], rng.random()))
        if not need and n_forced >= N_FORCED:
            break
        X, obs = _scene(key, rng, ospec["radius"])
        D, r, G, c, h, P = OD.qp_data(m, X, np.zeros(2), obs, ospec)
        if not (np.all(np.isfinite(G)) and np.isfinite(c[0]) and h != 0.0):
            continue
        forced = "act/" + "/".join("hi" if G[0, j] > 0 else "lo" for j in range(2))      # the corner that maximises a.u
        if n_forced < N_FORCED:
            need = [forced] + need
        for k in need:
            ur = _construct(rng, G[0], c[0], r[2:], D[2:], lo, hi, (k.startswith("act"),) + tuple(k.split("/")[1:]))
            if ur is None:
                continue
            x, st, h, cls, qp = _solve(key, X, ur, obs, ospec)
            if cls is not None and (count[cls] < N_PER_CLASS or (cls == forced and n_forced < N_FORCED)):
                rows.append(dict(X=X, ur=ur, obs=obs, x=x, status=st, h=h, cls=cls, qp=qp))
                count[cls] += 1
                n_forced += cls == forced
            break
    thin = {k for k in CLASSES if 0 < count[k] < MIN_PER_CLASS}      # a class is in the batch with at least MIN_PER_CLASS cases, or not at all
    rows = [row for row in rows if row["cls"] not in thin]
    while len(rows) <= 256 or len(rows) % 256 == 0 or len(rows) % 64 == 0:   # plain draws: inputs around the box, whatever class results
        X, obs = _scene(key, rng, ospec["radius"])
        ur = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo))
        x, st, h, cls, qp = _solve(key, X, ur, obs, ospec)
        if cls is not None and count[cls] >= MIN_PER_CLASS:
            rows.append(dict(X=X, ur=ur, obs=obs, x=x, status=st, h=h, cls=cls, qp=qp))
    rows = [rows[i] for i in rng.permutation(len(rows))]       # lanes of one wave take different branches: never sorted by class
    return _pack(key, rows)


def resolve(c, X=None, u_ref=None, obs=None, has_obs=None):
    """The oracle on the batch `c` with some inputs replaced (has_obs [B]: 0 = solve without the obstacle row): a dict like c."""
    X = c["X"] if X is None else X
    u_ref = c["u_ref"] if u_ref is None else u_ref
    obs = c["obs"] if obs is None else obs
    rows = []
    for i in range(len(X)):
        o = None if has_obs is not None and not has_obs[i] else obs[i]
        x, st, h, cls, qp = _solve(c["key"], X[i], u_ref[i], o, c["ospec"])
        rows.append(dict(X=X[i], ur=u_ref[i], obs=obs[i], x=x, status=st, h=h, cls=cls, qp=qp))
    return _pack(c["key"], rows)


@functools.lru_cache(maxsize=None)
def f32_cases(key, seed=SEED):
    """The batch as f32 storage holds it (as doubles), solved and classified again; the cases whose class changed under the rounding
    are dropped.  Also `kept` [B of cases(key)] bool."""
    c = cases(key, seed)
    r = resolve(c, *(c[k].astype(np.float32).astype(np.float64) for k in ("X", "u_ref", "obs")))
    kept = np.array([a == b for a, b in zip(r["cls"], c["cls"])])
    out = {k: (v[kept] if isinstance(v, np.ndarray) else v) for k, v in r.items()}
    out["qp"] = [q for q, k in zip(r["qp"], kept) if k]
    out["kept"] = kept
    return out


def class_counts(c):
    return {k: int((c["cls"] == k).sum()) for k in CLASSES}


def best_corner(c):
    """Per case, the corner class that maximises a.u over the box (where the inputs do the most for the row)."""
    out = []
    for D, r, G, cc in c["qp"]:
        out.append("act/" + "/".join("hi" if G[0, j] > 0 else "lo" for j in range(2)))
    return np.array(out, dtype=object)
