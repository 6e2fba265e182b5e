#!/usr/bin/env python3
"""How many waves of a DynamicUnicycle2D CBF-QP batch leave the fast path of cbfqp_coop8_du_kernel, and why.

CPU only.  The rows come from oracle/cbf_qp.assemble_rows on the storage-rounded (f32) inputs, are normalised as the kernel
normalises them, and are grouped as the kernel groups them: 8 agents of 8 rows per wave.  The kernel's fast path takes every lane
as ordinary; a wave leaves it for the generic K = 8 sequence
  * through the early exit when some row's flag is not 0 (a superellipsoid, or a flag that is neither 0 nor 1: the bad obstacle)
    or some agent has not |theta| < 1e5,
  * through the late exit when some row has not nn > 0 -- an all-zero row, a normal whose squares underflow, a NaN (in every wave,
    entering the solve or not) -- or, in a wave that enters the solve (some row violated at u_box = clamp(u_ref)), when a unit
    normal of ANY of its rows has a component that is exactly 0.0 (a flat direction of the box clip) or two rows of one agent have
    |n_i x n_j| <= eps_par (1e-12: a parallel partner).
The parallel-partner flag of the kernel is min over the seven partners of |a| <= eps_par, a = n_partner . d_line, which is
|n_i x n_j| of the unit normals.  The oracle's rows differ from the kernel's in the last bits (its sincos is the C library's), so
a pair that sits within a few ulp of eps_par could be counted differently; the smallest |n_i x n_j| and the smallest |component|
of the batch are printed so that the distance to the thresholds can be seen.  tests/test_cbfqp_straight_path.py asserts that the
benchmark batch meets none of the conditions.

usage: count_coop8_branches.py [--agents 4096] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import cbf_qp as ocbf, robots as R  # noqa: E402
from safe_control_amd import workloads as W  # noqa: E402

EPS_PAR = 1e-12


def unit_rows(X, obs, spec, cbf_mode="cbf"):
    """Normalised rows (n[B, K, 2], c[B, K]) and the bad-row mask of a batch, by the numpy oracle."""
    return unit_rows_nn(X, obs, spec, cbf_mode)[:3]


def unit_rows_nn(X, obs, spec, cbf_mode="cbf"):
    """unit_rows and nn[B, K], the sum of squares each row was normalised by (0 for a bad row: the kernel zeroes it)."""
    B, K = obs.shape[:2]
    n = np.zeros((B, K, 2)); c = np.zeros((B, K)); bad = np.zeros((B, K), dtype=bool); nns = np.zeros((B, K))
    cp = ocbf.default_cbf_param(R.MODEL_DU)
    for i in range(B):
        for r in range(K):
            try:
                A, b, _ = ocbf.assemble_rows(R.MODEL_DU, X[i], [obs[i, r]], spec, cp, 1, 0.05, cbf_mode)
            except ValueError:
                bad[i, r] = True
                continue
            nn = A[0, 0] ** 2 + A[0, 1] ** 2
            s = 1.0 / np.sqrt(nn) if nn > 0 else 1.0
            n[i, r] = A[0] * s
            c[i, r] = b[0] * s
            nns[i, r] = nn
    return n, c, bad, nns


def conditions(X, u_ref, obs, spec, cbf_mode="cbf"):
    """Per agent: violated rows at u_box, rows with an exactly zero component, parallel pairs, bad rows, rows whose flag is not a
    circle's, rows without nn > 0, the matrix of |n_i x n_j|; and the two minima."""
    n, c, bad, nns = unit_rows_nn(X, obs, spec, cbf_mode)
    lo, hi = ocbf.input_bounds(R.MODEL_DU, spec)
    ubox = np.clip(u_ref, lo, hi)
    zero_row = (n[:, :, 0] == 0) & (n[:, :, 1] == 0)
    viol = ((n * ubox[:, None, :]).sum(-1) + c < 0) & ~zero_row & ~bad
    flat = ((n[:, :, 0] == 0) | (n[:, :, 1] == 0)) & ~bad
    cross = np.abs(n[:, :, None, 0] * n[:, None, :, 1] - n[:, :, None, 1] * n[:, None, :, 0])
    K = n.shape[1]
    off = ~np.eye(K, dtype=bool)[None] & ~bad[:, :, None] & ~bad[:, None, :]
    par = (cross <= EPS_PAR) & off
    with np.errstate(invalid="ignore"):
        degenerate = ~(nns > 0)
    return dict(viol=viol, flat=flat, par=par, bad=bad, noncircle=obs[:, :, 6] != 0, degenerate=degenerate, cross=cross, min_cross=float(cross[np.broadcast_to(off, cross.shape)].min()),
                min_comp=float(np.abs(n[~bad]).min()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    X, _, u_ref, obs = W.du_cbfqp_batch(a.agents, 8, seed=a.seed)
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32).astype(np.float64)
    X, u_ref, obs = f32(X), f32(u_ref), f32(obs)
    spec = R.default_spec(R.MODEL_DU); spec.update(a_max=1.0, w_max=0.5, radius=0.25)
    c = conditions(X, u_ref, obs, spec)
    big_theta = ~(np.abs(X[:, 2]) < 1.0e5)
    pad = (-a.agents) % 8
    wave = lambda m: np.concatenate([m, np.zeros(pad, dtype=bool)]).reshape(-1, 8).any(axis=1)
    enters = wave(c["viol"].any(axis=1))
    flat = wave(c["flat"].any(axis=1)) & enters
    par = wave(c["par"].any(axis=(1, 2))) & enters
    bad = wave(c["bad"].any(axis=1))
    noncircle = wave(c["noncircle"].any(axis=1))
    degenerate = wave(c["degenerate"].any(axis=1))
    nv = c["viol"].sum(axis=1)
    print(f"{len(enters)} waves, {int(enters.sum())} enter the solve; violated rows per agent: max {int(nv.max())}, "
          f"{int((nv >= 2).sum())} agents with two or more")
    print(f"waves with a flat direction (late exit): {int(flat.sum())}   (smallest |component| of a unit normal: {c['min_comp']:.3e})")
    print(f"waves with a parallel partner (late exit): {int(par.sum())}   (smallest |n_i x n_j|: {c['min_cross']:.3e}, threshold {EPS_PAR:g})")
    print(f"waves with a bad obstacle (early exit, a flag that is not 0): {int(bad.sum())}")
    print(f"waves with a row that has not nn > 0 (late exit): {int(degenerate.sum())}")
    print(f"waves that hold a flag other than 0 (early exit): {int(noncircle.sum())}")
    print(f"waves that hold an agent without |theta| < 1e5 (early exit): {int(wave(big_theta).sum())}")


if __name__ == "__main__":
    main()
