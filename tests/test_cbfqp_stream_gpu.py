"""Bit identity of the cooperative CBF-QP kernel (csrc/cbf_qp_kernel.hpp, csrc/sc_group.hpp) across the rewrite that shortened
its instruction stream: every output of every case of workloads.cbfqp_stream_cases() must equal, bit for bit, what the build
BEFORE the rewrite returned on an MI355X.  That build's outputs are tests/golden/cbfqp_stream_bits.npz, recorded by
tools/record_cbfqp_stream_bits.py (its docstring names the commit); the reference is never the build under test.

Inputs: the first 203 draws of du_cbfqp_batch(seed=0) -- 25 groups of 8 lanes plus 3 agents, so the last wave and the last group
are partial -- at K = 8, 5, 1 (8 lanes per agent) and 16 (16 lanes), f32 / f64 and f64 / f64 storage / arithmetic, with and without
n_obs (0 and values above K included), a shared obstacle table, the hard mode, a batch where every third agent has one
superellipsoid obstacle (waves mix the two row paths), and one with a duplicated row, an all-zero row and a NaN state.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import c_oracle, cbf_qp as ocbf, robots as R  # noqa: E402
from safe_control_amd import workloads as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_cbfqp_stream_bits as REC  # noqa: E402  (the launch the fixture was recorded with)

GOLDEN = os.path.join(ROOT, "tests", "golden", "cbfqp_stream_bits.npz")
CASES = {c[0]: c for c in W.cbfqp_stream_cases()}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_fixture_holds_every_case(golden):
    assert sorted(golden.files) == sorted(f"{n}.{o}" for n in CASES for o in ("u", "status", "h"))


def test_batch_exercises_the_solve():
    """The rewrite is in the solve, which only runs for agents with a row violated at clamp(u_ref): by the C oracle the 203 draws
    hold at least 40 agents whose answer is not clamp(u_ref) and at least 5 infeasible ones (36 % and 7.5 % of the first 1024)."""
    _, _, _, _, X, u_ref, obs, _ = CASES["k8_f32c64"]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).astype(np.float64)      # what the kernel is given
    spec = R.default_spec(R.MODEL_DU); spec.update(a_max=1.0, w_max=0.5, radius=0.25)
    u, st, _ = c_oracle.cbfqp_batch(R.MODEL_DU, f32(X), f32(u_ref), f32(obs), spec, ocbf.default_cbf_param(R.MODEL_DU))
    box = np.clip(f32(u_ref), [-1.0, -0.5], [1.0, 0.5])
    moved = (st == 0) & (np.abs(u - box).max(axis=1) > 1e-9)
    print(f"oracle: {int(moved.sum())} agents away from clamp(u_ref), {int((st != 0).sum())} infeasible, of {len(st)}")
    assert moved.sum() >= 40
    assert (st != 0).sum() >= 5


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bits_equal_the_recorded_build(name, golden):
    _, io, comp, mode, X, u_ref, obs, n_obs = CASES[name]
    u, st, h = REC.solve_bits(io, comp, mode, X, u_ref, obs, n_obs)
    gu, gs, gh = golden[name + ".u"], golden[name + ".status"], golden[name + ".h"]
    assert u.dtype == gu.dtype and u.shape == gu.shape and h.dtype == gh.dtype and h.shape == gh.shape
    print(f"{name}: u differs at {int((u != gu).sum())}, status at {int((st != gs).sum())}, h at {int((h != gh).sum())} entries")
    assert np.array_equal(st, gs), f"{name}: status differs for agents {np.nonzero(st != gs)[0][:8]}"
    assert np.array_equal(u, gu), f"{name}: u differs for agents {np.nonzero((u != gu).any(axis=1))[0][:8]}"
    assert np.array_equal(h, gh), f"{name}: h differs for agents {np.nonzero((h != gh).any(axis=1))[0][:8]}"
