"""GPU-box tests of bench.py's control flow: the default N = 1 line carries every contract field, and the
N = 2 path (one process per rank, barrier, max-over-ranks) runs end to end.  The box has ONE GPU, so the
two ranks share it and rendezvous over gloo (SC_BENCH_BACKEND=gloo); RCCL itself is exercised only by the
driver's multi-GPU runs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def last_json(out):
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert lines, out
    return json.loads(lines[-1])


def test_single_gpu_line_has_contract_fields():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "2", "--full",
                        "--cpu-seconds", "1", "--no-sweep"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = last_json(r.stdout)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["unit"] == "solves/s" and d["vs_baseline"] is None
    assert d["value"] > 1e5                          # BASELINE target: >= 100k CBF-QP solves/s on one MI355X
    assert set(d["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"}
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["value"] > 0
    assert d["mpc_cbf"]["value"] > 5e3               # BASELINE target: >= 5k MPC-CBF (N = 10) solves/s
    # configs[2] runs in the reference's formulation (kernel 13: multiple shooting, IPOPT's algorithm), the condensed kernel beside it
    assert "mpcdu_ms_kernel" in d["mpc_cbf"]["roofline"]["kernel"] and d["mpc_cbf"]["condensed"]["kernel_ms"] > 0 and d["mpc_cbf"]["condensed"]["same_status"] > 0.99      # (kernel 13)
    assert d["mpc_cbf"]["cpu_baseline"]["cores"] >= 1 and d["mpc_cbf"]["cpu_baseline"]["value"] > 20      # (the compiled multi-core baseline)
    # configs[3] and configs[4] are on the one-GPU line
    assert d["kb_c3bf"]["agents"] == 16384 and d["kb_c3bf"]["ms_per_step"] < 0.5 and d["hetero_fleet"]["agents"] == 65536 and d["hetero_fleet"]["optimal_fraction"] > 0.99
    # every interior-point leg of the line, VTOL2D included, with its VALU-issue roofline and the flag that says whether the committed
    # counters were collected from this tree's kernel sources (tools/collect_profiles.sh after the last csrc change makes it False)
    for leg in ("od_mpc_cbf", "quad3d_mpc_cbf", "quad2d_mpc_cbf", "kinematic_bicycle_mpc_cbf", "vtol_mpc_cbf", "backup_cbf_qp"):
        assert leg in d and d[leg]["kernel_ms"] > 0, leg
        assert d[leg]["roofline"]["bound"] == "valu" and 0.0 < d[leg]["roofline"]["frac"] < 1.0, leg
    assert isinstance(d["stale_rooflines"], (list, int))                                              # (names of up to four such legs, else their number)
    # kernel 13's other robots: Unicycle2D as a leg of its own, the integrators and the bicycle inside their legs
    assert d["unicycle2d_mpc_cbf"]["optimal_fraction"] > 0.99 and d["unicycle2d_mpc_cbf"]["kernel_ms"] < d["unicycle2d_mpc_cbf"]["condensed_ms"]
    for leg in ("double_integrator_mpc_cbf", "single_integrator_mpc_cbf", "kinematic_bicycle_mpc_cbf"):
        assert d[leg]["ms"]["kernel_ms"] > 0 and d[leg]["ms"]["optimal_fraction"] > 0.9, leg
    # (the legs run the reference solver's budget of 3000 iterations as continuation launches; the one-launch time at the round-3
    # limit of 100 rides along)
    assert d["vtol_mpc_cbf"]["optimal_fraction"] > 0.9 and d["vtol_mpc_cbf"]["value"] > 3e3 and d["vtol_mpc_cbf"]["limit_100_ms"] < 150
    assert d["od_vtol_ms_mpc_cbf"]["kernel_ms"] > 0 and d["kinematic_bicycle_c3bf_mpc_cbf"].get("inaccurate", 0.0) <= 0.03


def test_plain_line_is_the_headline_and_dumps_its_outputs(tmp_path):
    """Without --full the line is the headline alone (no CPU baseline, sweep or extra legs); --dump-outputs writes the last timed
    step's outputs, and two runs with the same arguments write the same arrays."""
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        runs.append((last_json(r.stdout), d))
    line = runs[0][0]
    assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["dtype"] == "f64"
    assert line["unit"] == "solves/s" and line["higher_is_better"] is True and line["cpu_baseline"] is None
    assert abs(line["value"] - 4096 * 7 / (line["ms_per_step"] * 7 / 1e3)) / line["value"] < 1e-6
    assert not {"sweep", "mpc_cbf", "kb_c3bf", "hetero_fleet", "collective_leg"} & set(line)
    shapes = {"u": (4096, 2), "status": (4096,), "h": (4096, 8)}
    for name, shape in shapes.items():
        a, b = (np.load(d / f"{name}.npy") for _, d in runs)
        assert a.shape == shape and a.dtype in (np.float32, np.float64), name
        assert np.isfinite(a).all(), name
        np.testing.assert_array_equal(a, b)
    st, u = np.load(runs[0][1] / "status.npy"), np.load(runs[0][1] / "u.npy")
    assert ((st == 0).mean() > 0.5) and set(np.unique(st)) <= {0.0, 1.0, 2.0, 3.0}
    assert (st != 0).any() and (u[st != 0] == 0).all() and (np.abs(u[st == 0]).max(axis=1) > 0).mean() > 0.5
    assert sorted(p.name for p in runs[0][1].iterdir()) == sorted(f"{n}.npy" for n in shapes)


def test_two_rank_flow_on_one_gpu():
    env = dict(os.environ, SC_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29517", os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--steps", "20", "--warmup", "2"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = last_json(r.stdout)
    assert d["n_gpus"] == 2 and d["scaling"] == "weak"
    assert d["config"]["agents_per_gpu"] == 4096
    assert abs(d["value"] - 2 * 4096 * 20 / (d["ms_per_step"] * 20 / 1e3)) / d["value"] < 1e-6


def test_two_rank_heterogeneous_fleet_flow():
    """--workload hetero_fleet (BASELINE configs[4] as far as the reference defines it) on two ranks sharing the GPU:
    512 agents per rank = 1024 in total, half Unicycle2D and half Quad3D, MPC-CBF N = 20."""
    env = dict(os.environ, SC_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29519", os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--workload", "hetero_fleet", "--agents", "512", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = last_json(r.stdout)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["agents_total"] == 1024
    assert d["config"]["unicycle_optimal_fraction"] > 0.8 and d["config"]["quad3d_optimal_fraction"] > 0.5
    assert d["value"] > 5e3


def test_gpus_flag_starts_its_own_ranks():
    """``python bench.py --gpus 2`` with no launcher around it (how a driver would call it): the parent starts the two ranks as a
    child ``torch.distributed.run`` before touching the GPU, relays rank 0's line and exit code; the line says what the process
    group saw.  (One GPU here, so the ranks share it and rendezvous over gloo.)"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SC_BENCH_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "2", "--full"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = last_json(r.stdout)
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["scaling"] == "weak"
    assert "collective_leg" in d and d["collective_leg"]["all_gather_bytes_per_step"] == 16384 * 16


def test_a_failing_rank_fails_the_launch():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SC_BENCH_BACKEND"] = "no-such-backend"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode != 0
