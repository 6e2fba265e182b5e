"""CPU: the drift-car shield entry points (sc_drift_shield_*) exist with their argument types, the state size follows the
documented layout, the header's structs compile as C99 with the size and offsets of the ctypes mirror, and bad arguments
(null pointers, too many obstacles, n_nominal > max_nominal, a curved track) are refused before any HIP call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from safe_control_amd import _lib
from safe_control_amd.shielding.drift import BatchedDriftShield

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_CAR = 120 * 16 + 8 * 8 + 8 + 8 + 16        # committed inputs [C, 2], cursor [8], commit friction, next_event_time, 4 int32


def test_symbols_and_host_counts():
    lib = _lib.load()
    for name in ("sc_drift_shield_state_bytes", "sc_drift_shield_step_batch", "sc_drift_shield_rollout_batch"):
        assert getattr(lib, name).argtypes is not None
    assert lib.sc_drift_shield_step_batch.argtypes[0] == C.POINTER(_lib.DriftShieldParams)
    assert len(lib.sc_drift_shield_step_batch.argtypes) == 15 and len(lib.sc_drift_shield_rollout_batch.argtypes) == 15
    sh = BatchedDriftShield("gatekeeper", "lane_change")
    assert (sh.n_backup, sh.n_nominal, sh.discount_steps) == (60, 120, 5)          # int(3.0 / 0.05), int(6.0 / 0.05), int(0.25 / 0.05)
    assert sh.n_nominal // sh.discount_steps + 2 == 26                               # the example's candidates per event
    assert sh.backup["target_y"] == -4.0 and sh.keeper["target_y"] == 4.0
    assert sh.state_bytes(1) == PER_CAR and sh.state_bytes(7) == 7 * PER_CAR


def test_argument_validation_without_gpu():
    lib = _lib.load()
    ptr = np.zeros(4096).ctypes.data
    iptr = np.zeros(64, dtype=np.int32).ctypes.data
    sh = BatchedDriftShield("mps", "stop")
    p = sh.params(n_static=1, n_moving=2)
    step = lambda q, B=1, X=ptr, fr=ptr, so=ptr, mo=ptr, nx=None, nu=None, st=ptr, u=ptr: lib.sc_drift_shield_step_batch(
        C.byref(q) if q is not None else None, B, X, fr, so, mo, nx, nu, st, u, None, None, None, None, None)
    assert lib.sc_drift_shield_state_bytes(None, 4) == 0
    assert step(p, B=0) == 0
    assert step(None) == 1 and step(p, B=-1) == 1
    assert step(p, X=None) == 1 and step(p, fr=None) == 1 and step(p, st=None) == 1 and step(p, u=None) == 1
    assert step(p, so=None) == 1 and step(p, mo=None) == 1                           # a count without its table
    assert step(p, nx=ptr) == 1                                                      # nominal_u missing
    for field, bad, code in (("algo", 2, 1), ("io_dtype", 7, 1), ("track_type", 1, 2), ("track_type", 2, 2), ("n_nominal", 121, 1),
                             ("n_nominal", -1, 1), ("max_nominal", _lib.DRIFT_MAX_NOMINAL + 1, 2), ("n_backup", -1, 1),
                             ("discount_steps", 0, 1), ("n_static", 9, 2), ("n_moving", 9, 2), ("n_moving", -1, 1), ("n_puddles", 5, 2),
                             ("obs_shared", 2, 1), ("event_offset", float("nan"), 1), ("dt", 0.0, 1), ("m", 0.0, 1),
                             ("track_width", 0.0, 1), ("v_min", 30.0, 1)):
        q = sh.params(n_static=1, n_moving=2)
        setattr(q, field, bad)
        assert step(q) == code, field
        assert lib.sc_drift_shield_state_bytes(C.byref(q), 1) == 0, field
    q = sh.params(n_static=1, n_moving=2)
    q.backup.kind = 5
    assert step(q) == 2
    q = sh.params(n_static=1, n_moving=2)
    q.keeper.kind = _lib.DRIFT_STOP + 7                                              # device-side planning needs a lane keeper
    assert step(q) == 2
    roll = lambda q, n=1, ret=iptr, mo=ptr: lib.sc_drift_shield_rollout_batch(C.byref(q), 1, n, 0, ptr, ptr, ptr, mo, ptr, ptr, None, ret, iptr,
                                                                              None, None)
    assert roll(p, n=-1) == 1 and roll(p, ret=None) == 1 and roll(p, mo=None) == 1
    assert roll(sh.params(n_static=1, n_moving=2, obs_shared=True)) == 1
    assert lib.sc_drift_shield_rollout_batch(C.byref(p), 0, 5, 0, *([None] * 10), None) == 0


def test_refused_compositions_need_no_gpu():
    with pytest.raises(NotImplementedError):
        BatchedDriftShield("gatekeeper", robot_spec={"model": "DoubleIntegrator2D"})
    for tt in ("oval", "l_shape"):
        with pytest.raises(NotImplementedError):
            BatchedDriftShield("gatekeeper", track={"track_type": tt})
    with pytest.raises(NotImplementedError):
        BatchedDriftShield("gatekeeper", backup="evade")
    with pytest.raises(ValueError):
        BatchedDriftShield("backupcbf")


def test_header_structs_match_the_mirror(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safe_control_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(sc_drift_shield_params), sizeof(sc_drift_controller),\n'
                   '         offsetof(sc_drift_shield_params, dt), offsetof(sc_drift_shield_params, puddles),\n'
                   '         offsetof(sc_drift_shield_params, backup), offsetof(sc_drift_shield_params, keeper),\n'
                   '         offsetof(sc_drift_controller, holding_torque), SC_DRIFT_MAX_OBS, SC_DRIFT_MAX_PUDDLES, SC_DRIFT_MAX_NOMINAL);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S, K = _lib.DriftShieldParams, _lib.DriftController
    assert got == [C.sizeof(S), C.sizeof(K), S.dt.offset, S.puddles.offset, S.backup.offset, S.keeper.offset, K.holding_torque.offset,
                   _lib.DRIFT_MAX_OBS, _lib.DRIFT_MAX_PUDDLES, _lib.DRIFT_MAX_NOMINAL]
