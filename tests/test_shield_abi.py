"""CPU: the Gatekeeper / MPS entry points (sc_shield_*) reject bad arguments before any HIP call, the header's
sc_shield_params compiles as C99 with the size and offsets of the ctypes mirror, and the host-side counts are the
reference's Python integers."""
import ctypes as C
import os
import subprocess

import numpy as np

from safe_control_amd import _lib
from safe_control_amd.shielding import BatchedShield

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_counts_are_the_references():
    gk = BatchedShield("gatekeeper")
    assert (gk.n_backup, gk.n_nominal, gk.discount_steps) == (120, 100, 5)       # int(12.0 / 0.1), int(10.0 / 0.1), int(0.5 / 0.1)
    assert BatchedShield("gatekeeper", nominal_horizon=0.3).n_nominal == 2         # int(0.3 / 0.1) = int(2.9999999999999996)
    assert BatchedShield("gatekeeper", dt=0.05).discount_steps == 5
    assert gk.state_bytes(1) == 100 * 16 + 56                                     # about 1.7 KB per agent


def test_argument_validation_without_gpu():
    lib = _lib.load()
    buf = np.zeros(4096)
    ptr = buf.ctypes.data
    iptr = np.zeros(64, dtype=np.int32).ctypes.data
    sh = BatchedShield("gatekeeper")
    p = sh.params()
    assert lib.sc_shield_state_bytes(C.byref(p), 4) == 4 * (100 * 16 + 56)
    assert lib.sc_shield_state_bytes(None, 4) == 0
    assert lib.sc_shield_step_batch(C.byref(p), 0, *([None] * 10), None) == 0                          # B == 0
    assert lib.sc_shield_step_batch(None, 1, ptr, ptr, None, None, ptr, ptr, None, None, None, None, None) == 1
    assert lib.sc_shield_step_batch(C.byref(p), -1, ptr, ptr, None, None, ptr, ptr, None, None, None, None, None) == 1
    assert lib.sc_shield_step_batch(C.byref(p), 1, None, ptr, None, None, ptr, ptr, None, None, None, None, None) == 1   # X NULL
    assert lib.sc_shield_step_batch(C.byref(p), 1, ptr, ptr, None, None, None, ptr, None, None, None, None, None) == 1   # state NULL
    assert lib.sc_shield_step_batch(C.byref(p), 1, ptr, ptr, ptr, None, ptr, ptr, None, None, None, None, None) == 1    # nominal_u missing
    for field, bad, code in (("algo", 2, 1), ("n_nominal", 101, 1), ("n_nominal", -1, 1), ("max_nominal", 513, 2), ("n_backup", -1, 1),
                             ("discount_steps", 0, 1), ("predict_bullet", 2, 1), ("event_offset", float("nan"), 1)):
        q = sh.params()
        setattr(q, field, bad)
        assert lib.sc_shield_step_batch(C.byref(q), 1, ptr, ptr, None, None, ptr, ptr, None, None, None, None, None) == code, field
        assert lib.sc_shield_state_bytes(C.byref(q), 1) == 0, field
    q = sh.params()
    q.base.io_dtype = 7
    assert lib.sc_shield_step_batch(C.byref(q), 1, ptr, ptr, None, None, ptr, ptr, None, None, None, None, None) == 1
    q = sh.params()
    q.base.dt = 0.0
    assert lib.sc_shield_step_batch(C.byref(q), 1, ptr, ptr, None, None, ptr, ptr, None, None, None, None, None) == 1
    q = sh.params()
    q.base.pocket_x_max = q.base.pocket_x_min
    assert lib.sc_shield_step_batch(C.byref(q), 1, ptr, ptr, None, None, ptr, ptr, None, None, None, None, None) == 1
    # the closed loop
    assert lib.sc_shield_rollout_batch(C.byref(p), 1, -1, 0, ptr, ptr, ptr, ptr, None, iptr, iptr, None, None) == 1     # n_ctrl < 0
    assert lib.sc_shield_rollout_batch(C.byref(p), 1, 1, 0, ptr, ptr, ptr, ptr, None, None, iptr, None, None) == 1      # ret NULL
    assert lib.sc_shield_rollout_batch(C.byref(p), 0, 5, 0, *([None] * 8), None) == 0
    q = sh.params(bullet_shared=True)
    assert lib.sc_shield_rollout_batch(C.byref(q), 1, 1, 0, ptr, ptr, ptr, ptr, None, iptr, iptr, None, None) == 1     # shared bullet


def test_header_struct_matches_the_mirror(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safe_control_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(sc_shield_params), offsetof(sc_shield_params, event_offset),\n'
                   '         offsetof(sc_shield_params, base), offsetof(sc_shield_params, predict_bullet), SC_SHIELD_GATEKEEPER, SC_SHIELD_MPS,\n'
                   '         SC_SHIELD_MAX_NOMINAL);\n  return 0;\n}\n')
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S = _lib.ShieldParams
    assert got == [C.sizeof(S), S.event_offset.offset, S.base.offset, S.predict_bullet.offset, _lib.SHIELD_GATEKEEPER, _lib.SHIELD_MPS,
                   _lib.SHIELD_MAX_NOMINAL]
