"""MPS (model predictive shielding) backed by the gfx950 HIP kernel (csrc/shield.hip), on the evade scenario.

``MPS`` keeps the surface of the reference class (shielding/mps.py): the Gatekeeper drop-in's with the MPS constructor
(no nominal horizon, no discount), one candidate with one nominal step per call, and is_using_backup() = the output
differs from nominal_u_traj[0] by 1e-2 or more (mps.py:145-157)."""
from ._shield_host import MpsDropIn
from .gatekeeper import Gatekeeper


class MPS(MpsDropIn, Gatekeeper):
    """Drop-in for shielding.mps.MPS on the evade scenario (one robot per call)."""
