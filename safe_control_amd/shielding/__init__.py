"""Safety shields of the reference's shielding/ package on the evade scenario: Gatekeeper and MPS (csrc/shield.hip)."""
from .gatekeeper import BatchedShield, Gatekeeper  # noqa: F401
from .mps import MPS  # noqa: F401
from . import drift  # noqa: F401  (the same two shields on the drift-car scenario: csrc/shield_drift.hip)
