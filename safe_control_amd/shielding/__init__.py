"""Safety shields of the reference's shielding/ package on the evade scenario: Gatekeeper and MPS (csrc/shield.hip)."""
from .gatekeeper import BatchedShield, Gatekeeper  # noqa: F401
from .mps import MPS  # noqa: F401
