"""Drop-in name for the reference's scripts/internal/sim_polar_internal.py: the batched sweep of sim_polar.py."""
from .sim_polar import bler_fixed, bler_point, run_polar_simulation  # noqa: F401
