from .amppi import AMPPI  # noqa: F401
from .disco import MultiDISCO  # noqa: F401
from .dual import DualAMPPI, DualSVMPC  # noqa: F401
