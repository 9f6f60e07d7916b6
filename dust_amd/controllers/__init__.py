from .amppi import AMPPI, BatchAMPPI  # noqa: F401
from .disco import BatchDISCO, DiscoSimResult, MultiDISCO  # noqa: F401
from .dual import BatchDualAMPPI, BatchDualSVMPC, DualAMPPI, DualSVMPC  # noqa: F401
