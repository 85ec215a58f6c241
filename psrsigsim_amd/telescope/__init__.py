from .telescope import Telescope, GBT, Arecibo  # noqa: F401
from .receiver import Receiver, response_from_data  # noqa: F401
from .backend import Backend, DedispersedPlane, BoxcarPlane, PulseCandidates  # noqa: F401
from .backend import HarmonicPlane, PeriodCandidates, FoldedCandidates  # noqa: F401
from .backend import AccelPlane, AccelCandidates  # noqa: F401
from . import telescope  # noqa: F401
