from .telescope import Telescope, GBT, Arecibo  # noqa: F401
from .receiver import Receiver, response_from_data  # noqa: F401
from .backend import *  # noqa: F401,F403  (Backend and the result classes: backend.__all__)
from . import telescope  # noqa: F401
