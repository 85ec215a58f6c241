from .txtfile import TxtFile  # noqa: F401
from .psrfits import PSRFITS, read_psrfits, read_search_data, load_search_signal  # noqa: F401
