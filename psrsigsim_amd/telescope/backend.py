"""Backend -- mirrors ``psrsigsim/telescope/backend.py``; the stages of the search pipeline
(extensions) are a module and a class each, inherited here, their names re-exported."""
import torch

from .._units import make_quant, to_value
from .. import _engine, _lib
from .plane import DedispersedPlane, cluster_cells  # noqa: F401
from .channelize import ChannelizeStage
from .dedisperse import DedisperseStage
from .subband import SubbandStage, SubbandPlan  # noqa: F401
from .pulse_search import PulseSearchStage, BoxcarPlane, PulseCandidates, CANDIDATE_DTYPE  # noqa: F401
from .pulse_search import candidates_from_cells  # noqa: F401
from .periodicity import PeriodicityStage, HarmonicPlane, PeriodCandidates, PERIOD_DTYPE  # noqa: F401
from .periodicity import harmonic_log_fap, period_candidates_from_cells  # noqa: F401
from .accel import AccelStage, AccelPlane, AccelCandidates, ACCEL_DTYPE, C_M_S  # noqa: F401
from .fold_candidates import FoldStage, FoldedCandidates, fold_chi2, _fold_best  # noqa: F401
from .rfi import RfiStage, RfiMask, inject_rfi  # noqa: F401
from .whiten import WhitenStage, WhitenPlan  # noqa: F401
from .ffa import FFAStage, FFAPlane, FFACandidates, FFA_DTYPE, ffa_candidates_from_cells  # noqa: F401
from .toa import TOAStage, TOATemplate, TOAs, WidebandTOAs  # noqa: F401

__all__ = ['Backend', 'DedispersedPlane', 'BoxcarPlane', 'PulseCandidates', 'HarmonicPlane', 'PeriodCandidates',
           'FoldedCandidates', 'AccelPlane', 'AccelCandidates', 'RfiMask', 'inject_rfi', 'FFAPlane', 'FFACandidates',
           'SubbandPlan', 'WhitenPlan', 'TOATemplate', 'TOAs', 'WidebandTOAs']


class Backend(ChannelizeStage, RfiStage, DedisperseStage, SubbandStage, PulseSearchStage, WhitenStage, PeriodicityStage,
              AccelStage, FoldStage, FFAStage, TOAStage):
    def __init__(self, samprate=None, name=None):
        self._name = name
        self._samprate = make_quant(samprate, "MHz")

    def __repr__(self):
        return "Backend({:s})".format(self._name)

    @property
    def name(self):
        return self._name

    @property
    def samprate(self):
        return self._samprate

    def adc(self, signal):
        """backend.py:27-31 (unimplemented there too)."""

    def fold(self, signal, pulsar):
        """backend.py:34-49: Npbins = int(P * 2 * signal.samprate);
        sum over the N_fold blocks of Npbins//2 samples that follow the first
        Npbins samples.  As in the reference the reshape only succeeds when
        Nt - Npbins == N_fold * (Npbins//2), else ValueError."""
        data = signal.data
        Nf, Nt = data.shape
        P = float(to_value(pulsar.period, 's'))
        Npbins = int((P * 2 * signal._samprate_MHz()) * 1e6)
        N_fold = Nt // Npbins
        width = min(Nt, Npbins * (N_fold + 1)) - Npbins
        if width != N_fold * (Npbins // 2):
            raise ValueError("cannot reshape array of size %d into shape (%d,%d,%d)"
                             % (Nf * max(width, 0), Nf, N_fold, Npbins // 2))
        out = torch.empty((Nf, Npbins // 2), dtype=torch.float32, device=data.device)
        rc = _lib.lib().pss_fold(_engine.ptr(data), _engine.ptr(out), Nf, _engine.row_stride(data), Npbins,
                                 N_fold, _engine.stream_ptr())
        _lib.check(rc, "fold")
        return out

    def fold_periods(self, signal, pulsar, nbin=None):
        """Corrected fold (extension; the reference's ``fold`` above is only
        valid for exactly four periods): the sum of the signal over its whole
        periods of ``nbin`` samples (default ``int(P * samprate)``, the
        samples per period make_pulses uses), on the device.  Trailing samples
        of an incomplete period are dropped.  Returns [Nchan, nbin] float32."""
        data = signal.data
        Nf, Nt = data.shape
        if nbin is None:
            P = float(to_value(pulsar.period, 's'))
            nbin = int(P * signal._samprate_MHz() * 1e6)
        nbin = int(nbin)
        nper = Nt // nbin if nbin > 0 else 0
        if nbin < 1 or nper < 1:
            raise ValueError("fold_periods: %d samples hold no whole period of %d bins" % (Nt, nbin))
        out = torch.empty((Nf, nbin), dtype=torch.float32, device=data.device)
        rc = _lib.lib().pss_fold_periods(_engine.ptr(data), _engine.ptr(out), Nf, _engine.row_stride(data), nbin, nper,
                                         _engine.stream_ptr())
        _lib.check(rc, "fold_periods")
        return out
