"""Dedisperse: a search-mode filterbank into the DM-time plane on the device."""
import numpy as np
import torch

from .._units import to_value
from ..utils.constants import DM_K_VALUE
from .. import _engine, _lib
from .plane import DedispersedPlane


def _check_search_signal(what, signal):
    if getattr(signal, "sigtype", None) != "FilterBankSignal":
        raise ValueError("%s takes a FilterBankSignal, not %s"
                         % (what, getattr(signal, "sigtype", type(signal).__name__)))
    if signal.fold:
        raise ValueError("%s takes a search-mode signal (fold=False): a fold-mode buffer is tiled "
                         "sub-integrations, not a time series" % what)
    if signal._buf is None and signal._pending is None:
        raise ValueError("signal has no data: call Pulsar.make_pulses first")


def _ref_freq(signal, ref_freq):
    """The frequency the delays refer to, MHz: ``ref_freq``, or the largest of the WHOLE band."""
    if ref_freq is None:
        return float(np.max(np.asarray(to_value(signal.dat_freq, 'MHz'), dtype=np.float64)))
    return float(to_value(ref_freq, 'MHz'))


class DedisperseStage(object):
    @staticmethod
    def dedisperse_delays(signal, dms, ref_freq=None):
        """The integer delay table of :meth:`dedisperse` (host only, float64;
        nothing touches the device): int32 [nDM][C_local],

            x[j][c] = DM_K_VALUE * dms[j] * (f_c**-2 - f_ref**-2) [s] * samprate [Hz]
            d[j][c] = int(floor(x[j][c] + 0.5))

        with f_c the channel's entry in ``signal.dat_freq`` -- its lower edge,
        the frequency ``ISM.disperse`` delays it by -- so the DM that was
        injected undoes the sweep to within half a sample per channel.
        ``ref_freq`` (MHz) defaults to the largest ``dat_freq`` of the WHOLE
        band: the shards of a sharded signal (whose rows are
        ``local_dat_freq``) share one reference.  ValueError on an empty
        ``dms``, a negative or non-finite DM, a ``ref_freq`` below a channel
        frequency (negative delays) and a delay that does not fit in int32."""
        dm = np.atleast_1d(np.asarray(to_value(dms, 'pc/cm^3'), dtype=np.float64))
        if dm.ndim != 1 or dm.size < 1:
            raise ValueError("dedisperse: dms is empty or not one-dimensional")
        if not np.all(np.isfinite(dm)) or np.any(dm < 0):
            raise ValueError("dedisperse: a DM is negative or not finite")
        f = np.asarray(to_value(getattr(signal, "local_dat_freq", signal.dat_freq), 'MHz'), dtype=np.float64)
        fref = _ref_freq(signal, ref_freq)
        if not np.isfinite(fref) or fref <= 0 or np.any(f <= 0):
            raise ValueError("dedisperse: frequencies must be positive and finite")
        if np.any(f > fref):
            raise ValueError("dedisperse: ref_freq %r MHz is below a channel frequency (negative delays)" % fref)
        fs_hz = float(to_value(signal.samprate, 'MHz')) * 1e6
        x = DM_K_VALUE * dm[:, None] * (np.power(f, -2.0) - fref ** -2.0)[None, :] * fs_hz
        d = np.floor(x + 0.5)
        if not np.all(np.isfinite(d)) or d.max() > np.iinfo(np.int32).max:
            raise ValueError("dedisperse: a delay does not fit in int32")
        return d.astype(np.int32)

    @staticmethod
    def _dedisperse_plan(signal, dms, ref_freq=None):
        """Validate the arguments of :meth:`dedisperse` on the host (nothing
        touches the device): returns (dms, delays, ref_freq, max_delay, C, N)."""
        _check_search_signal("dedisperse", signal)
        dm = np.atleast_1d(np.asarray(to_value(dms, 'pc/cm^3'), dtype=np.float64))
        delays = DedisperseStage.dedisperse_delays(signal, dm, ref_freq)
        fref = _ref_freq(signal, ref_freq)
        C, N = delays.shape[1], int(signal._ncols)
        max_delay = int(delays.max())
        if max_delay >= N:
            raise ValueError("dedisperse: the largest delay (%d samples) leaves no output sample of %d"
                             % (max_delay, N))
        return dm, delays, fref, max_delay, C, N

    def dedisperse(self, signal, dms, ref_freq=None):
        """Incoherent dedispersion over the trial DMs ``dms`` on the device
        (extension: the reference has no counterpart): the DM-time plane

            plane[j][t] = sum_c data[c][t + d[j][c]],   t < T = N - max(d)

        of a search-mode FilterBankSignal -- from ``make_pulses`` /
        ``ISM.disperse`` / ``observe`` or from :meth:`channelize` -- with
        d = :meth:`dedisperse_delays` (signal, dms, ref_freq).  One kernel
        (``pss_dedisperse``), the exact direct sum in a fixed order, no host
        copy of the data.  For a sharded signal the result is this rank's
        partial sum over its channels.  Returns a :class:`DedispersedPlane`."""
        dm, delays, fref, max_delay, C, N = self._dedisperse_plan(signal, dms, ref_freq)
        data = signal.data                                    # flushes pending stages
        if data.shape[0] != C:
            raise ValueError("dedisperse: %d data rows for %d channel frequencies" % (data.shape[0], C))
        tab = _engine.to_dev(delays)
        T = N - max_delay
        # rows on the 16-B grid, as channelize's: what reads the plane next can load 16 B
        ld_out = (T + 3) // 4 * 4
        out = torch.empty((delays.shape[0], ld_out), dtype=torch.float32, device=data.device)[:, :T]
        rc = _lib.lib().pss_dedisperse(_engine.ptr(data), C, N, max(int(data.stride(0)), N), _engine.ptr(tab),
                                       delays.shape[0], max_delay, _engine.ptr(out), ld_out, _engine.stream_ptr())
        _lib.check(rc, "dedisperse")
        return DedispersedPlane(out, dm, delays, signal._samprate_MHz(), fref, max_delay)
