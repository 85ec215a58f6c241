"""Backend -- mirrors ``psrsigsim/telescope/backend.py``."""
import numpy as np
import torch

from .._units import make_quant, to_value
from ..utils.constants import DM_K_VALUE
from .. import _engine, _lib

__all__ = ['Backend', 'DedispersedPlane']


class DedispersedPlane(object):
    """Result of :meth:`Backend.dedisperse`: the DM-time plane on the device.

    ``data``      torch float32 [nDM, T] (T = N - max_delay), row j the sum over
                  the channels of the signal shifted by ``delays[j]``
    ``dms``       the trial DMs, float64 [nDM] (pc/cm^3)
    ``delays``    the host table, int32 [nDM][C_local] samples
    ``samprate``  sample rate of the series, MHz
    ``ref_freq``  the frequency the delays refer to, MHz
    ``max_delay`` the table's maximum, samples"""

    def __init__(self, data, dms, delays, samprate, ref_freq, max_delay):
        self.data = data
        self.dms = dms
        self.delays = delays
        self.samprate = samprate
        self.ref_freq = ref_freq
        self.max_delay = max_delay

    def __repr__(self):
        return "DedispersedPlane(%d trials x %d samples, ref %.6g MHz)" % (
            self.data.shape[0], self.data.shape[1], self.ref_freq)


class Backend(object):
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

    @staticmethod
    def pfb_coefficients(Nchan, ntap):
        """Prototype filter of :meth:`channelize` (host, float64): ``ntap * L``
        coefficients, L = 2 Nchan.  ``ntap == 1``: all ones (a plain FFT
        filterbank); else ``sinc((i - (T L - 1)/2) / L) * hamming(T L)[i]``,
        scaled so that sum(h^2) = L -- unit-variance white noise then gives
        E|X_k|^2 = L for every ntap."""
        C, T = int(Nchan), int(ntap)
        if C < 1 or T < 1:
            raise ValueError("pfb_coefficients: Nchan %d, ntap %d" % (C, T))
        L = 2 * C
        if T == 1:
            return np.ones(L, dtype=np.float64)
        i = np.arange(T * L, dtype=np.float64)
        h = np.sinc((i - (T * L - 1) / 2.0) / L) * np.hamming(T * L)
        return h * np.sqrt(L / np.sum(h * h))

    @staticmethod
    def _channelize_plan(signal, Nchan, ntap, tscrunch):
        """Validate the arguments of :meth:`channelize` on the host (nothing
        touches the device): returns (C, T, tscrunch, Npol, N, S)."""
        if getattr(signal, "sigtype", None) != "BasebandSignal":
            raise ValueError("channelize takes a BasebandSignal, not %s"
                             % getattr(signal, "sigtype", type(signal).__name__))
        if signal._buf is None and signal._pending is None:
            raise ValueError("signal has no data: call Pulsar.make_pulses first")
        C, T, ts = int(Nchan), int(ntap), int(tscrunch)
        if C != Nchan or T != ntap or ts != tscrunch:
            raise ValueError("channelize: Nchan, ntap and tscrunch are integers")
        if C < 16 or C > 4096 or (C & (C - 1)):
            raise ValueError("channelize: Nchan %d is not a power of two in [16, 4096]" % C)
        if T < 1 or T > 8:
            raise ValueError("channelize: ntap %d outside [1, 8]" % T)
        if ts < 1:
            raise ValueError("channelize: tscrunch %d < 1" % ts)
        fs = signal._samprate_MHz()
        bw = float(to_value(signal.bw, 'MHz'))
        if fs != 2.0 * bw:
            raise ValueError("channelize: sample rate %r MHz is not 2 x the bandwidth %r MHz" % (fs, bw))
        npol = int(signal.Nchan)
        if npol not in (1, 2):
            raise ValueError("channelize: %d polarisation rows (1 or 2)" % npol)
        N = int(signal._ncols)
        M = N // (2 * C) - T + 1
        S = M // ts if M > 0 else 0
        if S < 1:
            raise ValueError("channelize: %d samples hold no output sample of %d spectra of %d points and %d taps"
                             % (N, ts, 2 * C, T))
        return C, T, ts, npol, N, S

    def channelize(self, signal, Nchan, ntap=1, tscrunch=1):
        """Channelise and detect a baseband signal on the device (extension:
        the reference has no counterpart -- its ``BasebandSignal.to_FilterBank``
        and ``Backend.adc`` are stubs).

        ``signal`` is a BasebandSignal with data, sampled at 2 x its bandwidth,
        of 1 or 2 polarisation rows.  With C = Nchan (a power of two in
        [16, 4096]), L = 2 C, T = ntap in [1, 8] and the prototype filter
        h = :meth:`pfb_coefficients` (C, T):

            y_m[j]    = sum_{t<T} h[t L + j] x[(m + t) L + j]
            X_m[k]    = sum_j y_m[j] exp(-2 pi i j k / L)
            out[k][s] = 1/(L tscrunch) sum_pol sum_{m in group s} |X_m[k]|^2

        for k < C (bin 0 kept, the Nyquist bin dropped): a polyphase (T > 1)
        or plain FFT (T = 1) filterbank, squared, summed over polarisations and
        ``tscrunch`` spectra.  Trailing samples and a ragged last group are
        dropped.  One fused kernel (``pss_channelize``): the voltages are read
        once and the powers written once, no host copy.

        Returns a new search-mode FilterBankSignal of C channels (channel k at
        ``fcent - bw/2 + k bw/C``) sampled at ``fs / (L tscrunch)``, with the
        attributes ``make_pulses`` gives a search-mode signal of that length,
        so ``fold_periods`` and search-mode ``PSRFITS.save`` accept it:
        ``sublen`` is the period of the pulsar whose ``make_pulses`` filled the
        voltages and ``nsub = round(tobs / period)``.  Voltages that came by
        another route carry no period; the result is then one subint
        spanning ``tobs`` (``nsub = 1``), and ``_Smax`` is None."""
        C, T, ts, npol, N, S = self._channelize_plan(signal, Nchan, ntap, tscrunch)
        from ..signal import FilterBankSignal
        data = signal.data                                    # flushes pending stages
        h = _engine.to_dev(self.pfb_coefficients(C, T).astype(np.float32))
        fs = signal._samprate_MHz()
        out_rate = fs / (2 * C * ts)
        fb = FilterBankSignal(to_value(signal.fcent, 'MHz'), to_value(signal.bw, 'MHz'), Nsubband=C, fold=False)
        fb._samprate = make_quant(out_rate, 'MHz')            # (set here: the constructor warns below Nyquist)
        # rows on the 16-B grid (a row stride of S rounded up to 4 samples): the
        # kernels that keep their accumulators in registers then store 16 B
        ld_out = (S + 3) // 4 * 4
        out = torch.empty((C, ld_out), dtype=torch.float32, device=data.device)[:, :S]
        rc = _lib.lib().pss_channelize(_engine.ptr(data), npol, N, max(int(data.stride(0)), N), _engine.ptr(h), C, T,
                                       ts, _engine.ptr(out), ld_out, _engine.stream_ptr())
        _lib.check(rc, "channelize")
        fb._buf = out
        fb._ncols = S
        fb._nsamp = S
        fb._pending = None
        tobs = S / (out_rate * 1e6)
        fb._tobs = make_quant(tobs, 's')
        # search mode as Pulsar._make_pow_pulses leaves it: one subint per
        # period of the pulsar the voltages were made with
        P = getattr(signal, "_period_s", None)
        if P:
            fb._sublen = make_quant(P, 's')
            fb._nsub = int(np.round(tobs / P))
        else:
            fb._sublen = fb._tobs
            fb._nsub = 1
        fb._set_draw_norm(df=1)
        fb._Smax = getattr(signal, "_Smax", None)
        fb._dm = signal._dm
        fb._delay = None
        fb._null_error = None
        fb._null_checks = []
        return fb

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
        f_all = np.asarray(to_value(signal.dat_freq, 'MHz'), dtype=np.float64)
        f = np.asarray(to_value(getattr(signal, "local_dat_freq", signal.dat_freq), 'MHz'), dtype=np.float64)
        fref = float(np.max(f_all)) if ref_freq is None else float(to_value(ref_freq, 'MHz'))
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
        if getattr(signal, "sigtype", None) != "FilterBankSignal":
            raise ValueError("dedisperse takes a FilterBankSignal, not %s"
                             % getattr(signal, "sigtype", type(signal).__name__))
        if signal.fold:
            raise ValueError("dedisperse takes a search-mode signal (fold=False): a fold-mode buffer is tiled "
                             "sub-integrations, not a time series")
        if signal._buf is None and signal._pending is None:
            raise ValueError("signal has no data: call Pulsar.make_pulses first")
        dm = np.atleast_1d(np.asarray(to_value(dms, 'pc/cm^3'), dtype=np.float64))
        delays = Backend.dedisperse_delays(signal, dm, ref_freq)
        fref = (float(np.max(np.asarray(to_value(signal.dat_freq, 'MHz'), dtype=np.float64)))
                if ref_freq is None else float(to_value(ref_freq, 'MHz')))
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
        rc = _lib.lib().pss_fold(_engine.ptr(data), _engine.ptr(out), Nf, data.stride(0), Npbins,
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
        rc = _lib.lib().pss_fold_periods(_engine.ptr(data), _engine.ptr(out), Nf, data.stride(0), nbin, nper,
                                         _engine.stream_ptr())
        _lib.check(rc, "fold_periods")
        return out
