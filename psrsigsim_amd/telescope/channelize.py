"""Channelize: a baseband signal into a search-mode filterbank on the device."""
import numpy as np
import torch

from .._units import make_quant, to_value
from .. import _engine, _lib


class ChannelizeStage(object):
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
