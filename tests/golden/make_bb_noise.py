#!/usr/bin/env python
"""Record the amplitude radiometer-noise scale of the reference (TEST
INFRASTRUCTURE ONLY; a companion of make_golden.py, which it leaves alone).

Runs the *unmodified* reference's ``Receiver._make_amp_noise``
(telescope/receiver.py:123-138) under the test-only astropy.units stand-in in
``tests/golden/refshim`` with the normal draws replaced by ones, so the
returned array is the scalar ``norm`` itself, at two geometries: the
reference's own tests/test_telescope.py::test_bb_obs one (default-rate
BasebandSignal, 5-ms default-Gaussian pulsar, 0.01 s) and a small one.

Outputs ``tests/golden/fixtures/bb_noise.{json,npz}``.  Re-run with
``python -B tests/golden/make_bb_noise.py``.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PSS_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "fixtures")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "refshim"))
sys.path.insert(0, REF)

import scipy.stats._continuous_distns as _cd  # noqa: E402

import psrsigsim  # noqa: E402,F401
from psrsigsim.signal.bb_signal import BasebandSignal  # noqa: E402
from psrsigsim.pulsar.pulsar import Pulsar  # noqa: E402
from psrsigsim.telescope.receiver import Receiver  # noqa: E402
from psrsigsim.utils.utils import make_quant  # noqa: E402

_orig_norm = _cd.norm_gen._rvs


def _ones(self, size=None, random_state=None):
    return np.ones(size, dtype=np.float64)


def _v(q):
    return float(q.value) if hasattr(q, "value") else float(q)


GEOMS = {
    # tests/test_telescope.py::test_bb_obs (Receiver default Trec = 35 K, gain 1 K/Jy)
    "bb_obs": dict(fcent=1400, bw=400, sample_rate=None, period=0.005, Smean=10, tobs=0.01, Tsys=None, gain=1.0),
    "small": dict(fcent=1400, bw=0.512, sample_rate=None, period=0.005, Smean=2.5, tobs=0.02, Tsys=25.0,
                  gain=2.5),
}


def main():
    meta, arrays = {"case": "bb_noise", "draws": [], "geoms": {}}, {}
    for tag, g in GEOMS.items():
        sig = BasebandSignal(g["fcent"], g["bw"], sample_rate=g["sample_rate"], Nchan=2)
        psr = Pulsar(g["period"], g["Smean"], name="J1746-0118")
        np.random.seed(7)
        psr.make_pulses(sig, g["tobs"])
        rcvr = Receiver(fcent=g["fcent"], bandwidth=g["bw"], name="Lband")
        Tsys = rcvr.Trec if g["Tsys"] is None else make_quant(g["Tsys"], "K")
        _cd.norm_gen._rvs = _ones
        try:
            noise = rcvr._make_amp_noise(sig, Tsys, make_quant(g["gain"], "K/Jy"), psr)
        finally:
            _cd.norm_gen._rvs = _orig_norm
        noise = np.asarray(noise, dtype=np.float64)
        assert noise.shape == np.shape(sig.data) and np.all(noise == noise.flat[0])
        m = dict(g)
        m.update(norm=float(noise.flat[0]), samprate_MHz=_v(sig.samprate), nsamp=int(sig.nsamp), Smax=_v(sig._Smax),
                 Tsys_K=_v(Tsys), sum_max_profile=float(np.sum(psr.Profiles._max_profile)))
        meta["geoms"][tag] = m
        arrays["norm_" + tag] = np.array([m["norm"]], dtype=np.float64)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "bb_noise.npz"), **arrays)
    with open(os.path.join(OUT, "bb_noise.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True, default=float)
    print("wrote bb_noise", {k: v["norm"] for k, v in meta["geoms"].items()}, file=sys.stderr)


if __name__ == "__main__":
    main()
