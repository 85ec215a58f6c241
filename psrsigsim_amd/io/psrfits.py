"""Fold-mode PSRFITS output (reference: psrsigsim/io/psrfits.py:22-738).

Template mode (the reference's: ``PSRFITS(path, template=..., fits_mode=
'copy')``, what ``Simulation.save_simulation('psrfits')`` calls): the
template's HDUs are copied in order and edited exactly where the reference
edits them (psrfits.py:184-303, 305-424, 485-509):

* PRIMARY: OBSFREQ, OBSBW, CHAN_DM, STT_IMJD / STT_SMJD / STT_OFFS (the
  reference's _gen_metadata arithmetic, float-repr string splits included)
  and BE_DELAY; every other card image verbatim;
* HISTORY row 0: POL_TYPE, NSUB, NPOL, NBIN, NBIN_PRD, TBIN, CTR_FREQ, NCHAN,
  CHAN_BW, DM; the other rows and the header verbatim;
* PSRPARAM: the reference's hard-coded deletions (BINARY, A1, E, ... TZRSITE);
* POLYCO: verbatim -- the reference regenerates it with PINT, which is absent
  from this environment (a warning says so; files are not phase-connected);
* SUBINT: nsub new rows with the template's columns resized to the signal
  (DAT_FREQ / DAT_WTS [nchan], DAT_OFFS / DAT_SCL [nchan npol], DATA
  (NBIN, NCHAN, NPOL) int16 = the reference's ``astype('>i2')`` of the data,
  wrapped exactly as numpy wraps out-of-range values), OFFS_SUB / TSUBINT per
  row, and the header edits EPOCHS, CHAN_BW, POL_TYPE, TBIN, DM, NBIN.

The reference drives pdat/fitsio for this (absent here); this module restates
their effect on the file (parity of the file bytes is therefore unpinned:
tests/test_psrfits.py checks the copied bytes against the template and the
edited values against the reference's formulas).

Without a template a self-written layout of the same SUBINT columns is
written (an extension).  ``read_fits`` parses any FITS file of binary tables
(the reference's template included, for config C4's portrait:
:func:`template_profile`); ``read_psrfits`` returns the primary and SUBINT
parts of it.  The device data is read back once (one D2H copy of the folded
product; in a multi-GPU run gather it first with
``psrsigsim_amd.shard.gather_channels``).

Search mode (``PSRFITS(path, obs_mode="SEARCH")``, no template; an extension:
the reference leaves it a TODO): the float32 [nchan][nsamp] product is
quantised to 8 / 4 / 2 bits and transposed to the file's time-major order on
the device, in chunks of rows (``PSRFITS._save_search``); ``read_search_data``
unpacks such a file on the host, and ``load_search_signal``
(``PSRFITS(path).load_search()``) on the device, into a FilterBankSignal the
search stages take.
"""
import logging
import math

import numpy as np

from .._units import Quantity

__all__ = ["PSRFITS", "read_psrfits", "read_fits", "read_search_data", "load_search_signal",
           "template_profile"]

log = logging.getLogger("psrsigsim_amd")

# SUBINT columns of the reference's template, in its order (the pointing /
# angle columns carry zeros here: no telescope geometry is simulated)
_SUBINT_SCALARS = [("INDEXVAL", "D"), ("TSUBINT", "D"), ("OFFS_SUB", "D"), ("LST_SUB", "D"), ("RA_SUB", "D"),
                   ("DEC_SUB", "D"), ("GLON_SUB", "D"), ("GLAT_SUB", "D"), ("FD_ANG", "E"), ("POS_ANG", "E"),
                   ("PAR_ANG", "E"), ("TEL_AZ", "E"), ("TEL_ZEN", "E"), ("AUX_DM", "D"), ("AUX_RM", "D")]
_NP = {"D": ">f8", "E": ">f4", "I": ">i2", "J": ">i4", "K": ">i8", "B": "u1", "L": "u1", "A": "S1"}

_BLOCK = 2880


def _val(q):
    return q.value if isinstance(q, Quantity) else q


def _card(key, value=None, comment=""):
    if value is None:
        s = key.ljust(80)
    else:
        if isinstance(value, bool):
            v = ("T" if value else "F").rjust(20)
        elif isinstance(value, (int, np.integer)):
            v = str(int(value)).rjust(20)
        elif isinstance(value, (float, np.floating)):
            v = repr(float(value)).upper().rjust(20)       # shortest round-trip, FITS 'E' exponent
        else:
            v = ("'%s'" % str(value).replace("'", "''").ljust(8)).ljust(20)
        s = ("%-8s= %s" % (key, v))
        if comment:
            s += " / " + comment
    if len(s) > 80:
        raise ValueError("FITS card too long: %r" % s)
    return s.ljust(80)


def _header(cards):
    text = "".join(cards) + "END".ljust(80)
    pad = (-len(text)) % _BLOCK
    return (text + " " * pad).encode("ascii")


def _pad(b):
    return b + b"\0" * ((-len(b)) % _BLOCK)


# PSRPARAM lines the reference's _edit_psrfits_header drops (psrfits.py:296-302)
_DELETE_PARAMS = ("BINARY", "A1", "E", "T0", "PB", "OM", "SINI", "M2", "F1", "PMDEC", "PMRA", "TZRMJD",
                  "TZRFRQ", "TZRSITE")


def _card_comment(card):
    """The comment of an 80-char header card (after the '/' that follows the
    value; quotes respected), or ''."""
    v = card[10:]
    q = False
    for k, ch in enumerate(v):
        if ch == "'":
            q = not q
        elif ch == "/" and not q:
            return v[k + 1:].strip()
    return ""


def _set_cards(cards, values):
    """Header card images with ``values`` {key: value} replaced in place
    (keeping each card's comment) or appended when absent; every other card
    image is kept verbatim."""
    out = list(cards)
    for key, val in values.items():
        for n, c in enumerate(out):
            if c[:8].rstrip() == key and c[8:10] == "= ":
                cm = _card_comment(c)
                try:
                    out[n] = _card(key, val, cm)
                except ValueError:                         # value + old comment too long
                    out[n] = _card(key, val)
                break
        else:
            out.append(_card(key, val))
    return out


def _hdu_size(hdr, index):
    """(name, unpadded data bytes) of the HDU with the header ``hdr``, the
    ``index``-th of its file."""
    if "SIMPLE" in hdr:
        size = 0
        if int(hdr.get("NAXIS", 0)) > 0:
            size = abs(int(hdr["BITPIX"])) // 8
            for a in range(1, int(hdr["NAXIS"]) + 1):
                size *= int(hdr["NAXIS%d" % a])
        return "PRIMARY", size
    name = str(hdr.get("EXTNAME", "HDU%d" % index)).strip()
    return name, int(hdr["NAXIS1"]) * int(hdr["NAXIS2"]) + int(hdr.get("PCOUNT", 0))


def _raw_hdus(path):
    """[{name, cards (80-char images, END excluded), hdr (parsed), data
    (bytes, unpadded)}] of a FITS file, in file order."""
    with open(path, "rb") as f:
        buf = f.read()
    out = []
    pos = 0
    while pos < len(buf):
        hdr, end = _parse_header(buf, pos)
        text = buf[pos:end].decode("ascii", errors="replace")
        cards = []
        for k in range(0, len(text), 80):
            c = text[k:k + 80]
            if c[:8].rstrip() == "END":
                break
            cards.append(c)
        name, size = _hdu_size(hdr, len(out))
        out.append({"name": name, "cards": cards, "hdr": hdr, "data": buf[end:end + size]})
        pos = end + -(-size // _BLOCK) * _BLOCK
    return out


def _mjd_fields(ref_MJD, inc_len):
    """STT_IMJD / STT_SMJD / STT_OFFS exactly as the reference's
    _gen_metadata derives them (psrfits.py:206-243), string splitting of the
    float reprs included (make_quant turns ref_MJD into a float64 first)."""
    init_mjd = float(ref_MJD)
    init_frac_s = float("0." + str(init_mjd).split(".")[-1]) * 86400.0       # ('0.' + frac) day -> s
    init_smjd = float(str(init_frac_s).split(".")[0])
    init_offs = float("0." + str(init_frac_s).split(".")[-1])
    inc_len = float(inc_len)
    if inc_len == 0.0:
        next_mjd, next_s, next_frac = init_mjd, init_smjd, init_offs
    else:
        next_mjd = init_mjd + math.floor(inc_len)
        leftover_s = (inc_len - math.floor(inc_len)) * 86400.0
        next_s = init_smjd + math.floor(leftover_s)
        next_frac = init_offs + (leftover_s - math.floor(leftover_s))
    return int(next_mjd), int(next_s), float(next_frac)


def _wrap_i2(x):
    """numpy's ``astype('>i2')`` of the float64 data, the reference's cast
    (psrfits.py:353): truncation toward zero, out-of-range values wrapped as
    numpy does on this host (the values themselves, not a saturating cast)."""
    return np.asarray(x, dtype=np.float64).astype(">i2")


class PSRFITS(object):
    """psrfits.py:22-738: ``PSRFITS(path, obs_mode=None, template=None,
    copy_template=False, fits_mode='copy')``, ``get_signal_params``,
    ``save(signal, pulsar, parfile, MJD_start, segLength, inc_len, ref_MJD,
    usePint, eq_wts)``, ``make_signal_from_psrfits``.

    With a ``template`` (the reference's only mode) the file is the template
    copied HDU by HDU with the reference's edits (psrfits.py:184-303,
    305-424, 485-509): PRIMARY cards from _gen_metadata, HISTORY row 0, the
    PSRPARAM deletions, and a new SUBINT table of ``nsub`` rows.  Every card
    image and table byte the reference does not edit is the template's,
    verbatim.  The reference's pdat/fitsio layer is restated here (absent
    from this environment); the POLYCO table stays the template's because
    the reference regenerates it with PINT, which is absent too (a warning
    says so).  Without a template the self-written layout below is used
    (an extension; see the module docstring)."""

    def __init__(self, path=None, obs_mode=None, template=None, copy_template=False, fits_mode="copy"):
        self._path = path
        self._template = template
        self._fits_mode = fits_mode
        self._hdus = _raw_hdus(template) if template is not None else None
        if obs_mode is None:
            obs_mode = str(self._hdus[0]["hdr"].get("OBS_MODE", "PSR")).strip() if self._hdus else "PSR"
        if obs_mode == "SEARCH" and self._hdus is not None:
            raise NotImplementedError("search-mode output is self-written: the template copy is fold-mode only")
        if obs_mode not in ("PSR", "CAL", "SEARCH"):
            raise NotImplementedError("only fold-mode (PSR) and search-mode (SEARCH) output is written")
        self.obs_mode = obs_mode
        self.nchan = self.nbin = self.npol = self.nrows = self.nsblk = self.nsubint = None
        self.tbin = self.obsfreq = self.obsbw = self.chan_bw = self.tsubint = None

    path = property(lambda self: self._path)

    # -- template access --------------------------------------------------
    def _hdu(self, name):
        for h in self._hdus:
            if h["name"] == name:
                return h
        raise KeyError(name)

    def _records(self, name):
        h = self._hdu(name)
        return np.frombuffer(h["data"], dtype=_table_dtype(h["hdr"]), count=int(h["hdr"]["NAXIS2"]))

    def _psrparam(self, key):
        """psrfits.py:633-640: the value of a PSRPARAM line, or None."""
        for row in self._records("PSRPARAM"):
            tok = bytes(row[0]).split()
            if tok and tok[0].decode() == key:
                return np.float64(tok[1].decode().replace("D", "E"))
        return None

    def get_signal_params(self, signal=None):
        """psrfits.py:533-581."""
        sub = self._hdu("SUBINT")["hdr"] if self._hdus else {}
        if signal is None:
            if not self._hdus:
                raise ValueError("no template to read the parameters from")
            prim = self._hdu("PRIMARY")["hdr"]
            self.nchan, self.tbin, self.nbin = int(sub["NCHAN"]), float(sub["TBIN"]), int(sub["NBIN"])
            self.npol, self.nrows, self.nsblk = int(sub["NPOL"]), int(sub["NAXIS2"]), int(sub["NSBLK"])
            self.obsfreq, self.obsbw, self.chan_bw = float(prim["OBSFREQ"]), float(prim["OBSBW"]), float(sub["CHAN_BW"])
            self.tsubint = float(self._records("SUBINT")["TSUBINT"][0])
        else:
            self.nchan = int(signal.Nchan)
            self.tbin = 1.0 / (float(_val(signal.samprate)) * 1e6)
            self.nbin = int(signal.nsamp / signal.nsub)
            self.npol = int(signal.Npols)
            self.nrows = int(signal.nsub)
            self.nsblk = int(sub.get("NSBLK", 1))
            self.obsfreq, self.obsbw = float(_val(signal.fcent)), float(_val(signal.bw))
            self.chan_bw = float(_val(signal.bw)) / signal.Nchan
            self.tsubint = float(_val(signal.sublen)) if signal.sublen is not None else float(_val(signal.tobs))
        self.nsubint = self.nrows if self.obs_mode == "PSR" else None

    def make_signal_from_psrfits(self):
        """psrfits.py:439-483: a fold-mode FilterBankSignal with the
        template's geometry (sample rate = F0 x NBIN from PSRPARAM)."""
        from ..signal import FilterBankSignal
        self.get_signal_params()
        f, f0 = self._psrparam("F"), self._psrparam("F0")
        if f0 is not None:
            s_rate = f0 * self.nbin * 1e-6
        elif f is not None:
            s_rate = f * self.nbin * 1e-6
        else:
            raise ValueError("No pulsar frequency defined in input fits file.")
        S = FilterBankSignal(fcent=self.obsfreq, bandwidth=self.obsbw, Nsubband=self.nchan, sample_rate=s_rate,
                             dtype=np.float32, fold=True, sublen=self.tsubint)
        S._dat_freq = Quantity(np.atleast_1d(np.asarray(self._records("SUBINT")["DAT_FREQ"][0], dtype=np.float64)),
                               "MHz")
        S._dm = Quantity(self._psrparam("DM"), "pc/cm^3")
        return S

    # -- save ---------------------------------------------------------------
    def save(self, signal, pulsar, parfile=None, MJD_start=56000.0, segLength=60.0, inc_len=0.0,
             ref_MJD=56000.0, usePint=True, eq_wts=True, telescope="GBT", nbits=8, nsblk=4096, scale="minmax",
             clip_sigma=(2.0, 6.0), max_stage_bytes=256 << 20):
        """psrfits.py:305-424 (template) or the self-written layout.  The
        last five arguments belong to search mode (:meth:`_save_search`)."""
        if self.path is None:
            raise ValueError("no output path")
        if self.obs_mode == "SEARCH":
            return self._save_search(signal, pulsar, MJD_start, inc_len, ref_MJD, telescope, nbits, nsblk, scale,
                                     clip_sigma, max_stage_bytes)
        if self._hdus is None:
            return self._save_new(signal, pulsar, MJD_start, inc_len, ref_MJD, eq_wts, telescope)
        if inc_len == 0.0:
            inc_len = MJD_start - ref_MJD
        if self.nbin is None:
            self.get_signal_params(signal)
        if self.obs_mode != "SEARCH":
            self.nsblk = 1
        nsub, nbin, nchan, npol = int(self.nsubint), int(self.nbin), int(self.nchan), int(self.npol)
        stop = nbin * nsub
        data = signal.data
        if hasattr(data, "cpu"):
            data = data[:, :stop].cpu().numpy()
        sim_sig = _wrap_i2(np.asarray(data)[:, :stop])
        if sim_sig.shape[1] < stop:
            raise ValueError("signal holds %d samples per channel, %d subints x %d bins need %d"
                             % (sim_sig.shape[1], nsub, nbin, stop))
        if parfile is None:
            from ..utils import make_par
            print("No parfile provided, creating par file %s_sim.par" % (pulsar.name))
            make_par(signal, pulsar, outpar="%s_sim.par" % (pulsar.name))
            parfile = "%s_sim.par" % (pulsar.name)
        if not usePint:
            raise NotImplementedError("Only PINT is currently supported for generating polycos")
        log.warning("PINT is not available: the template's POLYCO table is kept (polycos for %s not regenerated)",
                    parfile)
        dm = float(_val(signal.dm))
        tbin = float(_val(pulsar.period)) / nbin
        imjd, smjd, offs = _mjd_fields(ref_MJD, inc_len)
        primary = {"OBSFREQ": float(self.obsfreq), "OBSBW": float(self.obsbw), "CHAN_DM": dm, "STT_IMJD": imjd,
                   "STT_SMJD": smjd, "STT_OFFS": offs, "BE_DELAY": 0.0}
        sub_cards = {"EPOCHS": "MIDTIME", "CHAN_BW": float(self.chan_bw), "POL_TYPE": "AA+BB", "TBIN": tbin,
                     "DM": dm, "NBIN": nbin}
        offs_sub = np.array([float(_val(signal.sublen)) / 2.0 + ii * float(_val(signal.sublen))
                             for ii in range(int(signal.nsub))], dtype=np.float64)
        out = []
        for h in self._hdus:
            name = h["name"]
            if name == "PRIMARY":
                out.append((_set_cards(h["cards"], primary), h["data"]))
            elif name == "HISTORY":
                rec = self._records("HISTORY").copy()
                for key, val in (("POL_TYPE", b"AA+BB"), ("NSUB", nsub), ("NPOL", npol), ("NBIN", nbin),
                                 ("NBIN_PRD", nbin), ("TBIN", tbin), ("CTR_FREQ", float(self.obsfreq)),
                                 ("NCHAN", nchan), ("CHAN_BW", float(self.chan_bw)), ("DM", dm)):
                    if key in rec.dtype.names:
                        rec[0][key] = val
                out.append((h["cards"], rec.tobytes()))
            elif name == "PSRPARAM":
                rec = self._records("PSRPARAM")
                keep = [r for r in rec if not (bytes(r[0]).split() and
                                               bytes(r[0]).split()[0].decode() in _DELETE_PARAMS)]
                kept = np.array(keep, dtype=rec.dtype) if keep else np.zeros(0, dtype=rec.dtype)
                out.append((_set_cards(h["cards"], {"NAXIS2": len(kept)}), kept.tobytes()))
            elif name == "SUBINT":
                out.append(self._subint(h, sim_sig, offs_sub, sub_cards, eq_wts, signal))
            else:
                out.append((h["cards"], h["data"]))      # POLYCO and any other table: verbatim
        with open(self.path, "wb") as f:
            for cards, data in out:
                f.write(_header(cards))
                if data:
                    f.write(_pad(bytes(data)))
        print("Finished writing and saving the file")

    def _subint(self, h, sim_sig, offs_sub, sub_cards, eq_wts, signal):
        """The new SUBINT table (pdat set_subint_dims + make_HDU_rec_array:
        the template's columns with DAT_FREQ / DAT_WTS [nchan], DAT_OFFS /
        DAT_SCL [nchan npol], DATA [nbin nchan npol] of nsub zero rows), then
        the reference's per-row assignments (psrfits.py:365-392, 284-287)."""
        hdr = h["hdr"]
        nsub, nbin, nchan, npol = int(self.nsubint), int(self.nbin), int(self.nchan), int(self.npol)
        sizes = {"DAT_FREQ": nchan, "DAT_WTS": nchan, "DAT_OFFS": nchan * npol, "DAT_SCL": nchan * npol,
                 "DATA": nbin * nchan * npol * int(self.nsblk)}
        cards = {}
        fields = []
        for i in range(1, int(hdr["TFIELDS"]) + 1):
            name = str(hdr["TTYPE%d" % i]).strip()
            form = str(hdr["TFORM%d" % i]).strip()
            k = 0
            while k < len(form) and form[k].isdigit():
                k += 1
            code = form[k]
            if name in sizes:
                n = sizes[name]
                cards["TFORM%d" % i] = "%d%s" % (n, code)
                if name == "DATA":
                    cards["TDIM%d" % i] = "(%d,%d,%d)" % (nbin, nchan, npol)
                    fields.append((name, _NP[code], (npol, nchan, nbin)))
                else:
                    fields.append((name, _NP[code], (n,)))
            else:
                n = int(form[:k] or 1)
                fields.append((name, "S%d" % n) if code == "A" else (name, _NP[code], (n,) if n > 1 else ()))
        dt = np.dtype(fields)
        tab = np.zeros(nsub, dtype=dt)
        tmpl = self._records("SUBINT")
        freqs = np.asarray(_val(signal.dat_freq), dtype=np.float64)
        for ii in range(nsub):
            tab[ii]["DATA"] = sim_sig[:, ii * nbin:(ii + 1) * nbin]
            tab[ii]["DAT_FREQ"] = freqs
            qq = min(ii, len(tmpl) - 1)       # more subints than the template: its last row's values
            if eq_wts:
                tab[ii]["DAT_SCL"] = 1.0
                tab[ii]["DAT_OFFS"] = 0.0
                tab[ii]["DAT_WTS"] = 1.0
            else:
                for key in ("DAT_SCL", "DAT_OFFS", "DAT_WTS"):
                    tab[ii][key] = np.resize(np.asarray(tmpl[qq][key]).ravel(), tab[ii][key].shape)
        tab["OFFS_SUB"][:len(offs_sub)] = offs_sub[:nsub]
        tab["TSUBINT"] = float(self.tsubint)
        cards.update({"NAXIS1": dt.itemsize, "NAXIS2": nsub, "NCHAN": nchan, "NPOL": npol, "NSBLK": int(self.nsblk)})
        cards.update(sub_cards)
        return _set_cards(h["cards"], cards), tab.tobytes()

    def _primary_cards(self, signal, pulsar, nchan, dm, MJD_start, inc_len, ref_MJD, telescope):
        """PRIMARY header cards of the self-written layouts."""
        if inc_len == 0.0:
            inc_len = MJD_start - ref_MJD
        # STT_* (psrfits.py:220-244): integer MJD, integer seconds, fraction
        start = ref_MJD + (math.floor(inc_len) if inc_len else 0.0)
        imjd = int(math.floor(start))
        secs = (start - imjd) * 86400.0 + ((inc_len - math.floor(inc_len)) * 86400.0 if inc_len else 0.0)
        smjd = int(math.floor(secs))
        offs = secs - smjd
        return [
            _card("SIMPLE", True, "file conforms to FITS standard"), _card("BITPIX", 8), _card("NAXIS", 0),
            _card("EXTEND", True), _card("HDRVER", "6.1"), _card("FITSTYPE", "PSRFITS"),
            _card("OBS_MODE", self.obs_mode), _card("TELESCOP", telescope), _card("FRONTEND", "sim"),
            _card("BACKEND", "psrsigsim_amd"), _card("FD_POLN", "LIN"), _card("SRC_NAME", str(pulsar.name)),
            _card("OBSFREQ", float(_val(signal.fcent))), _card("OBSBW", float(_val(signal.bw))),
            _card("OBSNCHAN", nchan), _card("CHAN_DM", dm), _card("STT_IMJD", imjd), _card("STT_SMJD", smjd),
            _card("STT_OFFS", offs), _card("BE_DELAY", 0.0),
        ]

    def _save_new(self, signal, pulsar, MJD_start, inc_len, ref_MJD, eq_wts, telescope):
        """The self-written layout (no template; extension)."""
        nchan = int(signal.Nchan)
        npol = 1
        period = float(_val(pulsar.period))
        nbin = int(_val(signal.samprate) * 1e6 * period)          # samples per period, as make_pulses
        nsub = int(signal.nsub)
        sublen = float(_val(signal.sublen)) if signal.sublen is not None else float(_val(signal.tobs))
        data = signal.data
        stop = nbin * nsub
        if hasattr(data, "cpu"):
            data = data[:, :stop].cpu().numpy()
        d16 = _wrap_i2(np.asarray(data)[:, :stop])
        if d16.shape[1] < stop:
            raise ValueError("signal holds %d samples per channel, %d subints x %d bins need %d"
                             % (d16.shape[1], nsub, nbin, stop))
        # [nsub][npol][nchan][nbin] (psrfits.py:357-366)
        out = d16.reshape(nchan, nsub, nbin).transpose(1, 0, 2)[:, None, :, :]
        freqs = np.asarray(_val(signal.dat_freq), dtype=np.float64)[:nchan]
        dm = float(_val(signal.dm)) if getattr(signal, "dm", None) is not None else 0.0
        primary = self._primary_cards(signal, pulsar, nchan, dm, MJD_start, inc_len, ref_MJD, telescope)
        cols = [(n, "1" + c, None) for n, c in _SUBINT_SCALARS]
        cols += [("DAT_FREQ", "%dD" % nchan, None), ("DAT_WTS", "%dE" % nchan, None),
                 ("DAT_OFFS", "%dE" % (nchan * npol), None), ("DAT_SCL", "%dE" % (nchan * npol), None),
                 ("DATA", "%dI" % (nbin * nchan * npol), "(%d,%d,%d)" % (nbin, nchan, npol))]
        row = np.dtype([(n, _NP[c]) for n, c in _SUBINT_SCALARS] +
                       [("DAT_FREQ", ">f8", (nchan,)), ("DAT_WTS", ">f4", (nchan,)),
                        ("DAT_OFFS", ">f4", (nchan * npol,)), ("DAT_SCL", ">f4", (nchan * npol,)),
                        ("DATA", ">i2", (npol, nchan, nbin))])
        tab = np.zeros(nsub, dtype=row)
        tab["INDEXVAL"] = np.arange(nsub)
        tab["TSUBINT"] = sublen
        tab["OFFS_SUB"] = sublen / 2.0 + np.arange(nsub) * sublen
        tab["DAT_FREQ"] = freqs
        tab["DAT_WTS"] = 1.0
        tab["DAT_OFFS"] = 0.0
        tab["DAT_SCL"] = 1.0
        tab["DATA"] = out
        if not eq_wts:
            raise NotImplementedError("template weights need the template file")
        sub = [_card("XTENSION", "BINTABLE"), _card("BITPIX", 8), _card("NAXIS", 2),
               _card("NAXIS1", row.itemsize), _card("NAXIS2", nsub), _card("PCOUNT", 0), _card("GCOUNT", 1),
               _card("TFIELDS", len(cols))]
        for i, (name, form, dim) in enumerate(cols, 1):
            sub.append(_card("TTYPE%d" % i, name))
            sub.append(_card("TFORM%d" % i, form))
            if dim:
                sub.append(_card("TDIM%d" % i, dim))
        sub += [_card("EXTNAME", "SUBINT"), _card("EPOCHS", "MIDTIME"), _card("INT_TYPE", "TIME"),
                _card("INT_UNIT", "SEC"), _card("NPOL", npol), _card("POL_TYPE", "AA+BB"),
                _card("TBIN", period / nbin), _card("NBIN", nbin), _card("NCHAN", nchan),
                _card("CHAN_BW", float(_val(signal.bw)) / nchan), _card("DM", dm), _card("NSBLK", 1),
                _card("NBITS", 16)]
        with open(self.path, "wb") as f:
            f.write(_header(primary))
            f.write(_header(sub))
            f.write(_pad(tab.tobytes()))


    def _save_search(self, signal, pulsar, MJD_start, inc_len, ref_MJD, telescope, nbits, nsblk, scale,
                     clip_sigma, max_stage_bytes):
        """Search-mode file (extension; the reference leaves search mode a
        TODO): ``nrows = nsamp // nsblk`` SUBINT rows of ``nsblk`` time
        samples, each sample its ``nchan`` channels as ``nbits``-bit codes,
        channel fastest, ``value = code * DAT_SCL + DAT_OFFS`` per (row,
        channel).  The device computes every block's min / max / sums
        (``pss_chan_stats``), the host derives DAT_OFFS / DAT_SCL from those
        [nrows][nchan] arrays in float64 --

        * ``scale="minmax"``: DAT_OFFS = min, DAT_SCL = (max - min) / L;
        * ``scale="sigma"``, ``clip_sigma=(lo, hi)``: DAT_OFFS = mu - lo sigma,
          DAT_SCL = (lo + hi) sigma / L (values outside clip to 0 / L);

        with L = 2^nbits - 1 -- and the device quantises and transposes
        (``pss_quantize_tmajor``) chunks of rows of at most ``max_stage_bytes``
        packed bytes, each copied to a pinned host buffer and appended to the
        file: neither the packed product nor a host copy of the float data is
        ever held whole, and ``signal.data`` is not modified.  A constant
        block gets code 0 everywhere (DAT_SCL 1.0 in the file); so does a
        block holding a NaN (DAT_OFFS 0, a warning is logged).  A trailing
        partial block is dropped.  One polarisation."""
        nchan = int(signal.Nchan)
        nbits, nsblk = int(nbits), int(nsblk)
        if nbits not in (8, 4, 2):
            raise ValueError("search-mode samples are 8, 4 or 2 bits wide, not %d" % nbits)
        if (nchan * nbits) % 8:
            raise ValueError("%d channels of %d bits do not fill whole bytes" % (nchan, nbits))
        if scale not in ("minmax", "sigma"):
            raise ValueError("scale %r: 'minmax' or 'sigma'" % (scale,))
        data = signal.data
        nsamp = int(data.shape[1])
        nrows = nsamp // nsblk if nsblk >= 1 else 0
        if nrows == 0:
            raise ValueError("nsblk %d: %d samples per channel hold no whole block" % (nsblk, nsamp))
        if int(data.shape[0]) != nchan:
            raise ValueError("signal.data holds %d channels, Nchan is %d" % (data.shape[0], nchan))
        if nrows * nsblk < nsamp:
            log.info("search-mode PSRFITS: dropping the trailing %d samples (partial block of %d)",
                     nsamp - nrows * nsblk, nsblk)
        L = (1 << nbits) - 1
        rowbytes = nsblk * nchan * nbits // 8

        import torch
        from .. import _engine, _lib
        if not isinstance(data, torch.Tensor):
            data = _engine.to_dev(np.asarray(data), dtype=torch.float32)
        elif data.dtype != torch.float32 or data.stride(1) != 1:
            data = data.to(torch.float32).contiguous()
        lib = _lib.lib()
        dev = data.device
        ld = max(int(data.stride(0)), nsamp)                   # (a one-channel tensor's stride is arbitrary)
        mn = torch.empty((nrows, nchan), dtype=torch.float32, device=dev)
        mx = torch.empty_like(mn)
        s1 = torch.empty((nrows, nchan), dtype=torch.float64, device=dev)
        s2 = torch.empty_like(s1)
        _lib.check(lib.pss_chan_stats(_engine.ptr(data), nchan, ld, nsblk, nrows, _engine.ptr(mn), _engine.ptr(mx),
                                      _engine.ptr(s1), _engine.ptr(s2), _engine.stream_ptr()), "chan_stats")
        if scale == "minmax":
            lo = mn.cpu().numpy().astype(np.float64)
            offs64 = lo
            scl64 = (mx.cpu().numpy().astype(np.float64) - lo) / L
        else:
            klo, khi = float(clip_sigma[0]), float(clip_sigma[1])
            mu = s1.cpu().numpy() / nsblk
            sigma = np.sqrt(np.maximum(s2.cpu().numpy() / nsblk - mu * mu, 0.0))
            offs64 = mu - klo * sigma
            scl64 = (klo + khi) * sigma / L
        with np.errstate(over="ignore", invalid="ignore"):
            offs = offs64.astype(np.float32)
            scl_k = scl64.astype(np.float32)                   # the kernel's: 0 -> code 0
        bad = ~(np.isfinite(offs) & np.isfinite(scl_k))
        if bad.any():
            log.warning("search-mode PSRFITS: %d (row, channel) blocks hold NaN or inf; their codes are 0",
                        int(bad.sum()))
            offs[bad] = 0.0
            scl_k[bad] = 0.0
        scl_file = np.where(scl_k == 0.0, np.float32(1.0), scl_k)
        d_scl = _engine.to_dev(scl_k)
        d_offs = _engine.to_dev(offs)

        dm = float(_val(signal.dm)) if getattr(signal, "dm", None) is not None else 0.0
        tbin = 1.0 / (float(_val(signal.samprate)) * 1e6)
        tsub = nsblk * tbin
        freqs = np.asarray(_val(signal.dat_freq), dtype=np.float64)[:nchan]
        primary = self._primary_cards(signal, pulsar, nchan, dm, MJD_start, inc_len, ref_MJD, telescope)
        nb = nchan * nbits // 8
        cols = [(n, "1" + c, None) for n, c in _SUBINT_SCALARS]
        cols += [("DAT_FREQ", "%dD" % nchan, None), ("DAT_WTS", "%dE" % nchan, None),
                 ("DAT_OFFS", "%dE" % nchan, None), ("DAT_SCL", "%dE" % nchan, None),
                 ("DATA", "%dB" % rowbytes, "(1,%d,1,%d)" % (nb, nsblk))]
        head = np.dtype([(n, _NP[c]) for n, c in _SUBINT_SCALARS] +
                        [("DAT_FREQ", ">f8", (nchan,)), ("DAT_WTS", ">f4", (nchan,)),
                         ("DAT_OFFS", ">f4", (nchan,)), ("DAT_SCL", ">f4", (nchan,))])
        tab = np.zeros(nrows, dtype=head)
        tab["INDEXVAL"] = np.arange(nrows)
        tab["TSUBINT"] = tsub
        tab["OFFS_SUB"] = (np.arange(nrows) + 0.5) * tsub
        tab["DAT_FREQ"] = freqs
        tab["DAT_WTS"] = 1.0
        tab["DAT_OFFS"] = offs
        tab["DAT_SCL"] = scl_file
        sub = [_card("XTENSION", "BINTABLE"), _card("BITPIX", 8), _card("NAXIS", 2),
               _card("NAXIS1", head.itemsize + rowbytes), _card("NAXIS2", nrows), _card("PCOUNT", 0),
               _card("GCOUNT", 1), _card("TFIELDS", len(cols))]
        for i, (name, form, dim) in enumerate(cols, 1):
            sub.append(_card("TTYPE%d" % i, name))
            sub.append(_card("TFORM%d" % i, form))
            if dim:
                sub.append(_card("TDIM%d" % i, dim))
        sub += [_card("EXTNAME", "SUBINT"), _card("EPOCHS", "MIDTIME"), _card("INT_TYPE", "TIME"),
                _card("INT_UNIT", "SEC"), _card("NPOL", 1), _card("POL_TYPE", "AA+BB"), _card("TBIN", tbin),
                _card("NBIN", 1), _card("NCHAN", nchan), _card("CHAN_BW", float(_val(signal.bw)) / nchan),
                _card("DM", dm), _card("NSBLK", nsblk), _card("NBITS", nbits), _card("ZERO_OFF", 0.0),
                _card("SIGNINT", 0), _card("NSUBOFFS", 0)]

        chunk = int(max(1, min(nrows, int(max_stage_bytes) // rowbytes)))
        stage = torch.empty(chunk * rowbytes, dtype=torch.uint8, device=dev)
        host = torch.empty(chunk * rowbytes, dtype=torch.uint8).pin_memory()
        host_np = host.numpy()
        with open(self.path, "wb") as f:
            f.write(_header(primary))
            f.write(_header(sub))
            for r0 in range(0, nrows, chunk):
                n = min(chunk, nrows - r0)
                rc = lib.pss_quantize_tmajor(data.data_ptr() + 4 * r0 * nsblk, nchan, ld, nsblk, n,
                                             d_scl.data_ptr() + 4 * r0 * nchan, d_offs.data_ptr() + 4 * r0 * nchan,
                                             nbits, _engine.ptr(stage), _engine.stream_ptr())
                _lib.check(rc, "quantize_tmajor")
                host[:n * rowbytes].copy_(stage[:n * rowbytes], non_blocking=True)
                torch.cuda.current_stream().synchronize()
                for i in range(n):
                    f.write(tab[r0 + i].tobytes())
                    f.write(host_np[i * rowbytes:(i + 1) * rowbytes])
            f.write(b"\0" * ((-nrows * (head.itemsize + rowbytes)) % _BLOCK))
        self.nchan, self.nrows, self.nsblk, self.tbin, self.npol = nchan, nrows, nsblk, tbin, 1

    # -- load ---------------------------------------------------------------
    def load_search(self, rows=None, apply_weights=True, period=None, max_stage_bytes=256 << 20):
        """The search-mode file at ``path`` as a device FilterBankSignal
        (:func:`load_search_signal`)."""
        if self.path is None:
            raise ValueError("no input path")
        return load_search_signal(self.path, rows=rows, apply_weights=apply_weights, period=period,
                                  max_stage_bytes=max_stage_bytes)


# pinned / staging buffer pairs of load_search_signal (tools/search_in_bench.py
# times one pair against two)
_LOAD_BUFFERS = 2


def _find_subint(path):
    """(primary header, SUBINT header, byte offset of the SUBINT table) of a
    FITS file, through a memory map: only the header blocks are read."""
    import mmap
    with open(path, "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    try:
        prim, pos = None, 0
        while pos < len(mm):
            hdr, pos = _parse_header(mm, pos)
            if "SIMPLE" in hdr:
                prim = hdr
            elif str(hdr.get("EXTNAME", "")).strip() == "SUBINT" and hdr.get("XTENSION") == "BINTABLE":
                if prim is None:
                    raise ValueError("%s: a SUBINT table without a primary header" % path)
                return prim, hdr, pos
            pos += -(-_hdu_size(hdr, 0)[1] // _BLOCK) * _BLOCK
    finally:
        mm.close()
    raise ValueError("%s holds no SUBINT table" % path)


def _search_layout(path, rows):
    """Everything :func:`load_search_signal` decides on the host, before any
    device use: the file's geometry, the selected rows, the polarisations to
    sum, the band's direction, and the SUBINT table as a memory map."""
    prim, sub, pos = _find_subint(path)
    nbits, signint, nbin = int(sub.get("NBITS", 0)), int(sub.get("SIGNINT", 0) or 0), int(sub.get("NBIN", 1) or 1)
    npol, pol_type = int(sub.get("NPOL", 1)), str(sub.get("POL_TYPE", "")).strip()
    if nbits not in (8, 4, 2):
        raise NotImplementedError("search-mode samples of NBITS = %d (8, 4 and 2 are read)" % nbits)
    if signint == 1:
        raise NotImplementedError("signed samples (SIGNINT = 1)")
    if nbin != 1:
        raise NotImplementedError("NBIN = %d: not a search-mode table (NBIN = 1)" % nbin)
    if npol == 1:
        nsum = 1
    elif npol == 2 or (npol == 4 and pol_type.startswith("AABB")):
        nsum = 2                                               # AA + BB
    elif npol == 4 and pol_type == "IQUV":
        nsum = 1                                               # I
    else:
        raise NotImplementedError("NPOL = %d with POL_TYPE %r (total intensity comes from NPOL 1, NPOL 2, "
                                  "AABB.. or IQUV)" % (npol, pol_type))
    nchan, nsblk, nrows = int(sub["NCHAN"]), int(sub["NSBLK"]), int(sub["NAXIS2"])
    if nchan < 1 or nsblk < 1 or (nchan * nbits) % 8:
        raise ValueError("%s: NCHAN %d, NSBLK %d at %d bits" % (path, nchan, nsblk, nbits))
    tbin = float(sub["TBIN"])
    if not tbin > 0.0:
        raise ValueError("%s: TBIN %r" % (path, tbin))
    r0, r1 = (0, nrows) if rows is None else (int(rows[0]), int(rows[1]))
    if not (0 <= r0 < r1 <= nrows):
        raise ValueError("rows %r outside the %d rows of %s" % (rows, nrows, path))
    # the DATA column as plain bytes, whatever its TDIM says
    names = [str(sub["TTYPE%d" % i]).strip() for i in range(1, int(sub["TFIELDS"]) + 1)]
    missing = [c for c in ("DAT_FREQ", "DAT_WTS", "DAT_OFFS", "DAT_SCL", "DATA") if c not in names]
    if missing:
        raise ValueError("%s: the SUBINT table lacks %s" % (path, ", ".join(missing)))
    flat = dict(sub)
    flat.pop("TDIM%d" % (names.index("DATA") + 1), None)
    dt = _table_dtype(flat)
    databytes = nsblk * npol * nchan * nbits // 8
    sizes = {"DATA": databytes, "DAT_FREQ": 8 * nchan, "DAT_WTS": 4 * nchan, "DAT_OFFS": 4 * npol * nchan,
             "DAT_SCL": 4 * npol * nchan}
    for name, want in sizes.items():
        if dt.fields[name][0].itemsize != want:
            raise ValueError("%s: column %s holds %d bytes a row, %d channels x %d polarisations x %d samples of %d "
                             "bits need %d" % (path, name, dt.fields[name][0].itemsize, nchan, npol, nsblk, nbits, want))
    rec = np.memmap(path, dtype=dt, mode="r", offset=pos, shape=(nrows,))
    freq = np.asarray(rec["DAT_FREQ"], dtype=np.float64).reshape(nrows, nchan)
    if (freq != freq[0]).any():
        raise ValueError("%s: DAT_FREQ differs between rows" % path)
    step = np.diff(freq[0])
    if not ((step > 0).all() or (step < 0).all()):
        raise ValueError("%s: DAT_FREQ is not monotonic" % path)
    if "OBSFREQ" not in prim or "OBSBW" not in prim:
        raise ValueError("%s: no OBSFREQ / OBSBW" % path)
    return dict(prim=prim, sub=sub, rec=rec, pos=pos, data_off=dt.fields["DATA"][1], databytes=databytes,
                nbits=nbits, npol=npol, nsum=nsum, pol_type=pol_type, nchan=nchan, nsblk=nsblk, nrows=nrows,
                tbin=tbin, r0=r0, r1=r1, freq=freq[0], flip=bool(nchan > 1 and step[0] < 0),
                zero_off=float(sub.get("ZERO_OFF", 0.0) or 0.0))


def load_search_signal(path, rows=None, apply_weights=True, period=None, max_stage_bytes=256 << 20):
    """A search-mode PSRFITS file as a search-mode FilterBankSignal on the
    device (extension): the inverse of :meth:`PSRFITS.save` in search mode, and
    a reader of foreign files of the same kind -- 8-, 4- or 2-bit unsigned
    samples, NPOL 1, NPOL 2 or ``AABB..`` (the first two polarisations are
    summed) or ``IQUV`` (the first is taken).  ``NotImplementedError`` names
    anything else (other NBITS, SIGNINT = 1, NBIN != 1, another POL_TYPE).

    The headers and the small SUBINT columns are read on the host through a
    memory map of the table.  The DATA column of the rows ``rows=(r0, r1)``
    (default: all) goes to the device in chunks of at most ``max_stage_bytes``
    packed bytes -- file to a pinned buffer, pinned buffer to a staging
    buffer, ``pss_unpack_tmajor`` from there into the final [nchan][nsamp]
    float32 tensor (row stride on the 16-B grid) -- with two buffer pairs, so
    that the host reads chunk k + 1 from the file while the device copies and
    unpacks chunk k; the only host waits are for a pinned buffer's previous
    copy.  Neither the DATA column nor a float copy of it is ever held whole
    on the host.  Every sample is

        (sum_p ((code - ZERO_OFF) * DAT_SCL[p] + DAT_OFFS[p])) * DAT_WTS

    in float32 (``apply_weights=False``: no weights).

    ``dat_freq`` is row 0's DAT_FREQ as the file gives it (this package's
    files hold channel lower edges there, foreign files centres; the search
    stages use ``dat_freq`` either way); a descending band is flipped, so that
    ``dat_freq`` ascends.  ``ValueError`` for a DAT_FREQ that is not monotonic
    or differs between rows, and for ``rows`` outside the file.  ``fcent`` and
    ``bw`` are OBSFREQ and |OBSBW|, ``samprate`` 1e-6 / TBIN MHz, ``dm`` the
    DM card (None when absent or 0).  The signal is one subint spanning
    ``tobs`` unless ``period`` (s) is given: then ``sublen = period`` and
    ``nsub = round(tobs / period)``, as ``make_pulses`` leaves a search-mode
    signal.  ``signal.psrfits`` records nbits, nsblk, nrows, npol, pol_type,
    zero_off, nsuboffs, flipped, weights (row 0's DAT_WTS in output channel
    order) and the two header dicts."""
    lay = _search_layout(path, rows)
    nchan, npol, nsblk, nbits = lay["nchan"], lay["npol"], lay["nsblk"], lay["nbits"]
    r0, r1, rec, databytes, flip = lay["r0"], lay["r1"], lay["rec"], lay["databytes"], lay["flip"]
    n = r1 - r0
    f32 = lambda col, width: np.ascontiguousarray(np.asarray(rec[col][r0:r1], dtype=np.float32).reshape(n, width))
    scl, offs = f32("DAT_SCL", npol * nchan), f32("DAT_OFFS", npol * nchan)

    import torch
    from .. import _engine, _lib
    from ..signal import FilterBankSignal
    from .._units import make_quant
    lib = _lib.lib()
    dev = _engine.device()
    d_scl, d_offs = _engine.to_dev(scl), _engine.to_dev(offs)
    d_wts = _engine.to_dev(f32("DAT_WTS", nchan)) if apply_weights else None
    nsamp = n * nsblk
    ld = (nsamp + 3) // 4 * 4                                  # rows on the 16-B grid, as channelize
    out = torch.empty((nchan, ld), dtype=torch.float32, device=dev)[:, :nsamp]
    chunk = int(max(1, min(n, int(max_stage_bytes) // databytes)))
    nbuf = min(_LOAD_BUFFERS, -(-n // chunk))
    host = [torch.empty(chunk * databytes, dtype=torch.uint8).pin_memory() for _ in range(nbuf)]
    stage = [torch.empty(chunk * databytes, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
    copied = [None] * nbuf
    raw = np.memmap(path, dtype=np.uint8, mode="r", offset=lay["pos"], shape=(lay["nrows"], rec.dtype.itemsize))
    raw = raw[:, lay["data_off"]:lay["data_off"] + databytes]
    for k, a in enumerate(range(r0, r1, chunk)):
        b, m = k % nbuf, min(chunk, r1 - a)
        if copied[b] is not None:
            copied[b].synchronize()                            # the copy that last read this pinned buffer
        host[b].numpy()[:m * databytes].reshape(m, databytes)[...] = raw[a:a + m]
        stage[b][:m * databytes].copy_(host[b][:m * databytes], non_blocking=True)
        copied[b] = torch.cuda.Event()
        copied[b].record()
        rc = lib.pss_unpack_tmajor(stage[b].data_ptr(), nchan, npol, lay["nsum"], nsblk, m,
                                   d_scl.data_ptr() + 4 * (a - r0) * npol * nchan,
                                   d_offs.data_ptr() + 4 * (a - r0) * npol * nchan,
                                   d_wts.data_ptr() + 4 * (a - r0) * nchan if d_wts is not None else None,
                                   lay["zero_off"], nbits, 1 if flip else 0, out.data_ptr() + 4 * (a - r0) * nsblk, ld,
                                   _engine.stream_ptr())
        _lib.check(rc, "unpack_tmajor")

    prim, sub, tbin = lay["prim"], lay["sub"], lay["tbin"]
    sig = FilterBankSignal(float(prim["OBSFREQ"]), abs(float(prim["OBSBW"])), Nsubband=nchan, fold=False,
                           dtype=np.float32)
    sig._samprate = make_quant(1e-6 / tbin, 'MHz')             # (set here: the constructor warns below Nyquist)
    order = slice(None, None, -1) if flip else slice(None)
    sig._dat_freq = Quantity(lay["freq"][order].copy(), 'MHz')
    sig._buf = out
    sig._ncols = nsamp
    sig._nsamp = nsamp
    sig._pending = None
    tobs = nsamp * tbin
    sig._tobs = make_quant(tobs, 's')
    if period:
        sig._sublen = make_quant(float(period), 's')
        sig._nsub = int(np.round(tobs / float(period)))
    else:
        sig._sublen = sig._tobs
        sig._nsub = 1
    sig._set_draw_norm(df=1)
    sig._Smax = None
    dm = sub.get("DM")
    sig._dm = make_quant(float(dm), 'pc/cm^3') if dm else None
    sig._delay = None
    sig._null_error = None
    sig._null_checks = []
    wts0 = np.asarray(rec["DAT_WTS"][0], dtype=np.float32).reshape(nchan)
    sig.psrfits = dict(nbits=nbits, nsblk=nsblk, nrows=n, npol=npol, pol_type=lay["pol_type"],
                       zero_off=lay["zero_off"], nsuboffs=int(sub.get("NSUBOFFS", 0) or 0), flipped=flip,
                       weights=wts0[order].copy(), primary=prim, subint=sub)
    return sig


def read_search_data(path):
    """A search-mode file of :meth:`PSRFITS.save` on the host: ``(codes,
    values, primary header, SUBINT header)`` with ``codes`` uint8
    [nchan][nrows * nsblk] (the NBITS-bit samples unpacked: the
    lower-numbered channel of a byte in its more significant bits) and
    ``values = codes * DAT_SCL + DAT_OFFS`` (float64 arithmetic, stored as
    float32) of the same shape."""
    prim, sub, rec = read_psrfits(path)
    nbits, nchan, nsblk, nrows = int(sub["NBITS"]), int(sub["NCHAN"]), int(sub["NSBLK"]), int(sub["NAXIS2"])
    if nbits not in (8, 4, 2) or int(sub.get("NPOL", 1)) != 1:
        raise NotImplementedError("search-mode data of %d bits, %d polarisations" % (nbits, sub.get("NPOL", 1)))
    per = 8 // nbits
    raw = np.ascontiguousarray(rec["DATA"]).reshape(nrows, nsblk, nchan // per)
    codes = np.empty((nrows, nsblk, nchan), dtype=np.uint8)
    for p in range(per):
        codes[:, :, p::per] = (raw >> (8 - nbits * (p + 1))) & ((1 << nbits) - 1)
    scl = np.asarray(rec["DAT_SCL"], dtype=np.float64).reshape(nrows, 1, nchan)
    offs = np.asarray(rec["DAT_OFFS"], dtype=np.float64).reshape(nrows, 1, nchan)
    values = (codes * scl + offs).astype(np.float32)
    tmajor = lambda a: np.ascontiguousarray(a.reshape(nrows * nsblk, nchan).T)
    return tmajor(codes), tmajor(values), prim, sub


def _parse_header(buf, pos):
    """(cards dict, position after the header) of the header at ``pos``."""
    cards = {}
    while True:
        block = buf[pos:pos + _BLOCK].decode("ascii", errors="replace")
        if len(block) < _BLOCK:
            raise ValueError("truncated FITS header")
        pos += _BLOCK
        for i in range(0, _BLOCK, 80):
            c = block[i:i + 80]
            key = c[:8].strip()
            if key == "END":
                return cards, pos
            if c[8:10] == "= ":
                v = c[10:]
                if v.lstrip().startswith("'"):
                    v = v.lstrip()
                    j = 1
                    out = []
                    while j < len(v):            # quoted string, '' escapes a quote
                        if v[j] == "'":
                            if j + 1 < len(v) and v[j + 1] == "'":
                                out.append("'")
                                j += 2
                                continue
                            break
                        out.append(v[j])
                        j += 1
                    v = "".join(out).rstrip()
                else:
                    v = v.split("/")[0].strip()
                    if v in ("T", "F"):
                        v = v == "T"
                    elif v == "":
                        v = None
                    else:
                        try:
                            v = int(v)
                        except ValueError:
                            v = float(v.replace("D", "E"))
                cards[key] = v


def _table_dtype(hdr):
    """numpy dtype of a BINTABLE row (TFORM rTa codes D E I J K B L A; TDIM
    reshapes, fastest axis first as FITS writes them)."""
    fields = []
    for i in range(1, int(hdr["TFIELDS"]) + 1):
        form = str(hdr["TFORM%d" % i]).strip()
        k = 0
        while k < len(form) and form[k].isdigit():
            k += 1
        n, code = int(form[:k] or 1), form[k]
        if code not in _NP:
            raise NotImplementedError("FITS column format %r" % form)
        shape = (n,) if n > 1 else ()
        dim = hdr.get("TDIM%d" % i)
        if dim and n > 1:
            shape = tuple(int(x) for x in str(dim).strip("() ").split(","))[::-1]
        if code == "A":
            fields.append((hdr["TTYPE%d" % i], "S%d" % n))
        else:
            fields.append((hdr["TTYPE%d" % i], _NP[code], shape))
    dt = np.dtype(fields)
    if dt.itemsize != int(hdr["NAXIS1"]):
        raise ValueError("row layout %d B != NAXIS1 %d" % (dt.itemsize, hdr["NAXIS1"]))
    return dt


def read_fits(path):
    """All HDUs of a FITS file of binary tables (PSRFITS):
    ``{"PRIMARY": (header, None), EXTNAME: (header, records or None)}``."""
    with open(path, "rb") as f:
        buf = f.read()
    out = {}
    pos = 0
    while pos < len(buf):
        hdr, pos = _parse_header(buf, pos)
        name, size = _hdu_size(hdr, len(out))
        if "SIMPLE" in hdr:
            out[name] = (hdr, None)
        else:
            rec = None
            if hdr.get("XTENSION") == "BINTABLE":
                try:
                    rec = np.frombuffer(buf, dtype=_table_dtype(hdr), count=int(hdr["NAXIS2"]), offset=pos)
                except NotImplementedError:
                    rec = None
            out[name] = (hdr, rec)
        pos += -(-size // _BLOCK) * _BLOCK
    return out


def read_psrfits(path):
    """(primary header dict, SUBINT header dict, SUBINT records) of a PSRFITS
    file: one written by :meth:`PSRFITS.save`, or the reference's template."""
    hdus = read_fits(path)
    sub, rec = hdus["SUBINT"]
    return hdus["PRIMARY"][0], sub, rec


def template_profile(path, subint=0, chan=0, pol=0, baseline="median"):
    """Pulse profile of a fold-mode PSRFITS template: DATA * DAT_SCL +
    DAT_OFFS of one (subint, channel, polarisation) -- the PSRFITS scaling
    (template SUBINT: 'Data scale factor (outval=dataval*scl + offs)') -- as
    float64 (NBIN,), with the baseline (the median bin; None: none) removed.
    Config C4's portrait is this profile of the reference's B1855+09 template
    (DataProfile of it, tiled over the channels)."""
    _, sub, rec = read_psrfits(path)
    npol = int(sub.get("NPOL", 1))
    nchan = int(sub.get("NCHAN", 1))
    r = rec[subint]
    data = np.asarray(r["DATA"], dtype=np.float64).reshape(npol, nchan, -1)[pol, chan]
    scl = np.asarray(r["DAT_SCL"], dtype=np.float64).reshape(-1)[pol * nchan + chan]
    offs = np.asarray(r["DAT_OFFS"], dtype=np.float64).reshape(-1)[pol * nchan + chan]
    prof = data * scl + offs
    if baseline == "median":
        prof = prof - np.median(prof)
    return prof
