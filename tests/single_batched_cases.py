"""Case scripts (tests/replay.py's ``run_case`` dicts) for the lengths the
single-workgroup kernel serves with several rows per workgroup, N = 64 ..
2048, and for the direct DFT.  Host only: tests/test_single_batched_cases.py
checks them on the CPU, tests/test_gpu_single_batched.py runs them.

Every case is eight 5 ms periods of Nph = N / 8 samples (search mode: eight
pulses; fold mode: eight sub-integrations of 50 periods), a Gaussian portrait
(0.5, 0.05, 1), a DM of 0.02 N / 64 (a few to tens of samples across the
band) and, where it has one, a null of 2 of the 8 pulses.  The band has
BATCH(N) + 3 channels: two workgroups, the last one partly filled, an odd
count.
"""
import numpy as np

PERIOD = 0.005
LENGTHS = (64, 128, 256, 512, 1024, 2048)          # the batched instantiations
ALL_SINGLE = LENGTHS + (4096, 8192)
# rows per workgroup: BATCH N = 4096, and one row at 8192 (the template
# arguments of launch_single_n, csrc/pss_single.hip, are the source of this rule)
BATCH = {64: 64, 128: 32, 256: 16, 512: 8, 1024: 4, 2048: 2, 4096: 1, 8192: 1}
DIRECT = (32, 66, 250, 1000)                       # direct-DFT lengths (5 rows)
DIRECT_ROWS = 5
NULL_FRAC = 0.25
MULTS = (4, 2.3, 5.5)                              # resampling: dt_tel = mult dt_sig
BRANCH = {4: "down", 2.3: "rebin", 5.5: "rebin", 64: "down", 128: "down"}
WINDOW_LENGTHS = (64, 128, 2048)                   # 4, 2 and 1 rows per wave
# down_sample by N: ONE window per row.  Only then do neighbouring lanes of
# different rows hold the same window index (the last lane of a row window
# L - 1, the first lane of the next window 0), i.e. only then would a wave
# that merged its lanes' sums across rows give other values
ONE_WINDOW = {64: 64, 128: 128}
UNDELAYED_LENGTHS = (64, 256, 2048)
ROWCOUNT_LENGTHS = (64, 128, 2048)
# seeds whose delayed null leaves no sample in the oracle's ambiguity band
# (search mode, nchan = BATCH + 3): the resampled copy cannot exclude any
ZERO_AMBIG_SEED = {64: 1, 128: 1, 2048: 1}


def nchan_of(N):
    return BATCH[N] + 3 if N in BATCH else DIRECT_ROWS


def nph_of(N):
    return N // 8 if N % 8 == 0 else N / 8.0


def samprate(N):
    """MHz: Nph samples per period."""
    return (N / 8.0) / (PERIOD * 1e6)


def dm_of(N):
    return 0.02 * N / 64


def dt_sig(N, fold):
    """The sample time observe() compares the backend's with (telescope.py:94-100)."""
    nph = N / 8.0
    return (50 * PERIOD if fold else PERIOD) / nph


def case(N, fold=False, null="delayed", nchan=None, chans=None, dtype=np.float32, prof=None, specidx=0.0,
         mult=None, noise=True, dm=None):
    """The chain pulses -> disperse -> null -> observe (``null`` = "delayed"),
    pulses -> null -> disperse -> observe ("undelayed") or without a null
    (None).  ``mult``: observe through a custom backend of sample time
    mult dt_sig (the down_sample / rebin branches); otherwise Arecibo's
    Lband_PUPPI (the full-rate copy).  ``chans``: a shard of the band."""
    nchan = nchan_of(N) if nchan is None else nchan
    sr = samprate(N)
    sig = dict(fcent=1400, bw=400, nchan=nchan, samprate=sr, fold=fold, dtype=dtype)
    if fold:
        sig["sublen"] = 50 * PERIOD
        tobs = 8 * 50 * PERIOD
    else:
        tobs = (N + 0.5) / (sr * 1e6)
    if chans is not None:
        sig["chans"] = tuple(chans)
    psr = dict(period=PERIOD, Smean=1.0, prof=prof if prof is not None else ("gauss", 0.5, 0.05, 1))
    if specidx:
        psr.update(specidx=specidx, ref_freq=1300)
    dm = dm_of(N) if dm is None else dm
    ops = [("make_pulses", tobs, "pulses")]
    if null == "undelayed":
        ops.append(("null", NULL_FRAC, "null"))
    if dm:
        ops.append(("disperse", dm, "disperse"))
    if null == "delayed":
        ops.append(("null", NULL_FRAC, "null"))
    if mult is None:
        ops.append(("observe", "Arecibo", "Lband_PUPPI", noise, "noise" if noise else None))
    else:
        ops.append(("observe", ("custom", 2 * mult * dt_sig(N, fold)), "T", noise, "noise" if noise else None))
    return dict(sig=sig, psr=psr, ops=ops)


def shards(N):
    """(full band's channel count, the two shards of §b): rows 1 .. BATCH + 1
    (two workgroups, off the band's first row) and the three rows from BATCH."""
    B = BATCH[N]
    return B + 5, ((1, B + 2), (B, B + 3))


def rowcounts(N):
    B = BATCH[N]
    return sorted({1, B - 1, B, B + 1, 2 * B + 1} - {0})


# ---------------------------------------------------------------------------
# the cases of tests/test_gpu_single_batched.py, by section: (id, case, seed)
# ---------------------------------------------------------------------------
def chain_cases():
    """(a) the full chain on every batched length, search and fold."""
    out = []
    for N in LENGTHS:
        for fold in (False, True):
            out.append(("%d-%s" % (N, "fold" if fold else "search"), case(N, fold=fold), 2 if fold else 1))
    for N in UNDELAYED_LENGTHS:
        out.append(("%d-search-undelayed" % N, case(N, null="undelayed"), 3))
    out.append(("128-search-int8", case(128, dtype=np.int8), 2))
    out.append(("512-search-portrait", case(512, prof=("data", nchan_of(512)), specidx=-1.6), 1))
    out.append(("1024-fold-portrait", case(1024, fold=True, prof=("data", nchan_of(1024)), specidx=-1.6), 3))
    return out


def shard_cases():
    """(b) shards of a wider band against the oracle (no null: the harness's
    rule).  Search mode with a spectral index: every row has its own table
    row.  The two fold-mode shards have none: the oracle of a shard holds only
    the shard's rows and a fold-mode portrait is renormalised to ITS maximum
    (portraits.py:32-45), which is the band's only where all rows are alike
    (the fold-mode table rows of a shard are tied to the full band's, bit for
    bit, by the Philox comparison, and the full band's to the oracle by
    chain_cases' 1024-fold-portrait)."""
    out = []
    for N in LENGTHS:
        full, pair = shards(N)
        for i, ch in enumerate(pair):
            fold = (N in (256, 2048)) and i == 1
            out.append(("%d-%d:%d%s" % (N, ch[0], ch[1], "-fold" if fold else ""),
                        case(N, fold=fold, null=None, nchan=full, chans=ch, prof=("data", full),
                             specidx=0.0 if fold else -1.6), 4 + i))
    return out


def window_cases():
    """(d) the resampled copy against the oracle: (id, case, seed, branch)."""
    out = []
    for N in WINDOW_LENGTHS:
        for m in MULTS + ((ONE_WINDOW[N],) if N in ONE_WINDOW else ()):
            out.append(("%d-x%g" % (N, m), case(N, null=None, mult=m), 5, BRANCH[m]))
            out.append(("%d-x%g-null" % (N, m), case(N, mult=m), ZERO_AMBIG_SEED[N], BRANCH[m]))
    return out


def direct_cases():
    """(e) the direct DFT: delayed null (float64 refine over the direct rows) and none."""
    out = []
    for N in DIRECT:
        out.append(("%d-null" % N, case(N), 1))
        out.append(("%d" % N, case(N, null=None), 2))
    out.append(("250-x2.3", case(250, null=None, mult=2.3), 2))
    return out


def null_cases():
    """Every (id, case, seed) above that has a delayed null (the oracle-only band check)."""
    every = chain_cases() + [c[:3] for c in window_cases()] + direct_cases()
    return [c for c in every if c[1]["ops"][-2][0] == "null"]


def nsamp_of(c):
    """The case's length as the reference computes it (pulsar.py:107-151)."""
    sr, tobs = c["sig"]["samprate"], c["ops"][0][1]
    if c["sig"]["fold"]:
        return int((int(np.round(tobs / c["sig"]["sublen"])) * (PERIOD * sr)) * 1e6)
    return int((tobs * sr) * 1e6)
