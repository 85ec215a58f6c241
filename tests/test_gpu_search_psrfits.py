"""Search-mode PSRFITS output on the device: pss_chan_stats and
pss_quantize_tmajor against a float64 NumPy restatement written here, and the
writer end to end.

Inputs: chi2(1) draws of a seeded ``np.random.default_rng`` times a
per-channel gain 1 + c, cast to float32.

Tolerances.  min / max: exact.  The float64 sums of n <= 4096 float32 values
carry <= n 2^-53 relative error (every term is exact in float64; each add
rounds once): mean rtol 1e-12.  sigma = sqrt(sumsq / n - mean^2) multiplies
that by (mu^2 + sigma^2) / sigma^2, asserted <= 1e2 here: rtol 1e-9.
Codes: equal to clip(rint(u), 0, L) with u = (x - offs) / scl in float64
except where u lies within 4 2^-24 max(|u|, 1) of a half-integer (one float32
subtract plus a divide or reciprocal-multiply), where they may differ by one
level; at most 0.1 % of the samples may lie in that band."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (nsblk, nrows, ld - nrows nsblk) of the stats shapes, reused by the quantiser
GEOMS = [(1, 1, 0), (7, 2, 5), (100, 3, 0), (64, 2, 3), (4096, 1, 0)]
STAT_SHAPES = [(1, 1, 1, 0), (3, 7, 2, 5), (24, 100, 3, 0), (136, 64, 2, 3), (65, 4096, 1, 0)]
BAND = 4.0 * 2.0 ** -24


def _draws(nchan, nsblk, nrows, pad, seed=20240):
    rng = np.random.default_rng(seed + 1000 * nchan + nsblk)
    x = rng.chisquare(1.0, (nchan, nrows * nsblk + pad)) * (1.0 + np.arange(nchan))[:, None]
    return x.astype(np.float32)


def _blocks(x, nsblk, nrows):
    """[nrows][nchan][nsblk] view of the rows' samples."""
    return x[:, :nrows * nsblk].reshape(x.shape[0], nrows, nsblk).transpose(1, 0, 2)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stats(hip_lib, d, nchan, nsblk, nrows):
    import torch
    mn = torch.empty((nrows, nchan), dtype=torch.float32, device="cuda")
    mx = torch.empty_like(mn)
    s1 = torch.empty((nrows, nchan), dtype=torch.float64, device="cuda")
    s2 = torch.empty_like(s1)
    rc = hip_lib.pss_chan_stats(d.data_ptr(), nchan, d.stride(0), nsblk, nrows, mn.data_ptr(), mx.data_ptr(),
                                s1.data_ptr(), s2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (mn, mx, s1, s2)]


@pytest.mark.parametrize("nchan,nsblk,nrows,pad", STAT_SHAPES)
def test_chan_stats_vs_numpy(hip_lib, nchan, nsblk, nrows, pad):
    x = _draws(nchan, nsblk, nrows, pad)
    b = _blocks(x, nsblk, nrows)
    b64 = b.astype(np.float64)
    d = _dev(x)
    mn, mx, s1, s2 = _stats(hip_lib, d, nchan, nsblk, nrows)
    np.testing.assert_array_equal(mn, b.min(axis=2))
    np.testing.assert_array_equal(mx, b.max(axis=2))
    mu_ref, sd_ref = b64.mean(axis=2), b64.std(axis=2)
    mu = s1 / nsblk
    sd = np.sqrt(np.maximum(s2 / nsblk - mu * mu, 0.0))
    print("mean max rel err", np.max(np.abs(mu - mu_ref) / np.abs(mu_ref)))
    np.testing.assert_allclose(mu, mu_ref, rtol=1e-12, atol=0)
    if nsblk == 1:
        np.testing.assert_array_equal(sd, 0.0)          # x^2 - x^2 is exact in float64
    else:
        amp = (mu_ref ** 2 + sd_ref ** 2) / sd_ref ** 2
        print("sigma max rel err", np.max(np.abs(sd - sd_ref) / sd_ref), "amplification", amp.max())
        assert amp.max() <= 1e2
        np.testing.assert_allclose(sd, sd_ref, rtol=1e-9, atol=0)
    # the same launch again: the same bits
    again = _stats(hip_lib, d, nchan, nsblk, nrows)
    for a, g in zip((mn, mx, s1, s2), again):
        assert a.tobytes() == g.tobytes()


@pytest.mark.parametrize("nchan,nsblk,nrows,pad", [(3, 7, 2, 5), (24, 100, 3, 0)])
def test_chan_stats_nan_poisons_its_block_only(hip_lib, nchan, nsblk, nrows, pad):
    x = _draws(nchan, nsblk, nrows, pad)
    clean = _stats(hip_lib, _dev(x), nchan, nsblk, nrows)
    r, c = nrows - 1, nchan // 2
    x[c, r * nsblk + nsblk // 3] = np.nan
    got = _stats(hip_lib, _dev(x), nchan, nsblk, nrows)
    for a, g in zip(clean, got):
        assert np.isnan(g[r, c])
        keep = np.ones(a.shape, dtype=bool)
        keep[r, c] = False
        assert a[keep].tobytes() == g[keep].tobytes()


# ---------------------------------------------------------------------------
# quantiser
# ---------------------------------------------------------------------------
def _unpack(packed, nbits):
    """bytes [..., nchan nbits / 8] -> codes [..., nchan]."""
    if nbits == 8:
        return packed.copy()
    per = 8 // nbits
    out = np.empty(packed.shape[:-1] + (packed.shape[-1] * per,), dtype=np.uint8)
    for p in range(per):                             # channel per k + p: bits from the top down
        out[..., p::per] = (packed >> (8 - nbits * (p + 1))) & ((1 << nbits) - 1)
    return out


def _scaling(b, nbits, scale):
    """float32 (offs, scl) [nrows][nchan] from the float64 restatement of the
    block statistics, as the writer derives them."""
    L = (1 << nbits) - 1
    b64 = b.astype(np.float64)
    if scale == "minmax":
        offs = b64.min(axis=2)
        scl = (b64.max(axis=2) - offs) / L
    else:
        mu, sd = b64.mean(axis=2), b64.std(axis=2)
        offs = mu - 2.0 * sd
        scl = 8.0 * sd / L
    return offs.astype(np.float32), scl.astype(np.float32)


def _quantize(hip_lib, d, nchan, nsblk, nrows, scl, offs, nbits, col0=0, guard=0):
    """Run the kernel on rows starting at column col0; returns the packed
    bytes [nrows][nsblk][nchan nbits / 8] and the two guard regions."""
    import torch
    nb = nchan * nbits // 8
    total = nrows * nsblk * nb
    buf = torch.full((guard + total + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ds, do = _dev(scl), _dev(offs)
    rc = hip_lib.pss_quantize_tmajor(d.data_ptr() + 4 * col0, nchan, d.stride(0), nsblk, nrows, ds.data_ptr(),
                                     do.data_ptr(), nbits, buf.data_ptr() + guard,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    return h[guard:guard + total].reshape(nrows, nsblk, nb), h[:guard], h[guard + total:]


def _check_codes(codes, b, scl, offs, nbits):
    """codes [nrows][nsblk][nchan] against the float64 restatement."""
    L = (1 << nbits) - 1
    x = b.astype(np.float64).transpose(0, 2, 1)                      # [nrows][nsblk][nchan]
    s, o = scl.astype(np.float64)[:, None, :], offs.astype(np.float64)[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (x - o) / s
    zero = np.broadcast_to(s == 0.0, u.shape)
    u = np.where(zero, 0.0, u)
    want = np.clip(np.rint(u), 0, L)
    band = np.abs(u - np.floor(u) - 0.5) <= BAND * np.maximum(np.abs(u), 1.0)
    frac = band.mean()
    diff = np.abs(codes.astype(np.float64) - want)
    print("band fraction", frac, "mismatches in band", int((diff[band] != 0).sum()))
    assert frac <= 1e-3
    assert (diff[~band] == 0).all()
    assert (diff[band] <= 1).all()
    assert not codes[zero].any()


# the issue's channel counts (their packed runs are 1, 3, 8, 24, 65, 129, 136 B:
# every non-8-bit one takes the element-wise path) plus one 4-byte-aligned run
# per sub-byte depth (68 B: the dword path, a second, ragged tile across)
QUANT_CASES = [(8, n) for n in (1, 8, 24, 136)] + [(4, n) for n in (2, 6, 130, 136)] + \
              [(2, n) for n in (4, 12, 516, 272)]


@pytest.mark.parametrize("nsblk,nrows,pad", GEOMS)
@pytest.mark.parametrize("nbits,nchan", QUANT_CASES)
def test_quantize_vs_numpy(hip_lib, nbits, nchan, nsblk, nrows, pad):
    x = _draws(nchan, nsblk, nrows, pad)
    b = _blocks(x, nsblk, nrows)
    d = _dev(x)
    for scale in ("minmax", "sigma"):
        offs, scl = _scaling(b, nbits, scale)
        packed, _, _ = _quantize(hip_lib, d, nchan, nsblk, nrows, scl, offs, nbits)
        _check_codes(_unpack(packed, nbits), b, scl, offs, nbits)


def test_quantize_half_values_clamp_nan_and_zero_scale(hip_lib):
    """scl = 1, offs = 0: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2 (half to even), -3 -> 0
    and 300 -> 255 (clamp), NaN -> 0; the same samples with scl = 0 -> 0."""
    x = np.array([[0.5, 1.5, 2.5, -3.0, 300.0, np.nan] * 2], dtype=np.float32)
    scl = np.array([[1.0], [0.0]], dtype=np.float32)
    offs = np.zeros((2, 1), dtype=np.float32)
    packed, _, _ = _quantize(hip_lib, _dev(x), 1, 6, 2, scl, offs, 8)
    np.testing.assert_array_equal(packed[0, :, 0], [0, 2, 2, 0, 255, 0])
    np.testing.assert_array_equal(packed[1], 0)


@pytest.mark.parametrize("nbits,nchan,nsblk", [(8, 24, 100), (4, 6, 7), (2, 272, 64)])
def test_quantize_chunk_offset_and_guard(hip_lib, nbits, nchan, nsblk):
    """Rows 1 and 2 of a four-row grid through an offset input pointer, into
    an output with 0xA5 guard regions on both sides: the guards stay intact
    and the bytes are those of the whole-grid call."""
    nrows, k, n, guard = 4, 1, 2, 256
    x = _draws(nchan, nsblk, nrows, 3 if nsblk % 4 else 0)
    b = _blocks(x, nsblk, nrows)
    d = _dev(x)
    offs, scl = _scaling(b, nbits, "sigma")
    whole, _, _ = _quantize(hip_lib, d, nchan, nsblk, nrows, scl, offs, nbits)
    part, before, after = _quantize(hip_lib, d, nchan, nsblk, n, scl[k:k + n], offs[k:k + n], nbits,
                                    col0=k * nsblk, guard=guard)
    assert (before == 0xA5).all() and (after == 0xA5).all()
    np.testing.assert_array_equal(part, whole[k:k + n])
    _check_codes(_unpack(part, nbits), b[k:k + n], scl[k:k + n], offs[k:k + n], nbits)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
DT = 20.48e-6


@pytest.fixture(scope="module")
def observed(hip_lib):
    """A 16-channel search-mode signal of 8192 samples: pulses, dispersion,
    radiometer noise."""
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile
    from psrsigsim_amd.ism import ISM
    from psrsigsim_amd.telescope import Telescope, Receiver, Backend
    from psrsigsim_amd._units import Quantity
    pss.seed(4242)
    sig = FilterBankSignal(1400, 400, Nsubband=16, fold=False, dtype=np.float32)
    psr = Pulsar(0.005, 1.0, profiles=GaussProfile(0.5, 0.05, 1))
    psr.make_pulses(sig, tobs=(8192 + 0.5) * DT)
    ISM().disperse(sig, 30)
    tel = Telescope(20.0, area=None, Tsys=25.0, name="T")
    tel.add_system(name="S", receiver=Receiver(fcent=1400, bandwidth=400, name="L"),
                   backend=Backend(samprate=1.0 / (2 * Quantity(DT, "s")), name="B"))
    tel.observe(sig, psr, system="S", noise=True)
    assert tuple(sig.data.shape) == (16, 8192)
    return sig, psr


def _count_calls(monkeypatch, hip_lib):
    calls = []
    real = hip_lib.pss_quantize_tmajor

    def counted(*a):
        calls.append(a[4])                           # nrows of the chunk
        return real(*a)
    monkeypatch.setattr(hip_lib, "pss_quantize_tmajor", counted)
    return calls


def test_search_file_end_to_end_8bit_minmax(observed, hip_lib, tmp_path, monkeypatch):
    from psrsigsim_amd.io import PSRFITS, read_search_data, read_psrfits
    sig, psr = observed
    before = sig.data.cpu().numpy().copy()
    calls = _count_calls(monkeypatch, hip_lib)
    path = str(tmp_path / "search8.fits")
    PSRFITS(path, obs_mode="SEARCH").save(sig, psr, nbits=8, nsblk=1024, max_stage_bytes=2 * 1024 * 16)
    assert len(calls) >= 3 and sum(calls) == 8, calls
    after = sig.data.cpu().numpy()
    assert before.tobytes() == after.tobytes()
    codes, values, prim, sub = read_search_data(path)
    _, _, rec = read_psrfits(path)
    assert rec.shape == (8,) and codes.shape == (16, 8192) and values.shape == (16, 8192)
    assert prim["OBS_MODE"] == "SEARCH" and prim["OBSNCHAN"] == 16
    assert sub["NBITS"] == 8 and sub["NSBLK"] == 1024 and sub["NBIN"] == 1 and sub["NCHAN"] == 16
    assert sub["NPOL"] == 1 and sub["POL_TYPE"] == "AA+BB" and sub["ZERO_OFF"] == 0 and sub["SIGNINT"] == 0
    assert sub["NSUBOFFS"] == 0 and sub["CHAN_BW"] == 25.0 and sub["DM"] == 30.0
    samprate = float(sig.samprate.value) * 1e6
    assert abs(sub["TBIN"] * samprate - 1.0) <= 2.0 ** -52
    np.testing.assert_array_equal(rec["DAT_FREQ"][3], np.asarray(sig.dat_freq.value, dtype=np.float64))
    np.testing.assert_array_equal(rec["DAT_WTS"], 1.0)
    np.testing.assert_array_equal(rec["TSUBINT"], 1024 * sub["TBIN"])
    np.testing.assert_array_equal(rec["OFFS_SUB"], (np.arange(8) + 0.5) * (1024 * sub["TBIN"]))
    scl = np.repeat(np.asarray(rec["DAT_SCL"], dtype=np.float64).T, 1024, axis=1)      # [nchan][nsamp]
    err = np.abs(values.astype(np.float64) - after.astype(np.float64))
    bound = (0.5 + BAND * 255) * scl
    print("max err / bound", (err / bound).max())
    assert (err <= bound).all()                      # minmax: nothing clips
    # one chunk: the same file
    one = str(tmp_path / "search8_one.fits")
    del calls[:]
    PSRFITS(one, obs_mode="SEARCH").save(sig, psr, nbits=8, nsblk=1024)
    assert calls == [8]
    assert open(one, "rb").read() == open(path, "rb").read()


def test_search_file_end_to_end_4bit_sigma(observed, hip_lib, tmp_path):
    from psrsigsim_amd.io import PSRFITS, read_search_data, read_psrfits
    sig, psr = observed
    data = sig.data.cpu().numpy().astype(np.float64)
    path = str(tmp_path / "search4.fits")
    PSRFITS(path, obs_mode="SEARCH").save(sig, psr, nbits=4, nsblk=1024, scale="sigma",
                                          max_stage_bytes=3 * 1024 * 8)
    codes, values, prim, sub = read_search_data(path)
    _, _, rec = read_psrfits(path)
    assert sub["NBITS"] == 4 and rec["DATA"].shape[1:] == (1024, 1, 8, 1)
    scl = np.repeat(np.asarray(rec["DAT_SCL"], dtype=np.float64).T, 1024, axis=1)
    offs = np.repeat(np.asarray(rec["DAT_OFFS"], dtype=np.float64).T, 1024, axis=1)
    # DAT_OFFS = mu - 2 sigma, DAT_SCL = 8 sigma / 15 of every block (float32 of the float64 formulas)
    b = data.reshape(16, 8, 1024)
    mu, sd = b.mean(axis=2), b.std(axis=2)
    # (1e-6 of the terms' size: float32 rounding of the result, float64 sums behind it)
    assert (np.abs(np.asarray(rec["DAT_OFFS"]).T - (mu - 2.0 * sd)) <= 1e-6 * (np.abs(mu) + 2.0 * sd)).all()
    np.testing.assert_allclose(np.asarray(rec["DAT_SCL"]).T, 8.0 * sd / 15, rtol=1e-6)
    u = (data - offs) / scl
    inside = (u >= 0) & (u <= 15)
    assert inside.mean() > 0.5 and (~inside).any()
    err = np.abs(values.astype(np.float64) - data)
    assert (err[inside] <= ((0.5 + BAND * 15) * scl)[inside]).all()
    assert (codes[u < 0] == 0).all() and (codes[u > 15] == 15).all()


def test_save_simulation_routes_search_format(observed, hip_lib, tmp_path):
    """Simulation.save_simulation(out_format='psrfits_search') needs no
    template and writes the same file as the writer called directly."""
    from psrsigsim_amd.io import PSRFITS
    from psrsigsim_amd.simulate import Simulation
    sig, psr = observed
    sim = Simulation.__new__(Simulation)
    sim._signal, sim._pulsar, sim._tempfile = sig, psr, None
    a, b = str(tmp_path / "a.fits"), str(tmp_path / "b.fits")
    sim.save_simulation(outfile=a, out_format="psrfits_search", nbits=2, nsblk=2048)
    PSRFITS(b, obs_mode="SEARCH").save(sig, psr, nbits=2, nsblk=2048, MJD_start=55999.9861)
    assert open(a, "rb").read() == open(b, "rb").read()
