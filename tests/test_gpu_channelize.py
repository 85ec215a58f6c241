"""Baseband channeliser / detector and amplitude radiometer noise on the GPU.

``pss_channelize`` is checked against the float64 NumPy restatement of its
definition written here (``ref_channelize``):

    y_m[j]    = sum_{t<T} h[t L + j] x[(m + t) L + j]            (L = 2 C)
    X_m[k]    = sum_j y_m[j] exp(-2 pi i j k / L)
    out[k][s] = 1/(L ts) sum_pol sum_{m = s ts}^{(s+1) ts - 1} |X_m[k]|^2,  k < C

Tolerance (per output value, no sample excluded).  A float32 FFT of length L
has a norm-wise error ||dX|| <= gamma ||X||, gamma = c log2(L) 2^-24, and
||X||^2 = L sum(y^2) (Parseval), so every bin of a frame is off by at most
gamma sqrt(L e_m), e_m = sum_j y_m[j]^2.  Squaring, summing over the frames and
polarisations of an output value and Cauchy-Schwarz give

    |out - ref| <= 2 gamma sqrt(ref E) + gamma^2 E,   E = sum(e_m) / ts.

The constant: the smallest c at which SciPy's single-precision pocketfft
restatement (float32 tap sums, ``scipy.fft.rfft`` of float32 frames, float32
powers) passes on the same inputs over every case below is C_POCKETFFT = 0.178
(computed on the CPU by ``pocketfft_constant()``: 0.1777 at the worst case,
(64, 4, 1, 2, 33), rounded up); the device is allowed C_DEVICE = 4 x that,
because its inter-stage twiddles come from v_sin / v_cos at 1.2e-7 absolute
error where pocketfft's are correctly rounded, and its radix-16 stages sum in
another order.

The API, the chain baseband pulses -> channelize -> fold_periods, the noise
statistics and search-mode PSRFITS output of the channelised signal follow.
"""
import numpy as np
import pytest

from tests import kernel_harness as kh
from tests.kernel_harness import engine_seed_restored  # noqa: F401 (autouse here)

pytestmark = pytest.mark.gpu

C_POCKETFFT = 0.178
C_DEVICE = 4 * C_POCKETFFT

# (C, T, tscrunch, Npol, M)
CASES = [
    (16, 1, 1, 2, 1),          # one frame
    (16, 1, 3, 1, 17),         # ragged scrunch group; odd frame count for the two-frames packing
    (64, 4, 1, 2, 33),         # PFB halo across workgroups
    (512, 8, 2, 2, 40),        # largest tap count, with scrunching
    (2048, 1, 1, 1, 18),       # large C with a single polarisation
    (4096, 4, 1, 2, 35),       # largest transform; a full 16-sample group plus a ragged tail
]


def pfb(C, T):
    from psrsigsim_amd.telescope import Backend
    return Backend.pfb_coefficients(C, T)


def make_input(case):
    """Seeded normal x (1 + 0.5 pol) plus a tone of amplitude 30 at a bin
    centre (small bins next to large ones), float32; N leaves a tail of 5."""
    C, T, ts, npol, M = case
    L = 2 * C
    N = (M + T - 1) * L + 5
    rng = np.random.default_rng(1000 * C + 100 * T + 10 * ts + npol)
    x = rng.standard_normal((npol, N)) * (1.0 + 0.5 * np.arange(npol))[:, None]
    k0 = C // 3
    x += 30.0 * np.cos(2 * np.pi * k0 * np.arange(N) / L)[None, :]
    return x.astype(np.float32)


def ref_channelize(x, C, T, ts, dtype=np.float64):
    """(out [C][S], E [S]) in ``dtype`` arithmetic (float64: the reference;
    float32: the pocketfft restatement the tolerance constant comes from)."""
    import scipy.fft
    x = np.asarray(x, dtype=dtype)
    npol, N = x.shape
    L = 2 * C
    frames = N // L
    M = frames - T + 1
    S = M // ts
    h = pfb(C, T).astype(dtype)
    xf = x[:, :frames * L].reshape(npol, frames, L)
    y = np.zeros((npol, M, L), dtype=dtype)
    for t in range(T):
        y += h[t * L:(t + 1) * L][None, None, :] * xf[:, t:t + M, :]
    X = scipy.fft.rfft(y, axis=-1)[..., :C]
    assert X.dtype == (np.complex128 if dtype == np.float64 else np.complex64)
    P = (X.real ** 2 + X.imag ** 2).sum(axis=0)                      # [M][C]
    out = P[:S * ts].reshape(S, ts, C).sum(axis=1).T / dtype(L * ts)
    e = (y.astype(np.float64) ** 2).sum(axis=-1).sum(axis=0)         # [M]
    E = e[:S * ts].reshape(S, ts).sum(axis=1) / ts
    return out, E


def tolerance(ref, E, L, c):
    g = c * np.log2(L) * 2.0 ** -24
    return 2 * g * np.sqrt(ref * E[None, :]) + g * g * E[None, :]


def needed_c(got, ref, E, L):
    """The smallest c at which ``got`` passes (the root of the bound in gamma)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    Eb = np.broadcast_to(E[None, :], ref.shape)
    g = (np.sqrt(ref * Eb + Eb * d) - np.sqrt(ref * Eb)) / Eb
    return float(g.max() / (np.log2(L) * 2.0 ** -24))


def pocketfft_constant():
    """max over CASES of the c SciPy's float32 restatement needs (CPU only)."""
    worst = {}
    for case in CASES:
        C, T, ts, npol, M = case
        x = make_input(case)
        ref, E = ref_channelize(x, C, T, ts)
        got, _ = ref_channelize(x, C, T, ts, dtype=np.float32)
        worst[case] = needed_c(got, ref, E, 2 * C)
    return worst


@kh.once
def reference(case):
    """The float64 reference of a case, computed once and shared."""
    C, T, ts, npol, M = case
    x = make_input(case)
    return (x,) + ref_channelize(x, C, T, ts)


def run_kernel(hip_lib, x, C, T, ts, ld=None, out_ld=None, fill=-7.0):
    """pss_channelize on host array x [npol][N] (guarded views,
    tests/kernel_harness.py); returns (out [C][S], pad columns [C][out_ld - S])."""
    import torch
    from psrsigsim_amd import _lib
    npol, N = x.shape
    L = 2 * C
    S = (N // L - T + 1) // ts
    ld = N if ld is None else ld
    out_ld = S if out_ld is None else out_ld
    xd = kh.GuardedInput(x, ld, guard=float("nan"))           # (a read past n would poison the output)
    h = torch.from_numpy(pfb(C, T).astype(np.float32)).cuda()
    out = kh.GuardedOutput(C, S, out_ld, guard=fill)
    rc = hip_lib.pss_channelize(xd.ptr, npol, N, ld, h.data_ptr(), C, T, ts, out.ptr, out_ld, None)
    _lib.check(rc, "channelize")
    torch.cuda.synchronize()
    return out.read(), out.rows_with_pad()[:, S:]


@pytest.mark.parametrize("aligned", [True, False], ids=["vec", "elem"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "C%d_T%d_ts%d_p%d_M%d" % c)
def test_parity(case, aligned, hip_lib):
    C, T, ts, npol, M = case
    x, ref, E = reference(case)
    N = x.shape[1]
    S = ref.shape[1]
    assert S == M // ts and N == (M + T - 1) * 2 * C + 5
    if aligned:
        ld, out_ld = (N + 3) // 4 * 4 + 8, (S + 3) // 4 * 4 + 4      # 16-B loads and stores
    else:
        ld, out_ld = N + 3, S + 1                                    # rows off the 16-B grid
    got, pad = run_kernel(hip_lib, x, C, T, ts, ld=ld, out_ld=out_ld)
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert (pad == -7.0).all()                                       # nothing written past S
    tol = tolerance(ref, E, 2 * C, C_DEVICE)
    err = np.abs(got.astype(np.float64) - ref)
    print("case", case, "aligned", aligned, "needed c", needed_c(got, ref, E, 2 * C), "max err/tol",
          float((err / tol).max()))
    assert (err <= tol).all()


@pytest.mark.parametrize("case", CASES + [(1024, 2, 1, 2, 19)], ids=lambda c: "C%d_T%d_ts%d_p%d_M%d" % c)
def test_aligned_and_ragged_layouts_give_the_same_bits(case, hip_lib):
    """16-B loads and stores or element accesses, chosen separately from the
    alignment of the input and of the output: one set of bits."""
    C, T, ts, npol, M = case
    x, ref, _ = reference(case)
    N, S = x.shape[1], ref.shape[1]
    Na, Sa = (N + 3) // 4 * 4, (S + 3) // 4 * 4
    base, _ = run_kernel(hip_lib, x, C, T, ts, ld=Na + 8, out_ld=Sa + 4)          # loads 16 B, stores 16 B
    for ld, out_ld in ((Na + 8, Sa + 1), (Na + 7, Sa + 4), (Na + 5, Sa + 3)):      # one or both off the grid
        got, pad = run_kernel(hip_lib, x, C, T, ts, ld=ld, out_ld=out_ld)
        assert got.tobytes() == base.tobytes(), (ld, out_ld)
        assert (pad == -7.0).all()


def test_normal_add_same_bits_on_and_off_the_16_byte_grid(hip_lib):
    import torch
    from psrsigsim_amd import _lib
    n, rows = 4099, 3
    start = torch.arange(rows * 4104, dtype=torch.float32, device="cuda").reshape(rows, 4104) * 1e-3
    a = start.clone()                                   # ld 4104, aligned
    b = torch.zeros(rows * 4101 + 1, dtype=torch.float32, device="cuda")[1:].reshape(rows, 4101)
    b[:, :n] = start[:, :n]                             # base and ld off the grid
    for t in (a, b):
        _lib.check(hip_lib.pss_normal_add(t.data_ptr(), rows, n, t.stride(0), 0.75, 99, 3, None), "normal_add")
    torch.cuda.synchronize()
    assert a[:, :n].cpu().numpy().tobytes() == b[:, :n].cpu().numpy().tobytes()
    assert (a[:, n:] == start[:, n:]).all() and (b[:, n:] == 0).all()           # nothing past n
    z = (a[:, :n] - start[:, :n]).cpu().numpy() / 0.75
    assert abs(z.mean()) < 0.1 and abs(z.std() - 1.0) < 0.1


# the transform lengths the table above leaves out (every C is its own kernel
# instantiation): the same check at small shapes
EXTRA_CASES = [(32, 2, 2, 1, 9), (128, 1, 1, 2, 37), (256, 3, 2, 1, 21), (1024, 2, 1, 2, 19), (1024, 1, 3, 1, 7)]


@pytest.mark.parametrize("case", EXTRA_CASES, ids=lambda c: "C%d_T%d_ts%d_p%d_M%d" % c)
def test_parity_other_lengths(case, hip_lib):
    C, T, ts, npol, M = case
    x, ref, E = reference(case)
    got, pad = run_kernel(hip_lib, x, C, T, ts, ld=x.shape[1] + 7, out_ld=ref.shape[1] + 4)
    assert got.shape == ref.shape and (pad == -7.0).all()
    err = np.abs(got.astype(np.float64) - ref)
    print("case", case, "needed c", needed_c(got, ref, E, 2 * C))
    assert (err <= tolerance(ref, E, 2 * C, C_DEVICE)).all()


@pytest.mark.parametrize("npol", [1, 2])
@pytest.mark.parametrize("C", [16, 2048])
@pytest.mark.parametrize("k0", ["0", "1", "C-1"])
def test_tone_lands_in_its_channel(k0, C, npol, hip_lib):
    """A pure tone at a bin centre in pol 0 (T = 1): > 0.999 of each spectrum's
    power in channel k0 -- a mirrored or shifted band fails."""
    k0 = {"0": 0, "1": 1, "C-1": C - 1}[k0]
    L = 2 * C
    N = 5 * L
    x = np.zeros((npol, N), dtype=np.float32)
    x[0] = np.cos(2 * np.pi * k0 * np.arange(N) / L + 0.3)
    got, _ = run_kernel(hip_lib, x, C, 1, 1)
    assert got.shape == (C, 5)
    frac = got[k0].astype(np.float64) / got.astype(np.float64).sum(axis=0)
    assert (frac > 0.999).all(), frac


@pytest.mark.parametrize("C,ts,npol,frame", [(16, 3, 1, 7), (16, 3, 1, 10), (64, 1, 2, 37), (2048, 2, 1, 5),
                                             (4096, 1, 2, 17)])
def test_impulse_lands_in_its_time_sample(C, ts, npol, frame, hip_lib):
    """One unit impulse at sample n0 (T = 1): nonzero output only in time
    sample (n0 // L) // ts, flat across channels."""
    L = 2 * C
    nfr = frame + 2 * ts + 1
    n0 = frame * L + (L // 3)
    x = np.zeros((npol, nfr * L + 3), dtype=np.float32)
    x[npol - 1, n0] = 1.0
    got, _ = run_kernel(hip_lib, x, C, 1, ts)
    s = (n0 // L) // ts
    assert got.shape[1] == nfr // ts > s
    other = np.delete(got, s, axis=1)
    assert (other == 0.0).all()
    ref = np.full(C, 1.0 / (L * ts))
    E = np.array([1.0 / ts])
    tol = tolerance(ref[:, None], E, L, C_DEVICE)[:, 0]
    assert (np.abs(got[:, s].astype(np.float64) - ref) <= tol).all()


# ---------------------------------------------------------------------------
# API, chain, noise, output: one device-made baseband signal shared
# ---------------------------------------------------------------------------
BW = 0.512                      # MHz: 1.024 MHz sampling
PERIOD = 0.016                  # s: 16384 voltage samples, 128 channelised samples at C = 64
NSAMP = 1 << 21
TSYS, SMEAN = 100.0, 1e-5       # a noise scale of the order of the pulse amplitudes


def _make_bb():
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import BasebandSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile
    pss.seed(20240611)
    bb = BasebandSignal(1400, BW, Nchan=2)
    psr = Pulsar(PERIOD, SMEAN, profiles=GaussProfile(0.5, 0.05, 1), name="J0000+0000")
    psr.make_pulses(bb, (NSAMP + 0.5) / 1.024e6)
    return bb, psr


@pytest.fixture(scope="module")
def chain(hip_lib):
    """(bb, psr, fb): baseband pulses and their 64-channel detection."""
    from psrsigsim_amd.telescope import Backend
    bb, psr = _make_bb()
    assert tuple(bb.data.shape) == (2, NSAMP)
    fb = Backend(samprate=1.0, name="B").channelize(bb, 64)
    return bb, psr, fb


def test_api_equals_the_cabi_call_and_fills_the_signal(chain, hip_lib):
    import torch
    from psrsigsim_amd import _lib
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.telescope import Backend
    from psrsigsim_amd._units import to_value
    bb, psr, _ = chain
    be = Backend(samprate=1.0, name="B")
    C, T, ts = 64, 4, 2
    fb = be.channelize(bb, C, ntap=T, tscrunch=ts)
    S = (NSAMP // (2 * C) - T + 1) // ts
    d = bb.data
    h = torch.from_numpy(Backend.pfb_coefficients(C, T).astype(np.float32)).cuda()
    out = torch.empty((C, S), dtype=torch.float32, device="cuda")
    _lib.check(hip_lib.pss_channelize(d.data_ptr(), 2, NSAMP, d.stride(0), h.data_ptr(), C, T, ts, out.data_ptr(), S,
                                      None), "channelize")
    torch.cuda.synchronize()
    assert fb.data.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
    # S = 8190 here: the signal's rows sit on the 16-B grid, and what reads the
    # data by its row stride takes it as it is
    assert S % 4 and fb.data.stride(0) % 4 == 0 and fb.data.stride(1) == 1 and fb.data.data_ptr() % 16 == 0
    nbin = 64
    folded = be.fold_periods(fb, psr, nbin=nbin).cpu().numpy()
    want = out.cpu().numpy().astype(np.float64)[:, :S // nbin * nbin].reshape(C, S // nbin, nbin).sum(axis=1)
    np.testing.assert_allclose(folded, want, rtol=1e-6)
    again = be.channelize(bb, C, ntap=T, tscrunch=ts)
    assert again is not fb and again.data.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
    # the result object
    assert fb.sigtype == "FilterBankSignal" and fb.fold is False and fb.Nchan == C
    assert tuple(fb.data.shape) == (C, S) and fb.data.dtype == torch.float32 and fb._pending is None
    assert to_value(fb.fcent, "MHz") == 1400 and to_value(fb.bw, "MHz") == BW
    rate = 1.024 / (2 * C * ts)
    assert fb._samprate_MHz() == rate
    assert fb.nsamp == S and fb._ncols == S
    assert float(to_value(fb.tobs, "s")) == S / (rate * 1e6)
    assert float(to_value(fb.sublen, "s")) == PERIOD
    assert fb.nsub == int(np.round(S / (rate * 1e6) / PERIOD))
    assert float(to_value(fb._Smax, "Jy")) == float(to_value(bb._Smax, "Jy"))
    assert fb.dm is bb.dm and fb.delay is None
    assert fb._draw_norm == 1 and fb._draw_max == 200
    hand = FilterBankSignal(1400, BW, Nsubband=C, sample_rate=1000.0, fold=False)
    np.testing.assert_array_equal(np.asarray(fb.dat_freq.value), np.asarray(hand.dat_freq.value))
    # (np.arange(first, last, step) as the reference builds it: bin k at entry k)
    np.testing.assert_allclose(np.asarray(fb.dat_freq.value)[:C], 1400 - BW / 2 + np.arange(C) * BW / C, rtol=1e-14)
    # the stubs stay stubs
    with pytest.raises(NotImplementedError):
        bb.to_FilterBank()


def test_voltages_from_another_route_give_one_subint(hip_lib):
    """A baseband buffer that make_pulses did not fill carries no period: the
    detected signal is one subint spanning tobs (documented in channelize)."""
    import torch
    from psrsigsim_amd.signal import BasebandSignal
    from psrsigsim_amd.telescope import Backend
    from psrsigsim_amd._units import to_value
    bb = BasebandSignal(1400, BW, Nchan=1)
    n = 32 * 40 + 3
    bb._buf = torch.randn((1, n), dtype=torch.float32, device="cuda")
    bb._ncols = bb._nsamp = n
    fb = Backend(samprate=1.0, name="B").channelize(bb, 16, ntap=2, tscrunch=3)
    S = (40 - 1) // 3
    assert tuple(fb.data.shape) == (16, S) and fb.nsub == 1 and fb._Smax is None
    assert float(to_value(fb.sublen, "s")) == float(to_value(fb.tobs, "s"))
    assert float(to_value(fb.tobs, "s")) == pytest.approx(S / (1.024e6 / (32 * 3)), rel=1e-14)
    ref, _ = ref_channelize(bb._buf.cpu().numpy(), 16, 2, 3)
    np.testing.assert_allclose(fb.data.cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * ref.max())


def test_chain_pulses_channelize_fold(chain, hip_lib):
    """Every channel's folded profile follows the pulsar profile at the same
    phases (correlation > 0.9); the off-pulse floor is < 1e-6 of the peak."""
    from psrsigsim_amd.telescope import Backend
    bb, psr, fb = chain
    assert tuple(fb.data.shape) == (64, NSAMP // 128)
    folded = Backend(samprate=1.0, name="B").fold_periods(fb, psr).cpu().numpy().astype(np.float64)
    assert folded.shape == (64, 128)                                # one period = 128 channelised samples
    phases = (np.arange(128) + 0.5) / 128.0
    prof = np.asarray(psr.Profiles.calc_profiles(phases, Nchan=1), dtype=np.float64).reshape(-1, 128)[0]
    for k in range(64):
        assert np.corrcoef(folded[k], prof)[0, 1] > 0.9, k
    off = (phases < 0.1) | (phases > 0.9)
    assert folded[:, off].max() < 1e-6 * folded.max()


def test_noise_statistics_and_channelised_floor(hip_lib):
    from scipy import stats
    import psrsigsim_amd as pss
    from psrsigsim_amd.telescope import Backend, Receiver
    be = Backend(samprate=1.0, name="B")
    rcvr = Receiver(fcent=1400, bandwidth=BW, name="L")
    bb, psr = _make_bb()
    before = bb.data.cpu().numpy().copy()
    fb0 = be.channelize(bb, 64).data.cpu().numpy().astype(np.float64)
    norm = Receiver.amp_noise_norm(bb, psr, TSYS, 1.0)
    assert 0.1 < norm < 10.0
    rcvr.radiometer_noise(bb, psr, gain=1.0, Tsys=TSYS)
    after = bb.data.cpu().numpy().copy()
    n = NSAMP
    z1 = (after.astype(np.float64) - before) / norm
    for row in z1:
        # n normal draws: the mean has sampling error 1/sqrt(n), the variance sqrt(2/n)
        assert abs(row.mean()) < 5.0 / np.sqrt(n)
        assert abs(row.var() - 1.0) < 5.0 * np.sqrt(2.0 / n)
        assert stats.kstest(row[::16], "norm").pvalue > 0.01
    assert abs(np.corrcoef(z1[0], z1[1])[0, 1]) < 5.0 / np.sqrt(n)
    # channelised: white noise of variance norm^2 per polarisation adds
    # Npol norm^2 to every channel (sum h^2 = L); off pulse nothing else is
    # there.  A value is norm^2 (chi2_2 / 2 per pol; chi2_1 in the real bin 0):
    # variance 2 norm^4 (4 norm^4 in bin 0), independent across bins and frames
    fb1 = be.channelize(bb, 64).data.cpu().numpy().astype(np.float64)
    S = fb1.shape[1]
    phase = ((np.arange(S) + 0.5) / 128.0) % 1.0
    off = (phase < 0.1) | (phase > 0.9)
    noff = int(off.sum())
    rise = fb1[:, off].mean() - fb0[:, off].mean()
    sigma = norm ** 2 * np.sqrt(2.0 * 63 * noff + 4.0 * noff) / (64 * noff)
    assert abs(rise - 2 * norm ** 2) < 5 * sigma
    # a second call draws fresh values
    rcvr.radiometer_noise(bb, psr, gain=1.0, Tsys=TSYS)
    z2 = (bb.data.cpu().numpy().astype(np.float64) - after) / norm
    for r in range(2):
        assert abs(np.corrcoef(z1[r], z2[r])[0, 1]) < 5.0 / np.sqrt(n)
    # the same seed repeats the bits
    bb2, psr2 = _make_bb()
    rcvr.radiometer_noise(bb2, psr2, gain=1.0, Tsys=TSYS)
    assert bb2.data.cpu().numpy().tobytes() == after.tobytes()


def test_channelised_signal_to_search_psrfits(chain, hip_lib, tmp_path):
    from psrsigsim_amd.io import PSRFITS, read_search_data, read_psrfits
    bb, psr, fb = chain
    path = str(tmp_path / "chan.fits")
    PSRFITS(path, obs_mode="SEARCH").save(fb, psr, nbits=8, nsblk=1024)
    codes, values, prim, sub = read_search_data(path)
    _, _, rec = read_psrfits(path)
    S = NSAMP // 128
    assert sub["NCHAN"] == 64 and prim["OBSNCHAN"] == 64 and sub["NBITS"] == 8 and sub["NSBLK"] == 1024
    assert abs(sub["TBIN"] * (1.024e6 / 128) - 1.0) <= 2.0 ** -50
    assert codes.shape == (64, S) and values.shape == (64, S) and rec.shape == (S // 1024,)
    data = fb.data.cpu().numpy().astype(np.float64)
    scl = np.repeat(np.asarray(rec["DAT_SCL"], dtype=np.float64).T, 1024, axis=1)       # [nchan][nsamp]
    assert (np.abs(values.astype(np.float64) - data) <= scl).all()
