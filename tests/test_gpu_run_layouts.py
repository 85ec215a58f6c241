"""The fused run (pss_run, pss_shift_rows, pss_filter_rows) on strided,
guarded rows, on every FFT path.

``load_search_signal`` and ``Backend.channelize`` hand out signals whose
buffer is a [:, :nsamp] view of padded rows, and the engine passes the row
stride straight through (PssPipeline.ld), so ld > nsamp is a product path.
Here the signal's buffer is swapped, before the first read-out, for a strided
view inside a guarded parent (``kernel_harness.GuardedRows``, two guard rows):

  padded         base on the 16-byte grid, ld = N + 4 (N rounded up to a
                 multiple of 4 where it is none)
  off the grid   the four layouts of ``kernel_harness.misaligned_layouts``:
                 ld odd and the base 3 floats off, the base alone (2 floats),
                 the odd stride alone, the base alone (1 float)

and every run must give THE SAME BITS as the same run (same seed, same calls)
on a contiguous buffer -- no kernel's arithmetic depends on an address -- and
leave every other word of the parent alone.  Loaded rows sit in 2^20: a read
outside a row lands in an FFT and moves every sample of the row.

The launch plan: the padded layout notes exactly the contiguous run's tokens;
off the grid the search-mode fast pass C (16-byte stores, gated by on_grid16 in
fast_epilogue) gives way to the generic one with pass A unchanged, the fold-mode
fast pass C (scalar stores, no gate) stays.

Lengths: the smallest of each kernel family (tests/fft_geometries.py).
Variant 0 is a load with per-row delays (also tied to the float64 oracle, per
row max|d| / max|ref| <= 1e-5, on the all-off-grid layout: a bug shared by
both layouts cannot pass as "the same bits"), 1 a delayed null (generic
kernels), 2 the scattering tail; "search" and "fold" are the fast passes.
"""
import numpy as np
import pytest

from tests import fft_geometries as G
from tests import kernel_harness as kh
from tests import replay
from tests.kernel_harness import engine_seed_restored  # noqa: F401 (autouse here)
from tests.test_gpu_fft_geometries import _fold_signal, _search_signal
from tests.test_gpu_tail import _signal

pytestmark = pytest.mark.gpu
TOL = 1e-5                    # BASELINE north_star, as G.check_shift_rows
IN_GUARD = float(1 << 20)
C_FAST = ("C:fast", "C:fast32", "C:cols16x2", "C:null", "N:fix_list")
BYTE_GUARD = 0xA5


def _layouts(N, which="all"):
    """(name, dict(ld, in_off)): the padded layout and the four off the grid
    (``which`` = "two": the padded and the all-off-grid one)."""
    ld = N + 4 if N % 4 == 0 else (N + 3) // 4 * 4
    odd = kh.odd(ld)
    a = list(kh.misaligned_layouts(ld, ld, odd, odd, in_off=3))
    b = list(kh.misaligned_layouts(ld, ld, odd, odd, in_off=2))
    out = [("padded", dict(ld=ld, in_off=0)),
           ("all-off-grid", dict(ld=a[0]["ld"], in_off=a[0]["in_off"])),
           ("base-off-2", dict(ld=b[1]["ld"], in_off=b[1]["in_off"])),
           ("odd-stride", dict(ld=a[2]["ld"], in_off=a[2]["in_off"])),
           ("base-off-1", dict(ld=a[3]["ld"], in_off=a[3]["out_off"]))]      # (in place: the output is the input)
    for name, lay in out:
        on = lay["ld"] % 4 == 0 and lay["in_off"] == 0
        assert lay["ld"] > N and on == (name == "padded"), (name, lay)
    return out if which == "all" else out[:2]


def _place(sig, layout, guard=IN_GUARD):
    """Swap the buffer of ``sig`` for a guarded strided one (its values, or
    zeros where the source generates them); returns read() -> the data after
    the run, guards asserted.  ``layout`` None: the contiguous buffer."""
    import torch
    N, rows = sig._ncols, sig._c1 - sig._c0
    if layout is None:
        if sig._buf is not None:
            assert sig._buf.stride(0) == N
        return lambda: sig.data.cpu().numpy()
    vals = sig._buf.cpu().numpy() if sig._buf is not None else np.zeros((rows, N), np.float32)
    g = kh.GuardedRows(vals, layout["ld"], in_off=layout["in_off"], guard=guard, guard_rows=2)
    sig._buf = g.rows

    def read():
        data = sig.data
        assert data.data_ptr() == g.ptr and data.stride(0) == layout["ld"]
        torch.cuda.synchronize()
        return g.read()
    return read


def _nchan(N):
    return 3 if N < 1 << 22 else 2                           # (3: one lone pair)


def _shifts(N, R):
    return np.array([0.37, -1234.5678, 3.0 * N + 17.25][:R])        # G.check_shift_rows'


def _delay_input(N):
    return np.random.default_rng(N).random((_nchan(N), N)).astype(np.float32)


def _run(N, variant, layout):
    """One fused run of ``variant`` at N samples on ``layout``: (data, plan lines)."""
    from psrsigsim_amd import _lib
    from psrsigsim_amd.ism import ISM
    from psrsigsim_amd.ism.ism import push_delay
    from psrsigsim_amd.telescope import telescope as T
    nchan = _nchan(N)
    L = _lib.lib()
    old = L.pss_set_flags(_lib.FLAG_NO_FAST) if variant == 1 else None
    _lib.plan_collect()
    try:
        if variant == 0:
            sig = _signal(nchan, N, _delay_input(N))
            read = _place(sig, layout)
            push_delay(sig, _shifts(N, nchan) * sig._dt_ms())
        elif variant == 2:                                   # tests/test_gpu_tail.py's chain
            sig = _signal(nchan, N, np.random.default_rng(N).random((nchan, N)) * 10)
            read = _place(sig, layout)
            ISM().scatter_broaden(sig, 1e-4, 1500.0, tail=True)
            push_delay(sig, np.linspace(3.0, 9.0, nchan))
        elif variant == "fold":
            sig, psr = _fold_signal(3, None, 30, 2048)
            assert sig._ncols == N
            read = _place(sig, layout)
            T.Arecibo().observe(sig, psr, system="Lband_PUPPI", noise=True)
        else:
            # a period of 16 samples where the default's 244 do not fit the row
            period = 0.005 if N >= 1000 else 16.5 * 20.48e-6
            sig, psr = _search_signal(N, nchan, variant != "search-no-null", period=period)
            assert sig._pending.null is not None or variant == "search-no-null"
            read = _place(sig, layout)
            T.Arecibo().observe(sig, psr, system="Lband_PUPPI", noise=True)
        got = read()
        return got, _lib.plan_collect()                      # (assert_plan takes the last nchan x N run: not null()'s probe)
    finally:
        if old is not None:
            L.pss_set_flags(old)


def _tokens(line):
    return set(line.split(":", 1)[1].split())


def _contiguous_tokens(N, variant):
    """The tokens a contiguous run must note (the geometry's, and the fast passes')."""
    g = G.of_length(N, {0: 0, 1: 1, 2: 2, "search": 1, "search-no-null": 0, "fold": 0}[variant])
    tok = g.tokens
    if variant == "search":
        assert g.search_fast, g
        tok += G.fast_tokens(g, shared_profile=True) + ("N:table", "N:fix_list")
        tok += ("C:null",) if (g.n1, g.n2) == (1024, 4096) else ()
    elif variant == "search-no-null":
        assert g.search_fast, g
        tok += G.fast_tokens(g, shared_profile=True)
    elif variant == "fold":
        assert g.fold_fast == ("A:fold", "C:fold"), g
        tok += g.fold_fast
    elif variant == 1 and g.kind == "fourstep":
        tok += ("A:generic", "C:generic")
    return g, tok


def _check_layouts(N, variant, which):
    nchan = _nchan(N)
    g, tok = _contiguous_tokens(N, variant)
    want, lines = _run(N, variant, None)
    line = replay.assert_plan(lines, nchan, N, tok)
    print("%s N=%d %s contiguous: %s" % (G.gid(g), N, variant, line))
    assert want.shape == (nchan, N) and np.isfinite(want).all() and want.std() > 0
    fast_c = variant in ("search", "search-no-null")
    for name, lay in _layouts(N, which):
        got, lines = _run(N, variant, lay)
        if name == "padded" or not fast_c:
            # (the fold fast pass C stores scalars: it stays off the grid too)
            got_line = replay.assert_plan(lines, nchan, N, tok)
            assert _tokens(got_line) == _tokens(line), (name, got_line, line)
        else:
            pass_a = tuple(t for t in _tokens(line) if t.startswith("A:"))
            got_line = replay.assert_plan(lines, nchan, N, g.tokens + pass_a + ("C:generic",), absent=C_FAST)
            assert {t for t in _tokens(got_line) if t.startswith("A:")} == set(pass_a), (name, got_line)
        print("%s N=%d %s %s %r: %s" % (G.gid(g), N, variant, name, lay, got_line))
        same = kh.same_bits(got, want)
        assert same, "%s: %d of %d samples differ from the contiguous run (first at %s)" % (
            name, int((got.view(np.uint32) != want.view(np.uint32)).sum()), want.size,
            np.argwhere(got.view(np.uint32) != want.view(np.uint32))[0])
        if variant == 0 and name == "all-off-grid":
            _oracle_tie(N, got)


def _oracle_tie(N, got):
    """The strided delay rows against the float64 oracle (G.check_shift_rows' bound)."""
    from oracle import pss_cpu as O
    x = _delay_input(N)
    s = _shifts(N, x.shape[0])
    for r in range(x.shape[0]):
        ref = O.shift_t(x[r].astype(np.float64), float(s[r]), dt=1.0)
        err = np.max(np.abs(got[r] - ref)) / np.max(np.abs(ref))
        print("oracle tie N=%d row %d: %.3g" % (N, r, err))
        assert err <= TOL, (N, r, err)


# (N, variant, layouts): the issue's table, one smallest length per kernel family
CASES = (
    [(66, v, "all") for v in (0, 1, 2)] +                                    # direct
    [(n, v, "all") for n in (64, 8192) for v in (0, 1, 2)] +                 # single
    [(1 << 14, v, "all") for v in (0, 1, 2, "search")] +                     # four-step 16 x 1024 (C:fast)
    [(1 << 22, "search", "all")] +                                           # 1024 x 4096 (C:null, f-dependent fix-up)
    [(1 << 24, "search", "two")] +                                           # 2048 x 8192 (C:fast32)
    [(6144, v, "all") for v in (0, 2)] +                                     # mixed radix, LDS columns 6 x 1024
    [(98304, v, "all") for v in (0, "search-no-null")] +                     # register columns 12 x 8192
    [(61440, "fold", "all")] +                                               # fold fast 30 x 2048
    [(3125000, 0, "two")] +                                                  # radix-5 1250 x 2500
    [(8194, v, "all") for v in (0, 1, 2)] +                                  # Bluestein 8 x 4096, pair fused
    [((1 << 22) + 2, 0, "two")])                                             # Bluestein 4096 x 4096, pair unfused


def test_cases_are_each_family_s_smallest_length(hip_lib):
    """The lengths above against the geometry table: no split is written down here."""
    for kind, n1, n2, N in (("direct", 0, 0, 66), ("single", 1, 64, 64), ("single", 1, 8192, 8192),
                            ("fourstep", 16, 1024, 1 << 14), ("fourstep", 1024, 4096, 1 << 22),
                            ("smooth", 6, 1024, 6144), ("smooth", 12, 8192, 98304), ("smooth", 30, 2048, 61440),
                            ("smooth", 1250, 2500, 3125000), ("bluestein", 8, 4096, 8194),
                            ("bluestein", 4096, 4096, (1 << 22) + 2)):
        assert G.find(kind, n1, n2, 0).nsamp == N and G.of_length(N, 0) == G.find(kind, n1, n2, 0)
    assert G.find("fourstep", 2048, 8192, 1).nsamp == 1 << 24
    assert {n for n, _, _ in CASES if n % 4 == 2} == {66, 8194, (1 << 22) + 2}         # the ragged last items


@pytest.mark.parametrize("N,variant,which", CASES, ids=["%d-%s" % (n, v) for n, v, _ in CASES])
def test_run_on_strided_guarded_rows(N, variant, which, hip_lib):
    _check_layouts(N, variant, which)


# ---------------------------------------------------------------------------
# null()'s probe of channel 0 on a signal shorter than one period
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("in_off", [0, 1])
def test_null_probe_stops_at_the_end_of_a_short_row(in_off, hip_lib):
    """N = 66 samples, a period of Nph = 244: the reference's
    ``data[0, :Nph]`` is the whole row, so shift_val = Nph // 2 - argmax(row 0).
    The rows sit between 2^20 guards, above every sample: a scan past the
    row's end meets them (another argmax, or a tie)."""
    import torch
    from psrsigsim_amd import _engine
    N, nph = 66, 244
    x = np.random.default_rng(66).random((3, N)).astype(np.float32)
    x[0, 5], x[1, 7] = 2.0, 3.0                              # (row 1 holds a larger value: it is not scanned)
    sig = _signal(3, N, x)
    g = kh.GuardedRows(x, 69, in_off=in_off, guard=IN_GUARD, guard_rows=2)
    sig._buf = g.rows
    out = _engine.null_shift_device(sig, _engine.Pending(None), nph)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == [nph // 2 - 5, 0]
    assert kh.same_bits(g.read(), x)
    # a whole period fits: the scan is the first nph samples, the shift count // 2 - argmax as before
    out = _engine.null_shift_device(sig, _engine.Pending(None), 4)
    assert out.cpu().numpy().tolist() == [2 - int(np.argmax(x[0, :4])), 0]


def test_null_on_a_signal_shorter_than_one_period(hip_lib):
    """The search chain at N = 66 with the default 5 ms period (244 samples,
    nsub = 0: no pulse is nulled, but null() still measures the shift, as the
    reference does): the probe replays channels 0..1 into a 2 x 66 scratch
    and must scan 66 samples of it, not 244; the read-out raises nothing."""
    sig, psr = _search_signal(66, 3, True)
    assert psr._nph(sig) == 244 and sig._pending.null is None and len(sig._null_checks) == 1
    shift = sig._null_checks[0][0].cpu().numpy()
    checks = list(sig._null_checks)
    data = sig.data.cpu().numpy()                            # (check_null_status passes)
    assert checks[0][1] == 244 and data.shape == (3, 66)
    assert shift.tolist() == [244 // 2 - int(np.argmax(data[0])), 0]


# ---------------------------------------------------------------------------
# observe()'s full-rate copy (PssPipeline.out: rows at stride N, float32 / int8)
# ---------------------------------------------------------------------------
def _observe_copy(N, dtype, layout):
    """The search chain with a delayed null and observe()'s full-rate copy
    (telescope.py's ``kind == "copy"`` branch with the copy in a guarded
    tensor of this test's): (data, copy)."""
    import torch
    from psrsigsim_amd import _lib
    from psrsigsim_amd.telescope import telescope as T
    sig, psr = _search_signal(N, 3, True, dtype=dtype)
    read = _place(sig, layout)
    tel = T.Arecibo()
    rcvr, bak = tel.systems["Lband_PUPPI"]
    assert tel.resample_branch(sig, bak)[0] == "copy"
    if dtype is np.int8:
        G8 = 64
        buf = torch.full((G8 + 1 + 3 * N + G8,), BYTE_GUARD, dtype=torch.uint8, device="cuda")
        out, kind = buf[G8 + 1:G8 + 1 + 3 * N].view(torch.int8).view(3, N), _lib.OUT_I8
    else:
        gout = kh.GuardedOutput(3, N, out_off=1)
        out, kind = gout.view, _lib.OUT_F32
    sig._pend().out = {"kind": kind, "tensor": out, "clip": float(sig._draw_max)}
    rcvr.radiometer_noise(sig, psr, gain=tel.gain, Tsys=tel.Tsys)
    data = read()
    if dtype is np.int8:
        h = buf.cpu().numpy()
        assert (h[:G8 + 1] == BYTE_GUARD).all() and (h[G8 + 1 + 3 * N:] == BYTE_GUARD).all(), "written around the copy"
        return data, h[G8 + 1:G8 + 1 + 3 * N].view(np.int8).reshape(3, N).copy()
    return data, gout.read()


@pytest.mark.parametrize("dtype", [np.float32, np.int8], ids=["float32", "int8"])
def test_observe_full_rate_copy_on_strided_rows(dtype, hip_lib):
    N = 1 << 14
    want, want_copy = _observe_copy(N, dtype, None)
    got, got_copy = _observe_copy(N, dtype, dict(_layouts(N))["all-off-grid"])
    assert kh.same_bits(got, want)
    assert got_copy.dtype == dtype and np.array_equal(got_copy.view(np.uint8), want_copy.view(np.uint8))
    assert want_copy.std() > 0 and not np.array_equal(want_copy.astype(np.float32), want)      # (pre-noise)


# ---------------------------------------------------------------------------
# odd length (shift_rows_odd) and the transfer-function run, through the C ABI
# ---------------------------------------------------------------------------
def _shift_rows(hip_lib, t, N, ld, shifts):
    from psrsigsim_amd import _engine, _lib
    R = len(shifts)
    ramp = _engine.u64_to_i64_tensor(_engine.ramp_words(shifts, N))
    nyq = _engine.to_dev(np.cos(np.pi * np.asarray(shifts)).astype(np.float32))
    ws = _engine.workspace(_lib.load().pss_workspace_bytes(R, N))
    rc = hip_lib.pss_shift_rows(_engine.ptr(t), R, N, ld, _engine.ptr(ramp), _engine.ptr(nyq), _engine.ptr(ws),
                                _engine.stream_ptr())
    _lib.check(rc, "shift_rows")


@pytest.mark.parametrize("ld,in_off", [(1003, 0), (1003, 1), (1004, 0), (1004, 1)])
def test_shift_rows_odd_length_on_strided_rows(ld, in_off, hip_lib):
    """N = 999: the first N - 1 columns are the shifted row (the reference's
    irfft returns N - 1 samples); column N - 1 is as the contiguous call
    leaves it and the pad holds the guard."""
    import torch
    N, R = 999, 3
    x = np.random.default_rng(999).random((R, N)).astype(np.float32)
    shifts = _shifts(N, R)
    c = torch.from_numpy(x).cuda()
    _shift_rows(hip_lib, c, N, N, shifts)
    want = c.cpu().numpy()
    assert not np.array_equal(want[:, :N - 1], x[:, :N - 1])
    g = kh.GuardedRows(x, ld, in_off=in_off, guard=IN_GUARD, guard_rows=2)
    _shift_rows(hip_lib, g.rows, N, ld, shifts)
    torch.cuda.synchronize()
    got = g.read()
    assert kh.same_bits(got[:, :N - 1], want[:, :N - 1])
    assert kh.same_bits(got[:, N - 1:], want[:, N - 1:])


@pytest.mark.parametrize("N", [4096, 8194])
def test_filter_rows_on_strided_rows(N, hip_lib):
    """pss_filter_rows (single pass at 4096, Bluestein at 8194) with the
    transfer function of test_gpu_baseband.test_filter_rows_vs_numpy."""
    import torch
    from psrsigsim_amd import _engine, _lib
    rng = np.random.default_rng(N)
    x = rng.standard_normal((3, N)).astype(np.float32)
    H = np.exp(1j * 2 * np.pi * rng.random(N // 2 + 1) * 50.0)

    class _S:
        def __init__(self, t):
            self.data = t

    g = G.of_length(N, 2)
    s = _S(torch.from_numpy(x).cuda())
    _lib.plan_collect()
    _engine.filter_rows(s, H)
    want = s.data.cpu().numpy()
    line = replay.assert_plan(_lib.plan_collect(), 3, N, g.tokens)
    ref = np.fft.irfft(np.fft.rfft(x.astype(np.float64), axis=1) * H.astype(np.complex64), axis=1)
    assert (np.max(np.abs(want - ref), axis=1) / np.max(np.abs(ref), axis=1)).max() <= TOL
    for name, lay in _layouts(N):
        rows = kh.GuardedRows(x, lay["ld"], in_off=lay["in_off"], guard=IN_GUARD, guard_rows=2)
        _engine.filter_rows(_S(rows.rows), H)
        torch.cuda.synchronize()
        got = rows.read()
        assert _tokens(replay.assert_plan(_lib.plan_collect(), 3, N, g.tokens)) == _tokens(line), name
        assert kh.same_bits(got, want), name


# ---------------------------------------------------------------------------
# end to end: a loaded search file (padded rows) through ISM.disperse
# ---------------------------------------------------------------------------
def test_loaded_search_file_disperses_as_its_contiguous_copy(hip_lib, tmp_path):
    """nsamp = 2 x 4097 = 8194 (Bluestein, ragged last item), so the loader
    pads its rows to ld = 8196.  The loader's 2 pad columns cannot be reached
    from the signal: values only."""
    from psrsigsim_amd.io import load_search_signal
    from psrsigsim_amd.ism import ISM
    from tests.search_load_ref import random_case, write_search_file
    nchan, nsblk, nrows = 3, 4097, 2
    codes, scl, offs = random_case(8, nchan, nsblk, nrows)
    path = str(tmp_path / "padded.fits")
    write_search_file(path, codes, scl, offs, np.ones((nrows, nchan), dtype=np.float32),
                      1200.0 + 12.5 * np.arange(nchan), 8, tbin=64e-6, obsfreq=1400.0, obsbw=400.0)
    out = []
    for contiguous in (False, True):
        sig = load_search_signal(path)
        assert sig._ncols == 8194 and tuple(sig._buf.shape) == (nchan, 8194) and sig._buf.stride(0) == 8196
        if contiguous:
            sig._buf = sig._buf.contiguous()
            assert sig._buf.stride(0) == 8194
        before = sig._buf.cpu().numpy()
        ISM().disperse(sig, 10)
        data = sig.data
        assert data.stride(0) == (8194 if contiguous else 8196)
        out.append(data.cpu().numpy())
        assert not np.array_equal(out[-1], before)
    assert kh.same_bits(out[0], out[1])
