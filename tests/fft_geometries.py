"""Every FFT plan geometry the length classifier can select (pss_plan.hpp:
plan_geometry -> fourstep_split / smooth_split / bs_geom, exported as
pss_plan_geometry), one row each -- the table the GPU geometry tests
(tests/test_gpu_fft_geometries.py, the length sweep of tests/test_gpu_parity.py)
run over.  tests/test_host_plan.py sweeps the classifier and asserts that the
set of geometries it can return EQUALS this table and that each row's
``nsamp`` is the smallest length reaching it: a geometry added to the
dispatch without a row here (and so without a GPU test) fails the CPU suite.

A row:
  kind, n1, n2   pss_plan_geometry's answer ("single": 1 x N, "fourstep" /
                 "smooth": columns x rows, "direct": 0 x 0, "bluestein": the
                 M1 x M2 of the chirp-z convolution)
  variant        0 a delay only, 1 with a delayed null, 2 with a transfer
                 function or the scattering tail
  nsamp          the smallest even length that reaches the geometry
  tokens         the launch-plan tokens (pss_plan_collect) a run of it notes
  search_fast    the fast search-mode passes that exist for it (plan tokens;
                 "A:fast" reads "A:fast_shared" when all channels share one
                 profile row), () if none
  fold_fast      the fold-mode fast passes (register columns), () if none
  also           further lengths of the geometry the sweeps keep running
"""
from collections import namedtuple

Geom = namedtuple("Geom", "kind n1 n2 variant nsamp tokens search_fast fold_fast also")

VARIANTS = (0, 1, 2)

# power-of-two four-step: log2 N -> N1 x N2 (2^24: a plain delay takes
# 1024 x 16384, anything else 2048 x 8192)
_FOURSTEP = {14: (16, 1024), 15: (16, 2048), 16: (16, 4096), 17: (32, 4096), 18: (64, 4096), 19: (128, 4096),
             20: (256, 4096), 21: (512, 4096), 22: (1024, 4096), 23: (1024, 8192)}
# mixed-radix four-step: N1 -> row lengths N2 (N2 = the largest 2^m <= 8192
# that leaves N1 even, so the N1 with a factor 4 exist on 8192-point rows only)
_SMOOTH = {6: (1024, 2048, 4096, 8192), 10: (1024, 2048, 4096, 8192), 30: (1024, 2048, 4096, 8192),
           12: (8192,), 20: (8192,), 24: (8192,), 40: (8192,), 48: (8192,), 60: (8192,)}
# Bluestein: M1 -> (M2, smallest N = M1 M2 / 4 + 2, further lengths the sweeps run)
_BLUESTEIN = {8: (4096, 8194, (10006,)), 16: (4096, 16386, ()), 32: (4096, 32770, (51200,)),
              64: (4096, 65538, (100002,)), 128: (4096, (1 << 17) + 2, ()), 256: (4096, (1 << 18) + 2, ()),
              512: (4096, (1 << 19) + 2, ((1 << 20) - 2,)), 1024: (4096, (1 << 20) + 2, ()),
              2048: (4096, (1 << 21) + 2, ()), 4096: (4096, (1 << 22) + 2, ())}


def _fast_c(n1):
    """Tokens of the search-mode fast passes on n1-point columns."""
    if n1 == 2048:
        return ("A:fast", "C:fast32")
    if n1 == 1024:
        return ("A:fast", "C:fast", "C:cols16x2")
    return ("A:fast", "C:fast")


def _rows():
    out = []
    for v in VARIANTS:
        for m in range(6, 14):
            out.append(Geom("single", 1, 1 << m, v, 1 << m, ("single", "%d" % (1 << m)), (), (), ()))
        for m, (n1, n2) in sorted(_FOURSTEP.items()):
            out.append(Geom("fourstep", n1, n2, v, 1 << m, ("fourstep", "%dx%d" % (n1, n2)), _fast_c(n1), (), ()))
        n1, n2 = (1024, 16384) if v == 0 else (2048, 8192)
        out.append(Geom("fourstep", n1, n2, v, 1 << 24, ("fourstep", "%dx%d" % (n1, n2)), _fast_c(n1), (), ()))
        if v != 1:
            # (a delayed null off the 2^m lengths runs on the packed paths)
            for n1, rows in sorted(_SMOOTH.items()):
                for n2 in rows:
                    # whole 4-sample items per thread (the fast search passes) need 4 | N1
                    fast = ("A:fast", "C:fast") if n1 % 4 == 0 else ()
                    out.append(Geom("smooth", n1, n2, v, n1 * n2, ("smooth", "%dx%d" % (n1, n2)), fast,
                                    ("A:fold", "C:fold"), ()))
            out.append(Geom("smooth", 1250, 2500, v, 3125000, ("smooth", "1250x2500"), ("A:fast", "C:fast"), (), ()))
        out.append(Geom("direct", 0, 0, v, 66, ("direct",), (), (), (244, 1000)))
        for m1, (m2, n, also) in sorted(_BLUESTEIN.items()):
            # pair mode (two channels per complex row) unless a delayed null
            # rides in the imaginary part; its first / last passes fused for
            # M1 <= 2048
            mode = ("rows",) if v == 1 else (("pair", "fused") if m1 <= 2048 else ("pair",))
            out.append(Geom("bluestein", m1, m2, v, n, ("bluestein", "%dx%d" % (m1, m2)) + mode, (), (), also))
        out.append(Geom("bluestein", 4096, 8192, v, (1 << 23) + 2,
                        ("bluestein", "4096x8192") + (("rows",) if v == 1 else ("pair",)), (), (),
                        ((1 << 24) - 2,)))
    return tuple(out)


GEOMETRIES = _rows()


# The length sweep of tests/test_gpu_parity.py::test_shift_t_rows_vs_oracle
# (its test ids); tests/test_gpu_fft_geometries.py runs the delay-only rows'
# lengths that are not in it, so the two together run every variant-0 row.
PARITY_SWEEP = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 1 << 17, 1 << 18,
                1 << 20, 1 << 23, 244, 1000, 30720,
                # mixed-radix four-step: N1 x N2 = 6 x 2048, 10 x 4096, 30 x 2048, 30 x 4096, 24 x 8192
                12288, 40960, 61440, 122880, 196608,
                # Bluestein (chirp-z) fallback: M1 x M2 = 8 x 4096 (2 x 5003), 64 x 4096,
                # 512 x 4096 (2^20 - 2), 4096 x 8192 (2^24 - 2); and the reference
                # simulate fixture's 3 125 000 = 2^3 5^8 (radix-5 four-step 1250 x 2500)
                10006, 100002, (1 << 20) - 2, 3125000, (1 << 24) - 2)


def delay_lengths():
    """Every length of the delay-only rows: nsamp and ``also``, in table order."""
    return [n for g in GEOMETRIES if g.variant == 0 for n in (g.nsamp,) + g.also]


def check_shift_rows(N, tol=1e-5):
    """utils.shift_t on rows of N samples against the float64 oracle, per row
    max|d| / max|ref| <= tol, and the launch plan of the run against the
    table row of N's geometry.  3 rows (the odd count leaves a lone last
    pair), 2 above 2^18 samples, 1 above 2^22; shifts by a fraction of a
    sample, by a thousand samples backwards and by more than three rows."""
    import numpy as np
    from oracle import pss_cpu as O
    from psrsigsim_amd import _lib
    from psrsigsim_amd.utils import shift_t
    from tests import replay
    g = of_length(N, 0)
    rng = np.random.default_rng(N)
    R = 3 if N <= (1 << 18) else (2 if N <= (1 << 22) else 1)
    x = rng.random((R, N)).astype(np.float32)
    shifts = np.array([0.37, -1234.5678, 3.0 * N + 17.25][:R])
    _lib.plan_collect()
    got = shift_t(x, shifts, dt=1.0)
    replay.assert_plan(_lib.plan_collect(), R, N, g.tokens)
    for r in range(R):
        ref = O.shift_t(x[r].astype(np.float64), float(shifts[r]), dt=1.0)
        err = np.max(np.abs(got[r] - ref)) / np.max(np.abs(ref))
        print("shift_t %s N=%d row %d: %.3g" % (gid(g), N, r, err))
        assert err < tol, (N, r, err)


def rows(kind=None, variant=None):
    return [g for g in GEOMETRIES if (kind is None or g.kind == kind) and (variant is None or g.variant == variant)]


def find(kind, n1, n2, variant=0):
    """The table row of a geometry (KeyError if the table does not have it)."""
    for g in GEOMETRIES:
        if (g.kind, g.n1, g.n2, g.variant) == (kind, n1, n2, variant):
            return g
    raise KeyError((kind, n1, n2, variant))


def of_length(nsamp, variant=0):
    """The table row of the geometry a run of ``nsamp`` samples takes, by the
    library's own classifier (host only)."""
    from psrsigsim_amd import _lib
    return find(*_lib.plan_geometry(nsamp, variant), variant=variant)


def gid(g):
    """Test id of a row: kind, split and variant ("smooth-12x8192-v0")."""
    return "%s-%dx%d-v%d" % (g.kind, g.n1, g.n2, g.variant)


def fast_tokens(g, shared_profile):
    """The row's search fast tokens as a run notes them."""
    return tuple("A:fast_shared" if (t == "A:fast" and shared_profile) else t for t in g.search_fast)
