"""What the tests of the stand-alone search stages share (dedispersion, pulse
search, periodicity, acceleration, candidate fold, channeliser).

The kernel tests give a kernel views inside larger tensors whose every other
word holds a sentinel: ``GuardedInput`` (a stray read meets the sentinel and
lands in a result), ``GuardedOutput`` (``read`` asserts that nothing but
the valid part of every row was written) and ``GuardedRows`` (both, for rows
that a kernel updates in place).  These guard checks are the only
evidence that a kernel stays inside its rows, so there is one implementation,
and tests/test_kernel_harness.py runs it on the CPU against a fake kernel.

The rest are the small pieces the test files repeated: ``same_bits``, the
misalignment sweep, the compute-once cache of references, ``backend``, the
``engine_seed_restored`` fixture and the C ABI rejection loop of the host
tests.  Nothing here touches a device when it is imported.
"""
import functools

import numpy as np
import pytest

IN_PAD = 8192                # guard floats before and after an input
OUT_PAD = 64                 # guard words before and after an output


class GuardedInput(object):
    """``values`` [rows][valid] float32 (or [rows][valid][2]: complex rows) as
    a strided view, row stride ``ld`` elements, inside a parent tensor that
    holds ``guard`` everywhere else: ``pad`` floats and ``guard_rows`` whole
    rows before the view, the same after it, and the columns [valid, ld) of
    every row.  ``in_off`` floats move the view off the grid of the parent.

    ``view`` is the device view [rows][ld](,[2]), ``ptr`` its address, ``base``
    the word address (bytes / 4) the view has at in_off = 0.
    """

    def __init__(self, values, ld, in_off=0, guard=float(1 << 20), guard_rows=0, pad=IN_PAD, device="cuda"):
        import torch
        values = np.array(values, dtype=np.float32)
        rows, valid = values.shape[:2]
        assert ld >= valid and in_off >= 0
        row = ld * int(np.prod(values.shape[2:], dtype=np.int64))         # floats per row
        lead = pad + guard_rows * row
        self.parent = torch.full((lead + in_off + (rows + guard_rows) * row + pad,), guard, dtype=torch.float32,
                                 device=device)
        self.view = self.parent[lead + in_off:lead + in_off + rows * row].view((rows, ld) + values.shape[2:])
        self.view[:, :valid] = torch.from_numpy(values).to(device)
        self.ptr = self.view.data_ptr()
        self.base = self.parent.data_ptr() // 4 + lead
        self.guard, self.shape, self.ld = guard, values.shape, ld
        # the parent's regions in order (name, words); "rows" is the view
        self.regions = (("the lead pad", pad), ("the guard rows before", guard_rows * row), ("the in_off slack", in_off),
                        ("rows", rows * row), ("the guard rows after", guard_rows * row), ("the tail pad", pad))


class GuardedRows(GuardedInput):
    """A ``GuardedInput`` whose rows a kernel updates in place: ``rows`` is the
    device view [rows][valid] the kernel gets (stride ``ld``), and ``read``
    says afterwards that the kernel stayed inside it."""

    @property
    def rows(self):
        return self.view[:, :self.shape[1]]

    def read(self):
        """A host copy of the valid part [rows][valid], after asserting that
        every other word of the parent still holds the guard: the lead pad, the
        guard rows before and after, the in_off slack, the columns [valid, ld)
        of every row and the tail pad."""
        o = self.parent.cpu().numpy()
        at = 0
        for name, words in self.regions:
            part = o[at:at + words]
            at += words
            if name != "rows":
                assert (part == self.guard).all(), "written in %s" % name
                continue
            body = part.reshape((self.shape[0], self.ld) + self.shape[2:])
            bad = np.argwhere(body[:, self.shape[1]:] != self.guard)
            assert not bad.size, "written in the pad columns [%d, %d) of row %d" % (self.shape[1], self.ld, bad[0][0])
            got = body[:, :self.shape[1]].copy()
        assert at == o.size
        return got


class GuardedOutput(object):
    """An output of ``rows`` x ``valid`` words (float32 or int32), row stride
    ``out_ld``, at word OUT_PAD + ``out_off`` of a parent tensor that holds
    ``guard`` in every word.  A flat output is the one-row case.

    ``ptr`` is the output's address and ``view`` the device view [rows][out_ld].
    """

    def __init__(self, rows, valid, out_ld=None, out_off=0, guard=-7.0, dtype=np.float32, device="cuda"):
        import torch
        out_ld = valid if out_ld is None else out_ld
        assert out_ld >= valid and out_off >= 0
        self.rows, self.valid, self.out_ld, self.guard = rows, valid, out_ld, guard
        self.lead = OUT_PAD + out_off
        self.parent = torch.full((self.lead + rows * out_ld + OUT_PAD,), guard,
                                 dtype=getattr(torch, np.dtype(dtype).name), device=device)
        self.view = self.parent[self.lead:self.lead + rows * out_ld].view(rows, out_ld)
        self.ptr = self.view.data_ptr()

    def rows_with_pad(self):
        """A host copy of the rows [rows][out_ld], pad columns included (nothing asserted)."""
        o = self.parent.cpu().numpy()
        return o[self.lead:self.lead + self.rows * self.out_ld].reshape(self.rows, self.out_ld).copy()

    def read(self):
        """A host copy of the valid part [rows][valid], after asserting that
        the words before the output, behind it and in the columns [valid,
        out_ld) of every row still hold the guard."""
        o = self.parent.cpu().numpy()
        end = self.lead + self.rows * self.out_ld
        assert (o[:self.lead] == self.guard).all(), "written before the output"
        assert (o[end:] == self.guard).all(), "written behind the output"
        body = o[self.lead:end].reshape(self.rows, self.out_ld)
        assert (body[:, self.valid:] == self.guard).all(), "written past the valid part of a row"
        return body[:, :self.valid].copy()

    def untouched(self):
        """Asserts that every word of the parent still holds the guard."""
        assert (self.parent.cpu().numpy() == self.guard).all(), "an output that was not asked for was written"


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def odd(v):
    """v, or v + 1 where v is even."""
    return v + 1 - (v % 2)


def misaligned_layouts(ld, out_ld, odd_ld, odd_out_ld, in_off=1):
    """The four layouts a misalignment sweep compares with the aligned run
    (ld, out_ld on the grid): everything off the grid, the input's base alone,
    its row stride alone, the output alone."""
    yield dict(ld=odd_ld, out_ld=odd_out_ld, in_off=in_off, out_off=1)
    yield dict(ld=ld, out_ld=out_ld, in_off=in_off, out_off=0)
    yield dict(ld=odd_ld, out_ld=out_ld, in_off=0, out_off=0)
    yield dict(ld=ld, out_ld=odd_out_ld, in_off=0, out_off=1)


def _freeze(v):
    if isinstance(v, np.ndarray):
        v.setflags(write=False)
    elif isinstance(v, dict):
        _freeze(list(v.values()))
    elif isinstance(v, (tuple, list)):
        for x in v:
            _freeze(x)
    return v


def once(fn):
    """fn(*key) computed once per key and shared: every array in the result
    (inside tuples, lists and dicts too) is marked read-only."""
    store = {}

    @functools.wraps(fn)
    def shared(*key):
        if key not in store:
            store[key] = _freeze(fn(*key))
        return store[key]
    return shared


def backend(samprate=0.01):
    from psrsigsim_amd.telescope import Backend
    return Backend(samprate=samprate, name="B")


@pytest.fixture(autouse=True)
def engine_seed_restored():
    """For the modules whose tests seed the engine (they import it, which
    makes it autouse there): put its seed and call counter back, pass or fail."""
    from psrsigsim_amd import _engine
    saved = dict(_engine._state)
    yield
    _engine._state.update(saved)


def check_rejections(entry, good, cases, prefix=None):
    """The argument checks of a C ABI entry point.  ``good`` holds valid
    arguments by name in call order (the trailing stream is NULL); every
    (overrides, word) of ``cases`` must return PSS_EINVAL and leave a
    last_error() that holds ``word`` and begins with ``prefix``."""
    from psrsigsim_amd import _lib
    for kw, word in cases:
        assert set(kw) <= set(good), kw
        assert entry(*dict(good, **kw).values(), None) == _lib.PSS_EINVAL, kw
        err = _lib.last_error()
        assert word in err, (kw, err)
        assert prefix is None or err.startswith(prefix), err


def host_pointer():
    """A non-NULL pointer to host memory for the entry points' argument checks
    (they precede any launch: it is never dereferenced)."""
    import ctypes
    return ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)     # (the cast keeps the array alive)
