"""The kernel-test harness (tests/kernel_harness.py) against a fake kernel: a
Python function that writes into CPU tensors.  Every guard the GPU kernel
tests rely on must catch one stray word; a clean write must pass."""
import numpy as np
import pytest

from tests import kernel_harness as kh

ROWS, VALID, OUT_LD = 3, 10, 13
GUARDS = {np.float32: -7.0, np.int32: -77}


def _output(dtype, out_off):
    return kh.GuardedOutput(ROWS, VALID, OUT_LD, out_off=out_off, guard=GUARDS[dtype], dtype=dtype, device="cpu")


def _values(dtype):
    return (np.arange(ROWS * VALID).reshape(ROWS, VALID) + 1).astype(dtype)


def fake_kernel(out, values):
    """Writes the valid part of every row, as a kernel that stays in bounds does."""
    import torch
    out.view[:, :VALID] = torch.from_numpy(values)


# where a stray word lands, as an index into the parent of an output at `lead`
STRAY = {
    "the word before the view": lambda lead: lead - 1,
    "the word after the view": lambda lead: lead + ROWS * OUT_LD,
    "a pad column of the first row": lambda lead: lead + VALID,
    "a pad column of the last row": lambda lead: lead + (ROWS - 1) * OUT_LD + VALID,
    "the last pad column of the last row": lambda lead: lead + ROWS * OUT_LD - 1,
}


@pytest.mark.parametrize("out_off", [0, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.int32], ids=["float32", "int32"])
def test_clean_write_passes_and_returns_the_valid_part(dtype, out_off):
    out = _output(dtype, out_off)
    assert out.ptr == out.parent.data_ptr() + 4 * (kh.OUT_PAD + out_off)
    fake_kernel(out, _values(dtype))
    got = out.read()
    assert got.dtype == dtype and got.shape == (ROWS, VALID) and np.array_equal(got, _values(dtype))
    assert np.array_equal(out.rows_with_pad()[:, :VALID], got)
    assert (out.rows_with_pad()[:, VALID:] == GUARDS[dtype]).all()
    got[0, 0] = 0                                            # a copy: the parent is left alone
    assert np.array_equal(out.read(), _values(dtype))


@pytest.mark.parametrize("where", sorted(STRAY))
@pytest.mark.parametrize("out_off", [0, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.int32], ids=["float32", "int32"])
def test_one_stray_word_fails_read(dtype, out_off, where):
    out = _output(dtype, out_off)
    fake_kernel(out, _values(dtype))
    out.parent[STRAY[where](kh.OUT_PAD + out_off)] = 1
    with pytest.raises(AssertionError):
        out.read()


@pytest.mark.parametrize("dtype", [np.float32, np.int32], ids=["float32", "int32"])
def test_untouched_fails_after_any_write(dtype):
    out = _output(dtype, 1)
    out.untouched()
    out.read()                                               # nothing written: the guards hold
    flat = kh.GuardedOutput(1, 24, guard=GUARDS[dtype], dtype=dtype, device="cpu")      # a flat output
    flat.untouched()
    assert flat.read().shape == (1, 24)
    for o, index in ((out, kh.OUT_PAD + 1), (out, kh.OUT_PAD + 1 + ROWS * OUT_LD - 1), (out, 0), (flat, kh.OUT_PAD + 23),
                     (flat, kh.OUT_PAD + 24)):
        o.parent.fill_(GUARDS[dtype])
        o.untouched()
        o.parent[index] = 1
        with pytest.raises(AssertionError):
            o.untouched()
    # a valid write alone: read passes, untouched does not
    out.parent.fill_(GUARDS[dtype])
    fake_kernel(out, _values(dtype))
    out.read()
    with pytest.raises(AssertionError):
        out.untouched()


@pytest.mark.parametrize("guard_rows,pad", [(0, kh.IN_PAD), (2, kh.IN_PAD), (0, 5 * 13)])
@pytest.mark.parametrize("in_off", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(3, 10), (3, 10, 2)], ids=["real", "complex"])
def test_input_view_sits_where_asked_between_guards(shape, in_off, guard_rows, pad):
    guard = float(1 << 20)
    vals = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    ld = 13
    g = kh.GuardedInput(vals, ld, in_off=in_off, guard=guard, guard_rows=guard_rows, pad=pad, device="cpu")
    width = 2 if len(shape) == 3 else 1
    assert tuple(g.view.shape) == (3, ld) + shape[2:] and g.view.stride(0) == ld * width
    assert g.ptr == g.view.data_ptr() and g.ptr % 4 == 0
    # the requested pointer offset
    assert (g.ptr // 4) % 4 == (g.base + in_off) % 4 and g.ptr // 4 == g.base + in_off
    lead = pad + guard_rows * ld * width
    assert g.base == g.parent.data_ptr() // 4 + lead
    assert g.parent.numel() == lead + in_off + (3 + guard_rows) * ld * width + pad
    # the values, and the guard in every other word: lead, guard rows, pad columns, tail
    assert np.array_equal(g.view[:, :10].numpy(), vals)
    p = g.parent.numpy().copy()
    body = p[lead + in_off:lead + in_off + 3 * ld * width].reshape((3, ld) + shape[2:])
    assert (body[:, 10:] == guard).all()
    body[:, :10] = guard
    assert (p == guard).all()
    assert (p == guard).sum() == p.size and p.size - vals.size >= 2 * (pad + guard_rows * ld * width)


IN_LD = 13
# (guard_rows, pad) of the in-place rows: the kernel tests' padding with and
# without guard rows, and a pad of 5 whole rows
IN_PLACE = [(0, kh.IN_PAD), (2, kh.IN_PAD), (2, 5 * IN_LD)]


def _rows_in_place(shape, in_off, guard_rows, pad):
    vals = np.random.default_rng(2).standard_normal(shape).astype(np.float32)
    return vals, kh.GuardedRows(vals, IN_LD, in_off=in_off, guard=float(1 << 20), guard_rows=guard_rows, pad=pad,
                                device="cpu")


def fake_in_place_kernel(g):
    """Doubles the valid part of every row, as an in-place kernel that stays in bounds does."""
    g.rows.mul_(2.0)


def _stray_in_place(g, where, width):
    """An index into the parent of ``g`` inside the named region (None where the layout has no such region)."""
    sizes = dict(g.regions)
    start = dict(zip([n for n, _ in g.regions], np.cumsum([0] + [w for _, w in g.regions])))
    row = IN_LD * width
    if where == "the first pad column of the first row":
        return int(start["rows"]) + VALID * width
    if where == "the last pad column of the last row":
        return int(start["rows"]) + ROWS * row - 1
    name, end = where
    if not sizes[name]:
        return None
    return int(start[name]) + (sizes[name] - 1 if end == "last" else 0)


STRAY_IN_PLACE = ["the first pad column of the first row", "the last pad column of the last row"] + [
    (name, end) for name in ("the lead pad", "the guard rows before", "the in_off slack", "the guard rows after",
                             "the tail pad") for end in ("first", "last")]


@pytest.mark.parametrize("guard_rows,pad", IN_PLACE)
@pytest.mark.parametrize("in_off", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(ROWS, VALID), (ROWS, VALID, 2)], ids=["real", "complex"])
def test_in_place_clean_write_passes_and_returns_the_valid_part(shape, in_off, guard_rows, pad):
    vals, g = _rows_in_place(shape, in_off, guard_rows, pad)
    assert tuple(g.rows.shape) == shape and g.rows.data_ptr() == g.ptr and g.rows.stride(0) == g.view.stride(0)
    assert sum(w for _, w in g.regions) == g.parent.numel()
    assert np.array_equal(g.read(), vals)                    # nothing written yet
    fake_in_place_kernel(g)
    got = g.read()
    assert got.dtype == np.float32 and np.array_equal(got, 2 * vals)
    got[0, 0] = 0                                            # a copy: the parent is left alone
    assert np.array_equal(g.read(), 2 * vals)


@pytest.mark.parametrize("where", STRAY_IN_PLACE, ids=lambda w: w if isinstance(w, str) else "%s word of %s" % (w[1], w[0]))
@pytest.mark.parametrize("guard_rows,pad", IN_PLACE)
@pytest.mark.parametrize("in_off", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(ROWS, VALID), (ROWS, VALID, 2)], ids=["real", "complex"])
def test_in_place_one_stray_word_fails_read_and_names_the_region(shape, in_off, guard_rows, pad, where):
    vals, g = _rows_in_place(shape, in_off, guard_rows, pad)
    fake_in_place_kernel(g)
    index = _stray_in_place(g, where, len(shape) - 1)
    if index is None:
        # (no guard rows, or in_off = 0: the region is empty in this layout and the clean read stands)
        assert np.array_equal(g.read(), 2 * vals)
        return
    g.parent[index] = 1
    with pytest.raises(AssertionError) as err:
        g.read()
    assert ("pad columns" if isinstance(where, str) else where[0]) in str(err.value), str(err.value)
    g.parent[index] = float(1 << 20)                         # the guard put back: that word alone failed it
    assert np.array_equal(g.read(), 2 * vals)


def test_small_pieces():
    a = np.array([0.0, -0.0, np.nan], dtype=np.float32)
    assert kh.same_bits(a, a.copy()) and not kh.same_bits(a, np.array([0.0, 0.0, np.nan], dtype=np.float32))
    assert not kh.same_bits(a, a[:2])
    assert [kh.odd(v) for v in (4, 5)] == [5, 5]
    assert list(kh.misaligned_layouts(8, 16, 7, 9, in_off=2)) == [
        dict(ld=7, out_ld=9, in_off=2, out_off=1), dict(ld=8, out_ld=16, in_off=2, out_off=0),
        dict(ld=7, out_ld=16, in_off=0, out_off=0), dict(ld=8, out_ld=9, in_off=0, out_off=1)]
    calls = []

    @kh.once
    def ref(name, n=3):
        calls.append(name)
        return np.zeros(n), dict(x=np.ones(2), k=[1, 2]), [np.ones(1)], "s"

    r = ref("a")
    assert ref("a") is r and ref("b") is not r and ref("a", 4)[0].size == 4 and calls == ["a", "b", "a"]
    for arr in (r[0], r[1]["x"], r[2][0]):
        with pytest.raises(ValueError):
            arr[0] = 5.0
