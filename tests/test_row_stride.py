"""The row pitch the library gets for a [rows, N] tensor (_engine.row_stride:
max(stride(0), N)).  torch reports an arbitrary stride for a one-row tensor --
``torch.empty(N, 1).t()`` is contiguous with stride (1, 1) -- and the entry
points reject ld < N, so the callers that passed a bare stride(0) (the fused
run, filter_rows, utils.shift_t / down_sample / rebin, Backend.fold /
fold_periods) failed on such a row."""
import numpy as np
import pytest
import torch

from psrsigsim_amd import _engine

N = 100


def test_row_stride_on_the_host():
    one = torch.empty(N, 1).t()
    assert tuple(one.shape) == (1, N) and one.stride(0) == 1 and one.is_contiguous()
    assert one.contiguous().stride(0) == 1                   # (.contiguous() does not mend it)
    assert _engine.row_stride(one) == N
    padded = torch.empty(3, N + 4)
    assert _engine.row_stride(padded[1:2, :N]) == N + 4      # one row of padded rows keeps their pitch
    assert _engine.row_stride(torch.empty(3, N)) == N
    assert _engine.row_stride(padded[:, :N]) == N + 4
    assert isinstance(_engine.row_stride(one), int)


def test_plane_rows_uses_it():
    from psrsigsim_amd.telescope.plane import PlaneStage
    one = torch.zeros(N, 1).t()
    data, ld = PlaneStage._plane_rows(one)
    assert data is one and ld == N
    data, ld = PlaneStage._plane_rows(torch.zeros(3, N + 4)[:, :N])
    assert ld == N + 4


def _one_row():
    """A one-row device tensor with stride (1, 1), and the same values with stride (N, 1)."""
    x = torch.from_numpy(np.random.default_rng(5).random((N, 1)).astype(np.float32)).cuda().t()
    assert tuple(x.shape) == (1, N) and x.stride(0) == 1
    # (x.clone() keeps the stride (1, 1))
    return x, torch.empty_strided((1, N), (N, 1), dtype=torch.float32, device=x.device).copy_(x)


@pytest.mark.gpu
def test_utils_on_a_one_row_transpose(hip_lib):
    from psrsigsim_amd.utils import shift_t, down_sample, rebin
    x, c = _one_row()
    assert c.stride(0) == N
    for fn, arg in ((shift_t, 0.3), (down_sample, 5), (rebin, 7)):
        got, ref = fn(x, arg).cpu().numpy(), fn(c, arg).cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), fn.__name__
    assert np.array_equal(x.cpu().numpy(), c.cpu().numpy())  # shift_t returns a new tensor


@pytest.mark.gpu
def test_fold_periods_on_a_one_channel_transpose(hip_lib):
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.telescope import Backend
    x, c = _one_row()
    out = []
    for buf in (x, c):
        sig = FilterBankSignal(1400, 400, Nsubband=1, fold=False)
        sig._buf, sig._ncols, sig._nsamp = buf, N, N
        out.append(Backend(samprate=0.01, name="B").fold_periods(sig, None, nbin=7).cpu().numpy())
    assert out[0].shape == (1, 7) and np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
    ref = x.cpu().numpy().astype(np.float64)[0, :98].reshape(14, 7).sum(axis=0)
    assert np.allclose(out[0][0], ref, rtol=1e-6)
