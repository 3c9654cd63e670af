"""What the batch entries' wrappers take for "a batch of rows" (minimodem_amd._row_view, _row_lengths),
on CPU tensors: the view is a function of shape, strides and dtype alone.  The expected values are
written out by hand."""
import pytest
import torch

import minimodem_amd as M


def view(t, **kw):
    return M._row_view(torch, t, cuda=False, **kw)


def fields(v):
    return (v.nstreams, v.width, v.stride, v.s16, v.vec)


def test_one_dimension_is_one_row():
    x = torch.zeros(8)
    v = view(x)
    assert fields(v) == (1, 8, 8, False, 4)
    assert tuple(v.t.shape) == (1, 8) and v.t.data_ptr() == x.data_ptr()
    with pytest.raises(AssertionError):
        view(x, one_row=False)


def test_a_lone_row_holds_whole_vectors():
    with pytest.raises(AssertionError, match="multiple of 4 samples"):
        view(torch.zeros(6))
    with pytest.raises(AssertionError, match="multiple of 8 floats"):
        view(torch.zeros((1, 12), dtype=torch.int16), unit="floats")
    assert fields(view(torch.zeros(6), whole=False)) == (1, 6, 6, False, 4)
    # (with more rows than one the stride says where they lie: the library judges it)
    assert fields(view(torch.zeros((2, 6)))) == (2, 6, 6, False, 4)


def test_rows_of_a_wider_tensor_keep_its_stride():
    big = torch.zeros((3, 48))
    v = view(big[:, :40])
    assert fields(v) == (3, 40, 48, False, 4)
    assert fields(view(big[:, 4:44])) == (3, 40, 48, False, 4)


def test_pcm16_rows():
    assert fields(view(torch.zeros((3, 40), dtype=torch.int16))) == (3, 40, 40, True, 8)


def test_samples_of_a_row_are_contiguous():
    with pytest.raises(AssertionError):
        view(torch.zeros((40, 3)).t())


def test_kinds_the_entry_does_not_take():
    with pytest.raises(AssertionError, match="kind"):
        view(torch.zeros((3, 40), dtype=torch.int16), dtypes=(torch.float32,))
    with pytest.raises(AssertionError, match="kind"):
        view(torch.zeros((3, 40), dtype=torch.float64))
    with pytest.raises(AssertionError, match="kind"):          # complex64 only where the entry names it
        view(torch.zeros((2, 12), dtype=torch.complex64), cx=True)
    assert fields(view(torch.zeros((3, 32), dtype=torch.uint8), dtypes=(torch.uint8,))) == (3, 32, 32, False, 16)


@pytest.mark.parametrize("make, s16, vec", [
    (lambda: torch.zeros((2, 12), dtype=torch.complex64), False, 2),
    (lambda: torch.zeros((2, 12, 2), dtype=torch.float32), False, 2),
    (lambda: torch.zeros((2, 12, 2), dtype=torch.int16), True, 4),
])
def test_complex_rows_count_in_complex_elements(make, s16, vec):
    v = view(make(), cx=True, dtypes=(torch.float32, torch.int16, torch.complex64))
    assert fields(v) == (2, 12, 12, s16, vec)
    assert tuple(v.t.shape) == (2, 12, 2) and v.t.dtype == (torch.int16 if s16 else torch.float32)
    big = torch.zeros((2, 20, 2), dtype=torch.int16 if s16 else torch.float32)
    assert fields(view(big[:, :12], cx=True)) == (2, 12, 20, s16, vec)


def test_one_complex_row():
    v = view(torch.zeros((12, 2)), cx=True)
    assert fields(v) == (1, 12, 12, False, 2) and tuple(v.t.shape) == (1, 12, 2)
    with pytest.raises(AssertionError):
        view(torch.zeros((12, 2)), cx=True, one_row=False)
    with pytest.raises(AssertionError, match="multiple of 2 elements"):
        view(torch.zeros((11, 2)), cx=True, unit="elements")
    with pytest.raises(AssertionError, match="interleaved"):
        view(torch.zeros((2, 12, 3)), cx=True)
    with pytest.raises(AssertionError, match="interleaved"):
        view(torch.zeros((2, 2, 12)).transpose(1, 2), cx=True)


def test_complex_rows_an_odd_number_of_floats_apart():
    flat = torch.zeros(2 * 25)
    rows = torch.as_strided(flat, (2, 12, 2), (25, 2, 1))
    with pytest.raises(AssertionError, match="interleaved"):
        view(rows, cx=True)
    assert fields(view(torch.as_strided(flat, (2, 12, 2), (26, 2, 1)), cx=True)) == (2, 12, 13, False, 2)


def test_a_device_tensor_is_asked_for_at_the_door():
    with pytest.raises(AssertionError):
        M._row_view(torch, torch.zeros(8))


def lengths(n, nstreams=3, width=40, **kw):
    return M._row_lengths(torch, n, nstreams, width, cuda=False, **kw)


def test_lengths():
    assert lengths(None) == (None, 40)
    assert lengths(5, allow_int=True) == (None, 5)
    with pytest.raises(AssertionError):
        lengths(5)
    n = torch.tensor([0, 5, 40], dtype=torch.int32)
    assert lengths(n) == (n.data_ptr(), 40)
    assert lengths(n, allow_int=True) == (n.data_ptr(), 40)
    with pytest.raises(AssertionError, match="int32/uint32"):
        lengths(torch.tensor([0, 5, 40], dtype=torch.int64))
    with pytest.raises(AssertionError):
        lengths(torch.tensor([0, 5], dtype=torch.int32))
    with pytest.raises(AssertionError):
        lengths(torch.tensor([[0, 5, 40]], dtype=torch.int32))
    with pytest.raises(AssertionError):
        lengths(torch.zeros(6, dtype=torch.int32)[::2])
    with pytest.raises(AssertionError, match="CUDA"):
        M._row_lengths(torch, n, 3, 40)
