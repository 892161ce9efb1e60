"""Shared by the exact tests of the text, atomics and streaming kernels
(test_text_exact.py, test_atomics_exact.py, test_elementwise_exact.py): the
``dev`` fixture that runs one test body on the CPU backend (unmarked) and on
the HIP kernels (``gpu`` mark), seeded data, and offset views.
"""
import numpy as np
import pytest
import torch


@pytest.fixture(params=["cpu", pytest.param("gpu", marks=pytest.mark.gpu)])
def dev(request):
    if request.param == "cpu":
        return torch.device("cpu")
    return request.getfixturevalue("gpu")


def seeded(*key):
    """A generator seeded by the key's characters (``hash`` of a str changes
    from run to run)."""
    return np.random.default_rng([int(b) for b in repr(key).encode()])


def view_at(a: np.ndarray, off: int, dev) -> torch.Tensor:
    """``a`` on ``dev`` as a contiguous view that starts ``off`` elements into
    a fresh allocation: the allocation is aligned far beyond 16 bytes, so the
    view's address is ``off`` elements past an aligned one."""
    a = np.ascontiguousarray(a)
    buf = torch.zeros(a.size + off, dtype=torch.from_numpy(a[:0].copy()).dtype, device=dev)
    v = buf[off:]
    v.copy_(torch.from_numpy(a.copy()))
    assert v.is_contiguous() and (a.size == 0 or v.data_ptr() % 16 == (off * a.itemsize) % 16)
    return v


LETTERS = np.arange(97, 123, dtype=np.uint8)
UPPER = np.arange(65, 91, dtype=np.uint8)
NON_LETTERS = np.array([0, 10, 32, 48, 64, 91, 96, 123, 127, 128, 200, 255], dtype=np.uint8)


def draw(key, n: int, alphabet) -> np.ndarray:
    alphabet = np.asarray(alphabet, dtype=np.uint8)
    return alphabet[seeded(key, n).integers(0, alphabet.size, n)]
