"""The hw3 text kernels (csrc/hip/text.hip) and their OpenMP twins, exactly:
every kernel against a plain numpy oracle (the ``ref_*`` functions of
ops/text.py, or one written here) at the sizes where the launch shape, the
grid-stride loop, a tile, a chunk or the 4-byte load changes, on empty input
and on views that start 1, 2 and 3 bytes past an aligned address.

Every test body runs on the CPU backend (unmarked) and on the HIP kernels
(``gpu``); the argument checks sit in the wrapper and run on the CPU.
"""
import numpy as np
import pytest
import torch
from text_util import LETTERS, NON_LETTERS, UPPER, dev, draw, seeded, view_at  # noqa: F401

from cme213x.ops import text as T

def host(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).copy())


def same(got: torch.Tensor, want: torch.Tensor, what):
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert torch.equal(got, want), what


# ============================================================== histogram_u8
# 1023..1025: one block of 256 lanes x 4 bytes; 1 048 576 + 5: the second trip
# of the grid-stride loop (the grid is capped at 1024 blocks x 1024 bytes)
HIST_N = [0, 1, 3, 4, 5, 1023, 1024, 1025, 4097, 1_048_576 + 5]
HIST_BINS = [(0, 256), (97, 26), (32, 100), (255, 1), (0, 1), (200, 256), (-3, 10)]


def hist_data(kind: str, n: int) -> np.ndarray:
    if kind == "random":
        return seeded("hist", n).integers(0, 256, n, dtype=np.uint8)
    if kind == "one":  # every lane adds to the same LDS word
        return np.full(n, 101, dtype=np.uint8)
    return np.full(n, 0xFF, dtype=np.uint8)  # "ff": the padded tail word is all 0xff as well


@pytest.mark.parametrize("kind", ["random", "one", "ff"])
@pytest.mark.parametrize("n", HIST_N)
def test_histogram_u8(dev, n, kind):
    a = hist_data(kind, n)
    offsets = (0, 1, 2, 3) if n <= 4097 or kind == "random" else (0, 1)
    want = {b: T.ref_histogram_u8(host(a), *b) for b in HIST_BINS}
    for off in offsets:
        x = view_at(a, off, dev)
        for lo, nbins in HIST_BINS:
            same(T.histogram_u8(x, lo, nbins), want[(lo, nbins)], (n, kind, off, lo, nbins))
    if kind == "one":
        assert int(T.histogram_u8(view_at(a, 1, dev))[101]) == n
    if kind == "ff":  # the 0xff that pad the last word are not data
        assert int(T.histogram_u8(view_at(a, 0, dev))[255]) == n
        assert int(T.histogram_u8(view_at(a, 3, dev), 255, 1)[0]) == n


def test_histogram_u8_arguments():
    x = torch.zeros(10, dtype=torch.uint8)
    for nbins in (0, -1, 257, 1000):
        with pytest.raises(ValueError):
            T.histogram_u8(x, 0, nbins)
    with pytest.raises(TypeError):
        T.histogram_u8(x.to(torch.int8))
    assert T.letter_histogram(x).tolist() == [0] * 26


# ========================================================= digraph_histogram
# 511..513 pairs' worth around one block; 300 001 bytes = 150 000 pairs, past
# the 512 blocks x 256 pairs of one trip of the grid
DIGRAPH_N = [0, 1, 2, 3, 511, 512, 513, 300_001]


@pytest.mark.parametrize("n", DIGRAPH_N)
def test_digraph_histogram(dev, n):
    # a third of the bytes are not lower-case letters: non-letters come first,
    # second and in both places of a pair
    a = draw("digraph", n, np.concatenate([LETTERS, LETTERS, NON_LETTERS, [65]]))
    for off in (0, 1):
        same(T.digraph_histogram(view_at(a, off, dev)), T.ref_digraph_histogram(host(a)), (n, off))
    if n % 2:  # the byte after the last whole pair is ignored
        same(T.digraph_histogram(view_at(a, 0, dev)), T.ref_digraph_histogram(host(a[:n - 1])), n)


@pytest.mark.parametrize("pair,count", [(b"ab", 1), (b"a ", 0), (b" b", 0), (b"  ", 0), (b"zz", 1), (b"A{", 0),
                                        (b"`a", 0), (b"a{", 0), (b"abc", 1), (b"ab d", 1), (b"a bc", 1), (b"a b ", 0),
                                        (b"abab", 2)])
def test_digraph_pairs(dev, pair, count):
    a = np.frombuffer(pair, dtype=np.uint8)
    got = T.digraph_histogram(view_at(a, 0, dev)).cpu()
    same(got, T.ref_digraph_histogram(host(a)), pair)
    assert int(got.sum()) == count


# ======================================================== residue_histograms
# 472 and 473: the last period whose [period][26] int table fits the 48 KiB of
# LDS (49 088 B) and the first that counts in global memory (49 192 B)
PERIODS = [1, 2, 26, 472, 473, 3000]
RESIDUE_N = [0, 5, 257, 200_003]  # 200 003: past the 512 x 256 bytes of one trip


@pytest.mark.parametrize("n", RESIDUE_N)
def test_residue_histograms(dev, n):
    a = draw("residue", n, np.concatenate([LETTERS, LETTERS, LETTERS, NON_LETTERS, UPPER[:3]]))
    x = view_at(a, 0, dev)
    for period in PERIODS + [n + 1]:  # n + 1: every residue holds at most one byte
        same(T.residue_histograms(x, period), T.ref_residue_histograms(host(a), period), (n, period))
    same(T.residue_histograms(view_at(a, 3, dev), 7), T.ref_residue_histograms(host(a), 7), (n, "offset"))


def test_residue_histograms_arguments():
    x = torch.full((10,), 97, dtype=torch.uint8)
    for period in (0, -1, -26):
        with pytest.raises(ValueError):
            T.residue_histograms(x, period)


# ============================================================== match_counts
MC_N = [0, 1, 2, 4095, 4096, 4097, 8209]  # tiles of 4096 bytes; 8209: three tiles
MC_NS = [0, 1, 3, 4, 5, 1024, 1025, 2049]  # four waves stride the shifts; batches of 1024 per launch


def mc_data(kind: str, n: int) -> np.ndarray:
    if kind == "two":  # about half of all pairs match
        return draw("mc", n, [97, 98])
    if kind == "random":
        return seeded("mc", n).integers(0, 256, n, dtype=np.uint8)
    return np.zeros(n, dtype=np.uint8)  # "zero": the tile's padding is 0 too


def mc_oracle(a: np.ndarray, s0: int, ns: int) -> np.ndarray:
    n = a.size
    return np.array([np.count_nonzero(a[s:] == a[:n - s]) if s < n else 0 for s in range(s0, s0 + ns)],
                    dtype=np.int64).reshape(ns)


@pytest.mark.parametrize("kind", ["two", "random", "zero"])
@pytest.mark.parametrize("n", MC_N)
def test_match_counts(dev, n, kind):
    a = mc_data(kind, n)
    x = view_at(a, 0, dev)
    for s0 in sorted({s for s in (0, 1, n - 1, n, n + 5) if s >= 0}):
        full = mc_oracle(a, s0, max(MC_NS))
        if kind == "zero":  # padding never matches: exactly the overlap
            assert full.tolist() == [max(n - s, 0) for s in range(s0, s0 + max(MC_NS))]
        for ns in MC_NS:
            same(T.match_counts(x, s0, ns), torch.from_numpy(full[:ns].copy()), (n, kind, s0, ns))
    same(T.match_counts(view_at(a, 1, dev), 1, 5), torch.from_numpy(mc_oracle(a, 1, 5)), (n, kind, "offset"))


def test_match_counts_arguments():
    x = torch.full((100,), 97, dtype=torch.uint8)
    for s0, ns in ((-1, 4), (-5, 10), (1, -1), (2**31 - 1, 1), (2**31 - 10, 11), (0, 2**31)):
        with pytest.raises(ValueError):
            T.match_counts(x, s0, ns)
    assert T.match_counts(x, 0, 1).tolist() == [100]  # shift 0 is legal and counts every byte
    assert T.match_counts(x, 2**31 - 11, 10).tolist() == [0] * 10
    assert T.match_counts(x, 5, 0).shape == (0,)


# ================================================================== sanitize
# 255..257: one row of a block; 4095..4097: one chunk; 8193, 12 289: two and
# three whole chunks and a byte
SAN_N = [0, 1, 255, 256, 257, 4095, 4096, 4097, 8193, 12_289]
SAN_KINDS = ["cycle", "kept", "none", "upper", "edges", "high"]


def san_data(kind: str, n: int) -> np.ndarray:
    if kind == "cycle":
        return (np.arange(n) % 256).astype(np.uint8)
    alphabet = {"kept": np.concatenate([LETTERS, UPPER]),
                "none": NON_LETTERS,
                "upper": UPPER,
                "edges": [64, 65, 90, 91, 96, 97, 122, 123],  # the bytes either side of A-Z and a-z
                "high": np.concatenate([np.arange(128, 256), [97, 90]])}[kind]
    return draw(("san", kind), n, alphabet)


@pytest.mark.parametrize("kind", SAN_KINDS)
def test_sanitize(dev, kind):
    for n in SAN_N:
        a = san_data(kind, n)
        want = T.ref_sanitize(host(a))
        if kind in ("kept", "upper"):
            assert want.numel() == n
        if kind == "none":
            assert want.numel() == 0
        for off in (0, 1) if n in (257, 4097) else (0,):
            same(T.sanitize(view_at(a, off, dev)), want, (kind, n, off))  # order and length


def test_sanitize_edge_bytes(dev):
    a = np.array([64, 91, 96, 123], dtype=np.uint8)
    assert T.sanitize(view_at(a, 0, dev)).numel() == 0
    a = np.array([64, 65, 90, 91, 96, 97, 122, 123, 193, 225], dtype=np.uint8)
    assert bytes(T.sanitize(view_at(a, 0, dev)).cpu().numpy()) == b"azaz"


def test_sanitize_many_blocks(dev):
    """4 194 304 + 4099 bytes: the 1024-block cap, with a chunk of 4101 bytes
    per block, which is no multiple of the 256 bytes a block scans at a time."""
    n = 4_194_304 + 4099
    a = san_data("cycle", n)
    same(T.sanitize(view_at(a, 0, dev)), T.ref_sanitize(host(a)), n)


# ================================================================== vigenere
VIG_N = [0, 1, 255, 257, 600_001]  # 600 001: past the 2048 blocks x 256 bytes of one trip
VIG_SHIFTS = [0, 1, 25, 26, 27, -1, -27, 1000, -1000, 2**31 - 1, -2**31]


def vig_oracle(a: np.ndarray, shifts: np.ndarray, decode: bool) -> torch.Tensor:
    t = a.astype(np.int64) - 97
    s = shifts.astype(np.int64)[np.arange(a.size) % shifts.size]
    return torch.from_numpy((np.mod(t - s if decode else t + s, 26) + 97).astype(np.uint8))


def vig_key(period: int, start: int = 0) -> np.ndarray:
    return np.array([VIG_SHIFTS[(start + i) % len(VIG_SHIFTS)] for i in range(period)], dtype=np.int64)


@pytest.mark.parametrize("n", VIG_N)
def test_vigenere(dev, n):
    texts = {"letters": draw("vig", n, LETTERS), "bytes": (np.arange(n) * 7 % 256).astype(np.uint8)}
    for period, start in [(1, 9), (1, 10), (2, 9), (123, 0), (n + 3, 5)]:
        key = vig_key(period, start)
        k = torch.from_numpy(key.astype(np.int32))
        for name, a in texts.items():
            x = view_at(a, 0, dev)
            enc = T.vigenere(x, k)
            same(enc, vig_oracle(a, key, False), (n, period, name, "encode"))
            same(T.vigenere(x, k, decode=True), vig_oracle(a, key, True), (n, period, name, "decode"))
            if name == "letters":
                same(T.vigenere(enc, k, decode=True), host(a), (n, period, "round trip"))


@pytest.mark.parametrize("shift", VIG_SHIFTS)
def test_vigenere_every_shift(dev, shift):
    """One shift for the whole text: each value of the list, INT_MAX and
    INT_MIN among them, on every byte value, in both directions."""
    a = (np.arange(257) % 256).astype(np.uint8)
    key = np.array([shift], dtype=np.int64)
    k = torch.tensor([shift], dtype=torch.int32)
    x = view_at(a, 1, dev)
    same(T.vigenere(x, k), vig_oracle(a, key, False), (shift, "encode"))
    same(T.vigenere(x, k, decode=True), vig_oracle(a, key, True), (shift, "decode"))


def test_vigenere_arguments():
    x = torch.full((10,), 97, dtype=torch.uint8)
    with pytest.raises(ValueError):
        T.vigenere(x, torch.empty(0, dtype=torch.int32))
    with pytest.raises(ValueError):
        T.vigenere(x[:0], torch.empty(0, dtype=torch.int32))
    assert T.vigenere(x[:0], torch.tensor([3])).shape == (0,)
