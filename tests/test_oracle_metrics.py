"""Pins oracle/metrics.py, the CPU restatement the device J / F metric is checked against, to independent formulations: its disk
dilation to scipy.ndimage.binary_dilation with the same structure, seg2bmap to a per-pixel restatement of the DAVIS boundary rule."""
import numpy as np
import pytest
from scipy import ndimage

from oracle import metrics as om

SHAPES = [(1, 1), (1, 37), (41, 1), (23, 31), (64, 70)]


def _strict_disk(r):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return (x * x + y * y) < r * r


@pytest.mark.parametrize("r", [0, 1, 2, 3, 4, 5, 12, 33])
def test_dilate_matches_scipy(r):
    rng = np.random.RandomState(r)
    for H, W in SHAPES:
        b = rng.rand(H, W) < 0.03
        b[rng.randint(H), rng.randint(W)] = True
        np.testing.assert_array_equal(om._dilate(b, r), ndimage.binary_dilation(b, structure=om._disk(r)))
    # one pixel in the middle of a map that holds the whole disk: the dilation is the disk itself, rim included
    n = 2 * r + 3
    one = np.zeros((n, n), dtype=bool)
    one[r + 1, r + 1] = True
    d = om._dilate(one, r)
    np.testing.assert_array_equal(d[1:-1, 1:-1], om._disk(r))
    assert d.sum() == om._disk(r).sum()
    if r >= 1:                                   # sensitivity: the disk without its rim is told apart
        assert not np.array_equal(d, ndimage.binary_dilation(one, structure=_strict_disk(r)))


def _bmap_direct(seg, neighbours=((0, 1), (1, 0), (1, 1))):
    """A pixel is a boundary pixel when it differs from any of its east, south and south-east neighbours that exist."""
    seg = seg.astype(bool)
    H, W = seg.shape
    b = np.zeros_like(seg)
    for y in range(H):
        for x in range(W):
            b[y, x] = any(seg[y + dy, x + dx] != seg[y, x] for dy, dx in neighbours if 0 <= y + dy < H and 0 <= x + dx < W)
    return b


@pytest.mark.parametrize("shape", SHAPES + [(2, 2), (3, 1), (1, 3)])
def test_seg2bmap_matches_direct_rule(shape):
    rng = np.random.RandomState(shape[0] * 100 + shape[1])
    differs = False
    for density in (0.1, 0.5, 0.9):
        seg = rng.rand(*shape) < density
        want = _bmap_direct(seg)
        np.testing.assert_array_equal(om.seg2bmap(seg), want)
        # sensitivity: the rule with the south-west neighbour in place of the south-east one is told apart
        differs |= not np.array_equal(_bmap_direct(seg, ((0, 1), (1, 0), (1, -1))), want)
    if min(shape) > 1:
        assert differs
