"""Adversarial planes for the Gaussian kernels: pixels whose quotient sits on an integer.

The reference's Gaussian (src/utils.cpp:26-68) is a chain of separately rounded float operations -- product, add in
ascending tap order, one division by the summed weight -- followed by a truncating cast.  A one-ulp slip anywhere in
the chain changes an output pixel only where the quotient q lies within one ulp of an integer: truncation hides every
other error.  On a random image a handful of pixels per frame are that close; on a flat neighbourhood of level g the
true quotient is exactly g and the float quotient is g or g minus one ulp, so every pixel of a flat region is such a
pixel.  The planes built here are piecewise constant:

* ``flat_batch(h, w)``: 256 frames, frame g filled with level g.  (24, 24) has every combination of left / right /
  top / bottom truncation for half-windows up to 8 with both borders independent; in (7, 40) every row renormalises,
  in (40, 7) every column.
* ``mosaic(h, w, frame=f)``: square cells of 23 x 23 pixels, each of one level drawn from a fixed permutation of
  0..255, the grid origin shifted per frame.  23 is odd and coprime to 4 and to every strip width of the marching
  kernels, so cell edges fall on every pixel-in-lane position and drift against the strip seams (some seams cut a
  cell's flat middle, others run next to a cell edge); for half-windows up to 8 every cell keeps a flat core of
  7 x 7 pixels.

``model`` is the reference's two passes in float32, vectorised, returning the plane before truncation; with
``mutant`` it makes one of four one-ulp mistakes instead.  ``critical`` marks the pixels that can reveal such a
mistake.  Everything here is plain numpy; tests/test_gaussian_planes.py checks the model against the oracle and
measures how sensitive the planes are, tests/test_gpu_gaussian_planes.py runs the kernels over them.
"""
from __future__ import annotations

import functools

import numpy as np

FLAT_SHAPES = ((24, 24), (7, 40), (40, 7))
MOSAIC_SHAPE = (300, 964)
MOSAIC_FRAMES = 4
CELL = 23
# half-windows 1..8: every instantiation of the marching kernels
HALF_WINDOW_SIGMAS = (0.3, 0.5, 1.0, 1.2, 1.4, 2.0, 2.3, 2.6)
# window 13 whose ascending weight sum, 1 - 5 * 2^-24, is not in the one-instruction division table
TABLE_MISS_SIGMA = 1.9362
MUTANTS = ("weights_descending", "fma", "pairs", "reciprocal")


def flat_batch(h: int, w: int) -> np.ndarray:
    """uint8 [256, h, w]: frame g is filled with level g."""
    return np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None], (256, h, w)))


@functools.lru_cache(maxsize=1)
def _perm() -> np.ndarray:
    return np.random.default_rng(1234).permutation(256).astype(np.uint8)


def mosaic(h: int, w: int, cell: int = CELL, *, frame: int) -> np.ndarray:
    """uint8 [h, w] of square cells of constant level.  The grid origin moves by ((5 frame) mod cell) rows and
    ((7 frame) mod cell) columns; the cell at (cy, cx) holds perm[(cy ncx + cx + 61 frame) mod 256]."""
    ncx = (w + cell) // cell + 1
    cy = (np.arange(h) + (5 * frame) % cell) // cell
    cx = (np.arange(w) + (7 * frame) % cell) // cell
    return _perm()[(cy[:, None] * ncx + cx[None, :] + 61 * frame) % 256]


def mosaics() -> np.ndarray:
    """The four mosaic frames, uint8 [4, 300, 964]."""
    return np.stack([mosaic(*MOSAIC_SHAPE, frame=f) for f in range(MOSAIC_FRAMES)])


def designed() -> dict:
    """Every designed batch by name: "flat24x24", "flat7x40", "flat40x7", "mosaic"."""
    out = {f"flat{h}x{w}": flat_batch(h, w) for h, w in FLAT_SHAPES}
    out["mosaic"] = mosaics()
    return out


def _pass(x: np.ndarray, taps: np.ndarray, mutant) -> np.ndarray:
    """One pass along the last axis: float32 [..., L] -> float32 quotients.  A tap contributes to the sum and to the
    weight where its pixel is inside the row, as in the reference."""
    f32 = np.float32
    taps = np.asarray(taps, f32)
    C = len(taps) // 2
    L = x.shape[-1]

    def span(k):  # output positions whose neighbour at offset k exists
        return max(0, -k), min(L, L - k)

    wsum = np.zeros(L, f32)
    order = range(C, -C - 1, -1) if mutant == "weights_descending" else range(-C, C + 1)
    for k in order:
        lo, hi = span(k)
        if lo < hi:
            wsum[lo:hi] += taps[C + k]

    if mutant == "fma":
        # fma(x, tap, acc): the exact product plus acc, rounded once (the product of a u8 or a float32 and a float32
        # is exact in float64)
        acc = np.zeros(x.shape, f32)
        for k in range(-C, C + 1):
            lo, hi = span(k)
            if lo < hi:
                exact = x[..., lo + k:hi + k].astype(np.float64) * np.float64(taps[C + k]) + acc[..., lo:hi]
                acc[..., lo:hi] = exact.astype(f32)
    elif mutant == "pairs":
        # (p[-k] + p[k]) * tap from the outermost pair inwards, the centre last; a lone neighbour at a border is
        # multiplied by itself
        acc = np.zeros(x.shape, f32)
        pos = np.arange(L)
        for k in range(C, 0, -1):
            left = np.zeros(x.shape, f32)
            right = np.zeros(x.shape, f32)
            lo, hi = span(-k)
            if lo < hi:
                left[..., lo:hi] = x[..., lo - k:hi - k]
            lo, hi = span(k)
            if lo < hi:
                right[..., lo:hi] = x[..., lo + k:hi + k]
            some = (pos - k >= 0) | (pos + k < L)
            term = (left + right) * taps[C + k]
            acc = np.where(some, acc + term, acc)
        acc = acc + x * taps[C]
    else:
        acc = np.zeros(x.shape, f32)
        for k in range(-C, C + 1):
            lo, hi = span(k)
            if lo < hi:
                acc[..., lo:hi] += x[..., lo + k:hi + k] * taps[C + k]

    if mutant == "reciprocal":
        return acc * (f32(1) / wsum)  # a * RN(1/b), without the two fma corrections
    return acc / wsum


def model(img, sigma_taps, mutant=None) -> np.ndarray:
    """The reference's Gaussian in float32: uint8 [..., H, W] and the taps (oracle.gaussian_kernel(sigma)) -> the
    float32 plane before the truncating cast.  mutant: None or one of MUTANTS, applied to both passes --
    "weights_descending": the weight summed in descending tap order; "fma": product and add fused; "pairs": symmetric
    taps paired, centre last; "reciprocal": a * RN(1/b) in place of the division."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(mutant)
    x = np.asarray(img)
    if x.dtype != np.uint8:
        raise ValueError("expected uint8 planes")
    rows = _pass(x.astype(np.float32), sigma_taps, mutant)
    cols = _pass(np.ascontiguousarray(np.swapaxes(rows, -1, -2)), sigma_taps, mutant)
    return np.ascontiguousarray(np.swapaxes(cols, -1, -2))


def critical(q) -> np.ndarray:
    """Pixels whose quotient is an integer or one ulp below one: only there can a one-ulp error change the output."""
    q = np.asarray(q, np.float32)
    up = np.nextafter(q, np.float32(np.inf))
    return (q == np.trunc(q)) | (up == np.trunc(up))


def border_distance(shape) -> np.ndarray:
    """int [H, W]: each pixel's distance to the nearest frame border (0 on the border itself)."""
    h, w = shape
    r, c = np.arange(h), np.arange(w)
    return np.minimum(np.minimum(r, h - 1 - r)[:, None], np.minimum(c, w - 1 - c)[None, :])
