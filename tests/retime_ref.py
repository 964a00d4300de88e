"""The definition of the frame retimer (include/avse.h avse_retime_*) restated in numpy: integer
arithmetic for uint8 frames, float64 for float32 ones.

p / q = fps_in / fps_out, reduced.  Output frame j sits at input position j p / q: c = j p, i0 = c div q, r = c mod q,
a = A[i0], b = A[min(i0 + 1, n - 1)];
  float32:  float32((float64(q - r) a + float64(r) b) / float64(q)), and a's bits for r == 0;
  uint8:    (2 (a (q - r) + b r) + q) div (2 q): round half up.
After n >= 1 frames G(n) = floor((n - 1) q / p) + 1 outputs are final; flushed, all ceil(n q / p)."""
from fractions import Fraction

import numpy as np


def ratio(fps_in, fps_out):
    """(p, q) of fps_in / fps_out; the rates are ints, Fractions or (num, den) pairs."""
    f = lambda x: Fraction(*x) if isinstance(x, tuple) else Fraction(x)
    pq = f(fps_in) / f(fps_out)
    return pq.numerator, pq.denominator


def total(p, q, n, flushed):
    if n <= 0:
        return 0
    return -(-n * q // p) if flushed else (n - 1) * q // p + 1


def frames(A, p, q, flushed=True):
    """A [n, 128, 128] (uint8 or float32) -> the final output frames [total(p, q, n, flushed), 128, 128]."""
    A = np.asarray(A)
    n = A.shape[0]
    out = np.empty((total(p, q, n, flushed),) + A.shape[1:], A.dtype)
    for j in range(out.shape[0]):
        c = j * p
        i0, r = divmod(c, q)
        a, b = A[i0], A[min(i0 + 1, n - 1)]
        if r == 0:
            out[j] = a
        elif A.dtype == np.uint8:
            a, b = a.astype(np.int64), b.astype(np.int64)
            out[j] = (2 * (a * (q - r) + b * r) + q) // (2 * q)
        else:
            assert A.dtype == np.float32
            with np.errstate(all="ignore"):
                out[j] = ((np.float64(q - r) * a.astype(np.float64) + np.float64(r) * b.astype(np.float64))
                          / np.float64(q)).astype(np.float32)
    return out


def slices(A, p, q, F, flushed=True):
    """-> [S, 128, 128, F]: the complete slices of frames(A), frame innermost; the remainder is dropped."""
    y = frames(A, p, q, flushed)
    S = y.shape[0] // F
    return np.ascontiguousarray(y[:S * F].reshape((S, F) + y.shape[1:]).transpose(0, 2, 3, 1))


def retime(A, p, q, F, flushed=True):
    """-> (frames, slices)."""
    return frames(A, p, q, flushed), slices(A, p, q, F, flushed)
