"""The Hough line rule of include/canny_hip.h restated in numpy: geometry, tables, accumulator,
five-way peaks, (votes descending, base ascending) order.  Shared by tests/test_hough_rule.py (host-only entry points)
and tests/test_gpu_hough_lines.py (every accumulator cell and every returned line, bit for bit).  Nothing here calls the
library: the GPU tests pass the library's own tables to `accumulate` so that no libm difference can enter."""
import numpy as np

F32 = np.float32
PI_F32 = F32(np.pi)


def geometry(height, width, rho, theta, min_theta=0.0, max_theta=np.pi):
    rho, theta, lo, hi = (float(F32(v)) for v in (rho, theta, min_theta, max_theta))
    numangle = int(np.floor((hi - lo) / theta)) + 1
    if numangle > 1 and abs(np.pi - (numangle - 1) * theta) < theta / 2:
        numangle -= 1
    numrho = int(np.rint((2.0 * (width + height) + 1.0) / rho))  # np.rint: half to even
    return numangle, numrho


def tables(rho, theta, min_theta, numangle):
    irho = F32(1.0) / F32(rho)
    ang, theta = F32(min_theta), F32(theta)
    tc, ts = np.empty(numangle, F32), np.empty(numangle, F32)
    for n in range(numangle):
        tc[n] = F32(np.cos(np.float64(ang)) * np.float64(irho))
        ts[n] = F32(np.sin(np.float64(ang)) * np.float64(irho))
        ang = F32(ang + theta)
    return tc, ts


def accumulate(points, width, numrho, tab_cos, tab_sin):
    """points: flat indices y * width + x of the set pixels -> int32 accumulator (numangle + 2, numrho + 2)."""
    p = np.asarray(points, np.int64)
    y, x = (p // width).astype(F32), (p % width).astype(F32)
    numangle = len(tab_cos)
    acc = np.zeros((numangle + 2, numrho + 2), np.int32)
    for n in range(numangle):
        v = (x * F32(tab_cos[n])).astype(F32) + (y * F32(tab_sin[n])).astype(F32)  # three float32 roundings
        r = np.rint(v.astype(F32)).astype(np.int64) + (numrho - 1) // 2
        assert r.size == 0 or (r.min() >= 0 and r.max() < numrho)
        acc[n + 1, 1:numrho + 1] = np.bincount(r, minlength=numrho)
    return acc


def peaks(acc, threshold):
    """All peaks of one accumulator in output order: (bases uint32, votes int32)."""
    a = acc.astype(np.int64)
    c = a[1:-1, 1:-1]
    mask = (c > threshold) & (c > a[1:-1, :-2]) & (c >= a[1:-1, 2:]) & (c > a[:-2, 1:-1]) & (c >= a[2:, 1:-1])
    n, r = np.nonzero(mask)
    base = (n + 1) * acc.shape[1] + r + 1
    votes = c[n, r]
    order = np.lexsort((base, -votes))
    return base[order].astype(np.uint32), votes[order].astype(np.int32)


def line_of(base, numrho, rho, theta, min_theta=0.0):
    """(line_rho, line_theta) float32 arrays of accumulator cells, each operation rounded to float32."""
    base = np.asarray(base, np.int64)
    n, r = base // (numrho + 2) - 1, base % (numrho + 2) - 1
    centre = F32(F32(numrho - 1) * F32(0.5))
    line_rho = ((r.astype(F32) - centre).astype(F32) * F32(rho)).astype(F32)
    line_theta = (F32(min_theta) + (n.astype(F32) * F32(theta)).astype(F32)).astype(F32)
    return line_rho, line_theta


def lines(acc, threshold, lines_max, rho, theta, min_theta=0.0):
    """What one frame returns: (lines float32 [k, 2], votes int32 [k], bases uint32 [k], true count)."""
    base, votes = peaks(acc, threshold)
    k = min(lines_max, base.size)
    lr, lt = line_of(base[:k], acc.shape[1] - 2, rho, theta, min_theta)
    return np.stack([lr, lt], axis=1).astype(F32).reshape(k, 2), votes[:k], base[:k], int(base.size)
