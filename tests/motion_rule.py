"""The frame-to-frame motion rule of include/canny_hip.h in numpy and plain Python ints: the judge of
canny_hip_estimate_motion (plain C++) and of the kernels of csrc/canny_motion.hip.  Every product here is a Python int, so no
width bound is assumed: the bounds the header states are what the C++ and the kernels have to keep."""
import numpy as np

TRANSLATION, SIMILARITY, AFFINE = 0, 1, 2
SAMPLE = (1, 2, 3)
WORDS = 16
MAX_HYPOTHESES = 4096
MASK = 0xFFFFFFFF
A_LIMIT = 1 << 24


def correspondences(qc, n_q, tc, n_t, matches):
    """(int64 [m, 4]: x, y, x', y'; int64 [m]: the query slots) of one pair, in ascending slot order.  qc, tc: [stride, 4]
    records, matches [stride_q, 4] (j, d1, d2, flags); the counts are clamped to the strides."""
    qc, tc, matches = np.asarray(qc, np.int64).reshape(-1, 4), np.asarray(tc, np.int64).reshape(-1, 4), \
        np.asarray(matches, np.int64).reshape(-1, 4)
    n_q, n_t = min(max(int(n_q), 0), len(qc)), min(max(int(n_t), 0), len(tc))
    out, slots = [], []
    for i in range(n_q):
        j, flags = int(matches[i, 0]), int(matches[i, 3])
        if not (flags & 8) or j < 0 or j >= n_t:
            continue
        c = (int(qc[i, 0]), int(qc[i, 1]), int(tc[j, 0]), int(tc[j, 1]))
        if all(0 <= v <= 65535 for v in c):
            out.append(c)
            slots.append(i)
    return np.array(out, np.int64).reshape(-1, 4), np.array(slots, np.int64), n_q


def sample(h, seed, m, k):
    """The first k sample indices of hypothesis h among m correspondences (m >= k)."""
    s = [(int(seed) + 0x9E3779B9 * (h + 1)) & MASK]

    def draw(n):
        s[0] = (s[0] * 1664525 + 1013904223) & MASK
        return (s[0] >> 16) % n

    i1 = draw(m)
    if k == 1:
        return [i1]
    i2 = draw(m - 1)
    i2 += i2 >= i1
    if k == 2:
        return [i1, i2]
    i3 = draw(m - 2)
    i3 += i3 >= min(i1, i2)
    i3 += i3 >= max(i1, i2)
    return [i1, i2, i3]


def hypothesis(c, idx, model):
    """(D, M11, M12, M21, M22) in Python ints from the sampled correspondences."""
    x1, y1, u1, v1 = (int(v) for v in c[idx[0]])
    if model == TRANSLATION:
        return 1, 1, 0, 0, 1
    x2, y2, u2, v2 = (int(v) for v in c[idx[1]])
    dx, dy, du, dv = x2 - x1, y2 - y1, u2 - u1, v2 - v1
    if model == SIMILARITY:
        D = dx * dx + dy * dy
        A = dx * du + dy * dv
        B = dx * dv - dy * du
        return D, A, -B, B, A
    x3, y3, u3, v3 = (int(v) for v in c[idx[2]])
    fx, fy, fu, fv = x3 - x1, y3 - y1, u3 - u1, v3 - v1
    D = dx * fy - dy * fx
    return D, du * fy - fu * dy, fu * dx - du * fx, dv * fy - fv * dy, fv * dx - dv * fx


def inliers_of(c, q1, hyp, thr_q4):
    """bool [m]: the inlier test of every correspondence, in Python ints (object arrays)."""
    D, m11, m12, m21, m22 = hyp
    o = c.astype(object)
    dx, dy = o[:, 0] - int(q1[0]), o[:, 1] - int(q1[1])
    du, dv = o[:, 2] - int(q1[2]), o[:, 3] - int(q1[3])
    rx = D * du - (m11 * dx + m12 * dy)
    ry = D * dv - (m21 * dx + m22 * dy)
    lhs = 256 * (rx * rx + ry * ry)
    return np.array(lhs <= thr_q4 * thr_q4 * D * D, bool)


def refit(c, model):
    """(ok, [a11, a12, tx, a21, a22, ty, sum, max]) over the inliers c (int64 [n, 4], n >= 1)."""
    n = len(c)
    o = c.astype(object)
    x, y, u, v = o[:, 0], o[:, 1], o[:, 2], o[:, 3]
    S = lambda a: int(a.sum())
    sx, sy, su, sv = S(x), S(y), S(u), S(v)
    C = lambda a, b, sa, sb: n * S(a * b) - sa * sb
    cxx, cxy, cyy = C(x, x, sx, sx), C(x, y, sx, sy), C(y, y, sy, sy)
    cxu, cxv, cyu, cyv = C(x, u, sx, su), C(x, v, sx, sv), C(y, u, sy, su), C(y, v, sy, sv)
    if model == TRANSLATION:
        a11, a12, a21, a22 = 65536, 0, 0, 65536
    elif model == SIMILARITY:
        dn = cxx + cyy
        if dn <= 0:
            return False, [0] * 8
        a11 = a22 = 65536 * (cxu + cyv) // dn
        a21 = 65536 * (cxv - cyu) // dn
        a12 = -a21
    else:
        det = cxx * cyy - cxy * cxy
        if det <= 0:
            return False, [0] * 8
        a11 = 65536 * (cxu * cyy - cyu * cxy) // det
        a12 = 65536 * (cyu * cxx - cxu * cxy) // det
        a21 = 65536 * (cxv * cyy - cyv * cxy) // det
        a22 = 65536 * (cyv * cxx - cxv * cxy) // det
    if max(abs(a11), abs(a12), abs(a21), abs(a22)) > A_LIMIT:
        return False, [0] * 8
    tx = (65536 * su - a11 * sx - a12 * sy) // n
    ty = (65536 * sv - a21 * sx - a22 * sy) // n
    total = worst = 0
    for xi, yi, ui, vi in c.tolist():
        gx = (65536 * ui - (a11 * xi + a12 * yi + tx)) >> 8
        gy = (65536 * vi - (a21 * xi + a22 * yi + ty)) >> 8
        gx, gy = min(max(gx, -A_LIMIT), A_LIMIT), min(max(gy, -A_LIMIT), A_LIMIT)
        e = gx * gx + gy * gy
        total += e
        worst = max(worst, e)
    return True, [a11, a12, tx, a21, a22, ty, total, worst]


def estimate(qc, n_q, tc, n_t, matches, model, thr_q4, hypotheses, seed):
    """One pair -> (int64 [16] record, int32 [clamped n_q] inlier flags: 1, 0, or -1 where the slot is no correspondence)."""
    c, slots, n_q = correspondences(qc, n_q, tc, n_t, matches)
    m, k = len(c), SAMPLE[model]
    rec = np.zeros(WORDS, np.int64)
    rec[1], rec[3], rec[12:15] = m, -1, -1
    flags = np.full(n_q, -1, np.int32)
    flags[slots] = 0
    best = None
    if m >= k:
        for h in range(hypotheses):
            idx = sample(h, seed, m, k)
            hyp = hypothesis(c, idx, model)
            if hyp[0] == 0:
                continue
            inl = inliers_of(c, c[idx[0]], hyp, thr_q4)
            count = int(inl.sum())
            if best is None or count > best[0]:
                best = (count, h, idx, hyp, inl)
    if best is None:
        return rec, flags
    count, h, idx, hyp, inl = best
    flags[slots[inl]] = 1
    ok, fit = refit(c[inl], model)
    rec[0], rec[2], rec[3] = 1 | (2 if ok else 0), count, h
    rec[4:12] = fit
    rec[12:12 + k] = slots[idx]
    rec[15] = hyp[0]
    return rec, flags


def estimate_pairs(q_corners, q_counts, t_corners, t_counts, pairs, matches, model, thr_q4, hypotheses, seed):
    """The batch form: corners [frames, stride, 4], matches [n_pairs, stride_q, 4] -> (int64 [n_pairs, 16], list of flags)."""
    recs, flags = [], []
    for p, (fq, ft) in enumerate(pairs):
        r, f = estimate(q_corners[fq], q_counts[fq], t_corners[ft], t_counts[ft], matches[p], model, thr_q4, hypotheses, seed)
        recs.append(r)
        flags.append(f)
    return np.array(recs, np.int64).reshape(-1, WORDS), flags


def apply_q16(rec, x, y):
    """The refit model of a record applied to a point, in pixels (floats: for reading results, not part of the rule)."""
    a11, a12, tx, a21, a22, ty = (int(v) for v in rec[4:10])
    return (a11 * x + a12 * y + tx) / 65536.0, (a21 * x + a22 * y + ty) / 65536.0


# ---- designed sets -----------------------------------------------------------------------------------------------------------
def designed(rng, n, motion, wrong, size=600):
    """n query points, their images under the exact integer motion (a11, a12, a21, a22, tx, ty), `wrong` of them replaced by
    random points.  Returns (qc [n, 4], tc [n, 4], matches [n, 4]) with a shuffled train order."""
    a11, a12, a21, a22, tx, ty = motion
    pts = set()
    while len(pts) < n:
        pts.add((int(rng.integers(0, size)), int(rng.integers(0, size))))
    q = np.array(sorted(pts), np.int64)[rng.permutation(n)]
    t = np.stack([a11 * q[:, 0] + a12 * q[:, 1] + tx, a21 * q[:, 0] + a22 * q[:, 1] + ty], 1)
    bad = rng.permutation(n)[:wrong]
    t[bad] = rng.integers(0, 3 * size, (wrong, 2))
    order = rng.permutation(n)
    qc, tc = np.zeros((n, 4), np.int64), np.zeros((n, 4), np.int64)
    qc[:, :2] = q
    tc[order, :2] = t
    qc[:, 3], tc[:, 3] = np.arange(n), np.arange(n)
    matches = np.zeros((n, 4), np.int32)
    matches[:, 0], matches[:, 3] = order, 15
    return qc, tc, matches


def from_correspondences(c):
    """Records and a match row whose correspondences are exactly the rows of c (x, y, x', y'), in order."""
    c = np.asarray(c, np.int64).reshape(-1, 4)
    n = len(c)
    qc, tc = np.zeros((n, 4), np.int64), np.zeros((n, 4), np.int64)
    qc[:, :2], tc[:, :2] = c[:, :2], c[:, 2:]
    matches = np.zeros((n, 4), np.int32)
    matches[:, 0], matches[:, 3] = np.arange(n), 15
    return qc, tc, matches


def with_gaps(rng, c, extra):
    """from_correspondences(c) with `extra` slots in between that are no correspondence: not accepted, a train index
    outside the count, or a coordinate outside [0, 65535]."""
    c = np.asarray(c, np.int64).reshape(-1, 4)
    n, total = len(c), len(c) + extra
    keep = np.sort(rng.permutation(total)[:n])
    qc, tc = np.zeros((total, 4), np.int64), np.zeros((total, 4), np.int64)
    matches = np.zeros((total, 4), np.int32)
    qc[:, :2], tc[:, :2] = rng.integers(0, 500, (total, 2)), rng.integers(0, 500, (total, 2))
    matches[:, 0], matches[:, 3] = np.arange(total), 15
    qc[keep, :2], tc[keep, :2] = c[:, :2], c[:, 2:]
    gaps = np.setdiff1d(np.arange(total), keep)
    for n_gap, i in enumerate(gaps.tolist()):
        kind = n_gap % 6
        if kind == 0:
            matches[i, 3] = 7                      # every test passed but "accepted"
        elif kind == 1:
            matches[i, 0] = total                  # j == the train count
        elif kind == 2:
            matches[i, 0] = -1
        elif kind == 3:
            qc[i, 0] = -1
        elif kind == 4:
            tc[i, 1] = 65536
        else:
            qc[i, 1] = 1 << 40
    return qc, tc, matches


def tie_set():
    """TRANSLATION: two shifts, (5, 0) and (0, 9), with four correspondences each and two strays: every hypothesis drawn
    from either group counts four, so the smallest valid h wins whichever group it drew from."""
    c = [(10 * i, 7 * i, 10 * i + 5, 7 * i) for i in range(4)] + [(300 + 9 * i, 11 * i, 300 + 9 * i, 11 * i + 9) for i in range(4)]
    c += [(50, 60, 400, 1), (70, 80, 2, 300)]
    return np.array(c, np.int64)


def threshold_set(model):
    """thr_q4 = 48 is 3 px.  TRANSLATION: the sample has shift (0, 0) wherever it is drawn among the first six; one
    correspondence is off by (3, 0): 256 * 9 <= 48^2, an inlier; one by (3, 1): 256 * 10 > 2304, not.  SIMILARITY: the model
    is scale 2 drawn from points at distance 5 (D = 25 != 1, M = 50 I): off by (3, 0) in the train frame is
    r = (75, 0), 256 * 5625 == 2304 * 625: an inlier on the equality; off by (3, 1) is not."""
    s = 1 if model == TRANSLATION else 2
    base = [(0, 0), (3, 4), (6, 8), (9, 12), (12, 16), (15, 20)]
    c = [(x, y, s * x, s * y) for x, y in base]
    c += [(40, 40, s * 40 + 3, s * 40), (60, 20, s * 60 + 3, s * 20 + 1)]
    return np.array(c, np.int64)
