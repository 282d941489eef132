"""The corner-descriptor and Hamming-matching rule of include/canny_hip.h, restated in numpy and plain
Python ints.  No device, no library: what the host functions and the kernels are compared with, word for word."""
import numpy as np

DESC_BITS, DESC_WORDS, DESC_RADIUS, DESC_ROTATIONS = 256, 4, 15, 32
DESC_STEERED, MATCH_CROSS_CHECK = 1, 1
NO_DISTANCE = 257
SEED = 0x43414E59
COS_Q14 = (16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0)


# ---- the pattern -----------------------------------------------------------------------------------------------------------
def cos_q14(k: int) -> int:
    """cos(2 pi k / 32) in Q14 from the nine constants, by symmetry."""
    k %= 32
    if k > 16:
        k = 32 - k
    return COS_Q14[k] if k <= 8 else -COS_Q14[16 - k]


def sin_q14(k: int) -> int:
    return cos_q14(k - 8)


def rd(v: int) -> int:
    return (v + 8192) >> 14   # floor((v + 8192) / 16384), also below zero


def rot(k: int, x: int, y: int):
    c, s = cos_q14(k), sin_q14(k)
    return rd(x * c - y * s), rd(x * s + y * c)


def base_tests():
    """(the 256 tests (ax, ay, bx, by) of rotation 0, the number of attempts the generator needed)."""
    s = SEED
    tests, seen, attempts = [], set(), 0

    def draw():
        nonlocal s
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        return (s >> 16) % 27 - 13

    while len(tests) < DESC_BITS:
        attempts += 1
        ax, ay, bx, by = draw(), draw(), draw(), draw()
        if ax * ax + ay * ay > 169 or bx * bx + by * by > 169:
            continue
        if abs(ax - bx) + abs(ay - by) < 4:
            continue
        if (ax, ay, bx, by) in seen or (bx, by, ax, ay) in seen:
            continue
        seen.add((ax, ay, bx, by))
        tests.append((ax, ay, bx, by))
    return tests, attempts


_PATTERN = None


def pattern():
    """int8 [32, 256, 4]: (ax, ay, bx, by) of every test in every rotation.  Read-only."""
    global _PATTERN
    if _PATTERN is None:
        tests, _ = base_tests()
        out = np.zeros((DESC_ROTATIONS, DESC_BITS, 4), np.int8)
        for k in range(DESC_ROTATIONS):
            for t, (ax, ay, bx, by) in enumerate(tests):
                out[k, t] = (*rot(k, ax, ay), *rot(k, bx, by))
        out.setflags(write=False)
        _PATTERN = out
    return _PATTERN


_DISC = None


def disc():
    """(dy, dx) int64 arrays of the 709 offsets with dx^2 + dy^2 <= 225."""
    global _DISC
    if _DISC is None:
        dy, dx = np.mgrid[-DESC_RADIUS:DESC_RADIUS + 1, -DESC_RADIUS:DESC_RADIUS + 1]
        keep = dx * dx + dy * dy <= DESC_RADIUS * DESC_RADIUS
        _DISC = (dy[keep].astype(np.int64), dx[keep].astype(np.int64))
        assert len(_DISC[0]) == 709
    return _DISC


# ---- descriptors -----------------------------------------------------------------------------------------------------------
def orientation_of(m10: int, m01: int) -> int:
    """The smallest k that maximises m10 * C_k + m01 * S_k (Python ints)."""
    scores = [int(m10) * cos_q14(k) + int(m01) * sin_q14(k) for k in range(DESC_ROTATIONS)]
    return scores.index(max(scores))


def describe_scalar(P, x: int, y: int, steered: bool):
    """(four words, meta) of one record, in plain Python ints."""
    P = np.asarray(P)
    h, w = P.shape
    if not (0 <= x < w and 0 <= y < h):
        return [0, 0, 0, 0], -1

    def at(yy, xx):
        return int(P[min(max(yy, 0), h - 1), min(max(xx, 0), w - 1)])

    k = 0
    if steered:
        dy, dx = disc()
        m10 = sum(int(u) * at(y + int(v), x + int(u)) for v, u in zip(dy, dx))
        m01 = sum(int(v) * at(y + int(v), x + int(u)) for v, u in zip(dy, dx))
        k = orientation_of(m10, m01)
    words = [0, 0, 0, 0]
    for t, (ax, ay, bx, by) in enumerate(pattern()[k].tolist()):
        if at(y + ay, x + ax) < at(y + by, x + bx):
            words[t // 64] |= 1 << (t % 64)
    r = DESC_RADIUS
    border = int(x - r < 0 or y - r < 0 or x + r > w - 1 or y + r > h - 1)
    return words, k + 256 * border


def describe(P, xy, steered: bool):
    """(uint64 [n, 4], int32 [n]) of the records at xy (int [n, 2]: x, y) on plane P, vectorised over the records."""
    P = np.asarray(P).astype(np.int64)
    h, w = P.shape
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    n = len(xy)
    x, y = xy[:, 0], xy[:, 1]
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    xc, yc = np.where(inside, x, 0), np.where(inside, y, 0)
    k = np.zeros(n, np.int64)
    if steered and n:
        dy, dx = disc()
        v = P[np.clip(yc[:, None] + dy, 0, h - 1), np.clip(xc[:, None] + dx, 0, w - 1)]
        m10, m01 = (v * dx).sum(1), (v * dy).sum(1)
        c = np.array([cos_q14(i) for i in range(DESC_ROTATIONS)], np.int64)
        s = np.array([sin_q14(i) for i in range(DESC_ROTATIONS)], np.int64)
        k = np.argmax(m10[:, None] * c + m01[:, None] * s, axis=1)   # the first maximum
    pat = pattern().astype(np.int64)[k]                                  # [n, 256, 4]
    a = P[np.clip(yc[:, None] + pat[:, :, 1], 0, h - 1), np.clip(xc[:, None] + pat[:, :, 0], 0, w - 1)]
    b = P[np.clip(yc[:, None] + pat[:, :, 3], 0, h - 1), np.clip(xc[:, None] + pat[:, :, 2], 0, w - 1)]
    bits = (a < b).reshape(n, DESC_WORDS, 64).astype(np.uint64)
    words = (bits << np.arange(64, dtype=np.uint64)).sum(2, dtype=np.uint64)
    r = DESC_RADIUS
    border = (xc - r < 0) | (yc - r < 0) | (xc + r > w - 1) | (yc + r > h - 1)
    meta = (k + 256 * border).astype(np.int32)
    words[~inside] = 0
    meta[~inside] = -1
    return words, meta


# ---- matching --------------------------------------------------------------------------------------------------------------
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def distances(q, t):
    """int64 [nq, nt]: the Hamming distances of uint64 [nq, 4] against uint64 [nt, 4]."""
    q = np.ascontiguousarray(q, np.uint64).reshape(-1, DESC_WORDS)
    t = np.ascontiguousarray(t, np.uint64).reshape(-1, DESC_WORDS)
    x = q[:, None, :] ^ t[None, :, :]
    return _POP8[np.ascontiguousarray(x).view(np.uint8)].reshape(len(q), len(t), -1).sum(2)


def match(q, t, max_distance=64, ratio_q8=205, options=MATCH_CROSS_CHECK):
    """(int32 [nq, 4]: j, d1, d2, flags; the number accepted) of one pair of descriptor sets."""
    q = np.ascontiguousarray(q, np.uint64).reshape(-1, DESC_WORDS)
    t = np.ascontiguousarray(t, np.uint64).reshape(-1, DESC_WORDS)
    nq, nt = len(q), len(t)
    out = np.zeros((nq, 4), np.int32)
    if nq == 0:
        return out, 0
    if nt == 0:
        j = np.full(nq, -1, np.int64)
        d1 = d2 = np.full(nq, NO_DISTANCE, np.int64)
        mutual = np.zeros(nq, bool)
    else:
        D = distances(q, t)
        j = np.argmin(D, axis=1)                      # the first minimum: the smallest (d, j)
        rows = np.arange(nq)
        d1 = D[rows, j]
        rest = D.copy()
        rest[rows, j] = NO_DISTANCE
        d2 = rest.min(axis=1)
        back = np.argmin(D, axis=0)                   # per train j the smallest (d, i)
        mutual = back[j] == rows
    f0 = d1 <= max_distance
    f1 = (d1 * 256 < ratio_q8 * d2) if ratio_q8 else np.ones(nq, bool)
    acc = f0 & f1 & (mutual if options & MATCH_CROSS_CHECK else True)
    out[:, 0], out[:, 1], out[:, 2] = j, d1, d2
    out[:, 3] = f0 * 1 + f1 * 2 + mutual * 4 + acc * 8
    return out, int(acc.sum())


def match_scalar(q, t, max_distance, ratio_q8, options):
    """The same in plain Python ints, one query at a time."""
    q = [[int(v) for v in row] for row in np.asarray(q, np.uint64).reshape(-1, DESC_WORDS)]
    t = [[int(v) for v in row] for row in np.asarray(t, np.uint64).reshape(-1, DESC_WORDS)]

    def dist(a, b):
        return sum(bin(u ^ v).count("1") for u, v in zip(a, b))

    out = []
    for i, a in enumerate(q):
        ds = [dist(a, b) for b in t]
        if not ds:
            j, d1, d2, mutual = -1, NO_DISTANCE, NO_DISTANCE, False
        else:
            d1 = min(ds)
            j = ds.index(d1)
            d2 = min([d for jj, d in enumerate(ds) if jj != j], default=NO_DISTANCE)
            col = [dist(b, t[j]) for b in q]
            mutual = col.index(min(col)) == i
        f0 = d1 <= max_distance
        f1 = ratio_q8 == 0 or d1 * 256 < ratio_q8 * d2
        acc = f0 and f1 and (mutual or not options & MATCH_CROSS_CHECK)
        out.append([j, d1, d2, f0 * 1 + f1 * 2 + mutual * 4 + acc * 8])
    return np.array(out, np.int32).reshape(-1, 4), sum(r[3] >> 3 for r in out)


# ---- designed sets -----------------------------------------------------------------------------------------------------
def random_set(rng, n, spread=24):
    """n descriptors around a few centres, so that distances are small enough for the tests to bite."""
    centres = rng.integers(0, 1 << 63, (max(n // 3, 1), 4)).astype(np.uint64)
    out = centres[rng.integers(0, len(centres), n)].copy()
    for _ in range(spread):
        bit = rng.integers(0, 256, n)
        out[np.arange(n), bit // 64] ^= (np.uint64(1) << (bit % 64).astype(np.uint64))
    return out


def duplicated_sets(rng):
    """Query and train sets with duplicated descriptors: ties go to the smaller index, d2 == d1."""
    base = random_set(rng, 20, 6)
    t = np.concatenate([base, base[::-1], base[:7]])
    q = np.concatenate([base[5:15], base[5:15], random_set(rng, 6, 6)])
    return q, t
