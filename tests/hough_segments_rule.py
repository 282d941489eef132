"""The Hough segment rule of include/canny_hip.h restated in numpy: for every line of a list the
full-plane vote, S = W & (vote == r), a reduction along the minor axis and a run split.  There is no search window here:
this is the definition.  Shared by tests/test_hough_segments_rule.py (the host-only entry point) and
tests/test_gpu_hough_segments.py.  Nothing here calls the library; the tests pass the library's own tables in, so that no
libm difference can enter."""
import numpy as np

F32 = np.float32
SEGMENT_INTS = 6


def vote_plane(height, width, c, s, numrho):
    """vote(x, y) of every pixel for one angle: three float32 roundings, then round half to even."""
    x = np.arange(width, dtype=F32)[None, :]
    y = np.arange(height, dtype=F32)[:, None]
    v = ((x * F32(c)).astype(F32) + (y * F32(s)).astype(F32)).astype(F32)
    return np.rint(v).astype(np.int64) + (numrho - 1) // 2


def segments(mask, bases, numrho, tab_cos, tab_sin, min_length=0, max_gap=0, exclusive=0):
    """All records of one frame in output order: int32 [total, 6] rows x0, y0, x1, y1, k, support."""
    work = np.array(mask, dtype=bool)  # W, a private copy
    height, width = work.shape
    numangle = len(tab_cos)
    planes = {}
    out = []
    for k, base in enumerate(np.asarray(bases, np.int64)):
        n, r = int(base) // (numrho + 2) - 1, int(base) % (numrho + 2) - 1
        if not (0 <= n < numangle and 0 <= r < numrho):
            continue
        if n not in planes:
            planes[n] = vote_plane(height, width, tab_cos[n], tab_sin[n], numrho)
        support = work & (planes[n] == r)
        major_x = bool(np.abs(F32(tab_sin[n])) >= np.abs(F32(tab_cos[n])))
        s_tm = support.T if major_x else support            # [t, m]
        cnt = s_tm.sum(axis=1)
        lo = s_tm.argmax(axis=1)                            # the first (smallest) set m of each on position
        on = np.flatnonzero(cnt)
        if on.size == 0:
            continue
        cuts = np.flatnonzero(np.diff(on) - 1 > max_gap)
        firsts = np.concatenate([[0], cuts + 1])
        lasts = np.concatenate([cuts, [on.size - 1]])
        keep = np.zeros(s_tm.shape[0], bool)
        for a, b in zip(on[firsts], on[lasts]):
            if b - a < min_length:
                continue
            p0, p1 = (a, lo[a]), (b, lo[b])
            if not major_x:
                p0, p1 = p0[::-1], p1[::-1]
            out.append((p0[0], p0[1], p1[0], p1[1], k, int(cnt[a:b + 1].sum())))
            keep[a:b + 1] = True
        if exclusive:
            claimed = s_tm & keep[:, None]
            work &= ~(claimed.T if major_x else claimed)
    return np.array(out, np.int32).reshape(len(out), SEGMENT_INTS)


# ---- masks both test files use -----------------------------------------------------------------------------------------
MIN_LENGTH, MAX_GAP = 5, 3  # the parameters the drawn patterns are built around


def pattern(length, variant=0, min_length=MIN_LENGTH, max_gap=MAX_GAP):
    """On / off positions along a line of `length` pixels with one feature across positions 63 / 64 and another across
    1023 / 1024 (where they fit) -- the borders of a wave's chunk and of a 1024-lane workgroup pass:
      variant 0: a gap of exactly max_gap (bridged)      | a run with tb - ta = min_length (kept)
      variant 1: a gap of max_gap + 1 (splits)           | a run with tb - ta = min_length - 1 (dropped)
      variant 2, 3: the same with the borders swapped."""
    p = np.zeros(length, bool)

    def put(a, b):  # inclusive, clipped
        if a < length:
            p[a:min(b, length - 1) + 1] = True

    def gap_at(border, gap):  # the off positions end ON the border: the run in front of them is known only by its carry
        put(border - gap - 15, border - gap)
        put(border + 1, border + 9)

    def run_at(border, extent):  # positions a .. a + extent with border and border + 1 among them, alone
        a = border - extent // 2
        put(a, a + extent)

    borders = (63, 1023) if variant < 2 else (1023, 63)
    gap_at(borders[0], max_gap + (variant & 1))
    run_at(borders[1], min_length - (variant & 1))
    p[:2] = True                              # touching position 0
    p[length - 1] = True                      # a single pixel at the very end
    return p


def drawn(height, width):
    """Four horizontal and four vertical broken lines (pattern variants 0..3) and a diagonal one, which sits on the
    major-axis tie at theta = pi / 4."""
    m = np.zeros((height, width), bool)
    for j in range(4):
        m[(2 * j + 1) * height // 9, :] |= pattern(width, j)
        m[:, (2 * j + 1) * width // 9] |= pattern(height, j)
    i = np.flatnonzero(pattern(min(height, width)))
    m[i, i] = True
    return m


def mask_kinds(height, width, seed):
    """name -> mask: empty, all set, 1 % random, drawn broken lines."""
    rng = np.random.default_rng(seed)
    return {"empty": np.zeros((height, width), bool), "all": np.ones((height, width), bool),
            "random": rng.random((height, width)) < 0.01, "drawn": drawn(height, width)}


SHAPES = [(1, 1), (1, 70), (70, 1), (3, 5), (97, 161), (40, 1100), (1100, 40)]
RHOS = [0.5, 1.0, 2.5]
PI = float(np.pi)
# (theta, min_theta, max_theta): the two resolutions of the grid and a restricted range
ANGLES = [(PI / 180, 0.0, PI), (PI / 4, 0.0, PI), (PI / 180, PI / 4, 3 * PI / 4)]


def parameter_sets(height, width):
    """(min_length, max_gap) triples every case runs with: nothing bridged or dropped, the drawn patterns' own, one run."""
    return [(0, 0), (MIN_LENGTH, MAX_GAP), (0, max(height, width))]
