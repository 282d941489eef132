"""The contour rule of include/canny_hip.h restated in plain Python / numpy, for the tests.

Components, min_area filter and numbering are those of components_rule.components.  For each kept component the chain is
its outer border, followed as in Suzuki & Abe's border following restricted to outer borders, with 8-connectivity, from
the component's first pixel.  Directions are numbered clockwise on the displayed image, as (row, column) steps:
0 E (0,+1), 1 SE (+1,+1), 2 S (+1,0), 3 SW (+1,-1), 4 W (0,-1), 5 NW (-1,-1), 6 N (-1,0), 7 NE (-1,+1); pixels outside the
frame are unset.

  1. p0 = first.  Examine p0's neighbours clockwise after W: directions 5, 6, 7, 0, 1, 2, 3.  The first set one is q1, in
     direction d_last; if there is none the chain is [p0].
  2. cur = p0, s = (d_last - 1) & 7.  Repeat: examine cur's neighbours counter-clockwise in directions s, s - 1, ... (mod
     8, all eight); the first set one is nxt, in direction d.  If nxt == p0 and cur == q1, stop.  Otherwise append nxt,
     cur = nxt, s = (d + 3) & 7.
  3. The chain is p0 followed by the appended pixels, as indices r * width + c; p0 is not repeated at the end.

contours(mask, min_area) -> (stats int32 [K, 6], chains: list of K int32 arrays)
csr(maps, min_area)      -> (stats [total, 6], offsets u64 [N + 1], chain_offsets u64 [total + 1], points int32 [P],
                             point_offsets u64 [N + 1])

Nothing here is shared with the library: the walk reads a padded byte string pixel by pixel."""
import numpy as np

import components_rule

DY = (0, 1, 1, 1, 0, -1, -1, -1)
DX = (1, 1, 0, -1, -1, -1, 0, 1)


def chain(mask, first):
    """The chain of the component of `mask` (bool [H, W]) whose first pixel has index `first`."""
    h, w = mask.shape
    pitch = w + 2
    cells = np.pad(np.asarray(mask) != 0, 1).astype(np.uint8).tobytes()
    step = [DY[d] * pitch + DX[d] for d in range(8)]          # in the padded map
    index_step = [DY[d] * w + DX[d] for d in range(8)]        # in r * width + c
    p0 = int(first)
    at = (p0 // w + 1) * pitch + p0 % w + 1
    out = [p0]
    d_last = next((d for d in (5, 6, 7, 0, 1, 2, 3) if cells[at + step[d]]), None)
    if d_last is None:
        return np.array(out, np.int32)
    q1 = p0 + index_step[d_last]
    cur, s = p0, (d_last - 1) & 7
    while True:
        d = next(dd & 7 for dd in range(s, s - 8, -1) if cells[at + step[dd & 7]])
        nxt = cur + index_step[d]
        if nxt == p0 and cur == q1:
            break
        out.append(nxt)
        cur, at, s = nxt, at + step[d], (d + 3) & 7
    return np.array(out, np.int32)


def contours(mask, min_area=1):
    mask = np.asarray(mask) != 0
    _, stats = components_rule.components(mask, min_area)
    return stats, [chain(mask, rec[components_rule.FIRST]) for rec in stats]


def csr(maps, min_area=1):
    res = [contours(m, min_area) for m in maps]
    n = len(res)
    offsets, point_offsets = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum([s.shape[0] for s, _ in res], dtype=np.uint64)
    chains = [c for _, cs in res for c in cs]
    chain_offsets = np.zeros(len(chains) + 1, np.uint64)
    chain_offsets[1:] = np.cumsum([c.size for c in chains], dtype=np.uint64)
    point_offsets[1:] = np.cumsum([sum(c.size for c in cs) for _, cs in res], dtype=np.uint64)
    stats = np.concatenate([s for s, _ in res]) if n else np.zeros((0, 6), np.int32)
    points = np.concatenate(chains).astype(np.int32) if chains else np.zeros(0, np.int32)
    return stats, offsets, chain_offsets, points, point_offsets
