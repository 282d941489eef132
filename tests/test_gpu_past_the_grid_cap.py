"""Every analysis-stage kernel that runs on a capped grid, pushed past its cap: some wave or thread
of each launch takes a SECOND item of its grid-stride loop, and the whole output of the call -- every frame, every CSR
offset -- is compared exactly with the stage's numpy rule.

How a case is built.  A batch cycles K = 7 distinct small frames (one empty, one dense), so the frame a wave meets on its
second trip differs from the one it met on the first: a result stored at "index minus stride", state carried over from
the previous item or an index that is right on the first trip only shows up as a difference.  The rule is computed once
per DISTINCT frame and the batch's expectation is assembled from it.  Every case first asserts, through
canny_hip_selftest_launch_plan, that each launch it is there for takes at least two trips and that its last trip is a
partial one, and that the stride of a trip is no multiple of the cycle (the single long frames behind dev_canny are noise
with flat bands and have no cycle).  Every output buffer is pre-filled with a sentinel and followed by guard words.  Where
the call takes a capacity, it runs once with room for everything and once with a capacity that ends inside the second
trip of the kernels the case is there for; the contour / polygon case cuts its point and vertex capacities there too.

Both sources run where the kernels are templated on them: packed bits through the *_bits forms, and the converged strong
plane behind dev_canny_* (reference: oracle.canny of each distinct frame, then the same rule)."""
import numpy as np
import pytest

import components_rule
import contours_rule
import edt_rule
import hough_circles_rule
import hough_rule
import oracle
import polygons_rule
from test_colour_rules import gray as gray_rule_of

pytestmark = pytest.mark.gpu

K = 7                                   # distinct frames of a cycle: prime
N_GUARD = 64
S32 = np.int32(0x5A5A5A5A)
S8 = np.uint8(0xA5)
S64 = np.uint64(0xEEEEEEEEEEEEEEEE)
M64 = np.int64(0x5A5A5A5A5A5A5A5A)
SIGMA, LO, HI = 1.0, 50, 150            # the canny route


# ---- the batches ----------------------------------------------------------------------------------------------------------
def _masks(h, w, seed, lattice=False):
    """K distinct h x w masks: [0] empty, [1] every pixel set, then Bernoulli maps of growing density; with `lattice`,
    [2..5] are the four stride-2 lattices of isolated pixels (the densest a map of components can be)."""
    rng = np.random.default_rng(seed)
    m = np.zeros((K, h, w), bool)
    m[1] = True
    for k in range(2, K):
        if lattice and k < 6:
            m[k, (k - 2) // 2::2, (k - 2) % 2::2] = True
        if not m[k].any():  # no lattice asked for, or none with this offset in a frame one pixel wide
            m[k] = rng.random((h, w)) < 0.12 * (k - 1)
    assert len({a.tobytes() for a in m}) == K and not m[0].any() and m[1].all()
    return m


def _images(h, w, seed):
    """K distinct h x w frames for the canny route and their maps by the oracle: [0] flat and [1] noise below the low
    threshold (empty maps), full-range noise after them (one edge pixel in five or so: as dense as this detector's maps
    get)."""
    rng = np.random.default_rng(seed)
    img = np.zeros((K, h, w), np.uint8)
    img[1] = rng.integers(0, 24, (h, w), dtype=np.uint8)
    for k in range(2, K):
        img[k] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    maps = np.stack([oracle.canny(f, SIGMA, LO, HI) for f in img])
    dens = (maps != 0).mean(axis=(1, 2))
    assert dens[0] == 0 and dens.max() > 0.1 and len({a.tobytes() for a in maps}) == K - 1, dens
    return img, maps != 0


def _cycle(n):
    return np.arange(n) % K


def _csr(idx, per):
    """Rows of per[k] for every frame of the batch, concatenated, and their offsets."""
    counts = np.array([len(p) for p in per], np.int64)
    off = np.zeros(idx.size + 1, np.uint64)
    off[1:] = np.cumsum(counts[idx])
    return np.concatenate([per[k] for k in idx]), off


def _plan(hip, kind, n=1, h=1, w=1, extra=0, trips=2, units_per_frame=None):
    """The launch of `kind` takes at least `trips` trips, the last one partial; the stride of a trip is no multiple of the
    cycle's units, so that the second item of a wave is not the same frame and row as its first."""
    p = hip.launch_plan(kind, n, h, w, extra)
    per_trip = p.grid * p.per_group
    assert p.trips >= trips and p.units % per_trip != 0, f"{kind}: {p}"
    if units_per_frame is not None:
        assert per_trip % (K * units_per_frame) != 0, f"{kind}: a trip covers whole cycles of {K} frames"
    return p


class _Dev:
    """Guarded, sentinel-filled device buffers of one case, and the device memory it needed."""

    def __init__(self, ctx):
        self.ctx, self.ptrs, self.bytes, self.peak = ctx, {}, 0, 0

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.ctx.malloc(max(a.nbytes, 16) + 16)
        self.ptrs[p] = a.nbytes
        self.bytes += a.nbytes
        self.peak = max(self.peak, self.bytes)
        self.ctx.h2d(p, a)
        return p

    def free(self, *ptrs):
        for p in ptrs:
            self.bytes -= self.ptrs.pop(p)
            self.ctx.free(p)

    def filled(self, count, fill):
        return self.put(np.full(int(count) + N_GUARD, fill))

    def get(self, ptr, count, dtype, fill, what, used=None):
        """The first `count` elements; everything from `used` (default count) on, guard included, must hold the sentinel."""
        out = np.empty(int(count) + N_GUARD, dtype)
        self.ctx.d2h(out, ptr)
        tail = out[int(count if used is None else used):]
        assert np.all(tail == fill), f"{what}: written past what fits"
        return out[:int(count if used is None else used)]

    def report(self, name):
        ws = sum(size for _, ptr, size, _ in self.ctx.selftest_workspaces() if ptr)
        print(f"[past-the-cap] {name}: buffers {self.peak / 2**20:.0f} MiB at their peak + workspaces {ws / 2**20:.0f} MiB")

    def close(self):
        self.free(*list(self.ptrs))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _source(dev, source, idx, h, w, seed, lattice=False):
    """(device pointer of the batch, masks of the K distinct frames) for source 'bits' or 'canny'."""
    if source == "bits":
        masks = _masks(h, w, seed, lattice)
        return dev.put(np.packbits(masks, axis=-1)[idx]), masks
    img, masks = _images(h, w, seed)
    return dev.put(img[idx]), masks


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), \
        f"{what}: {int((got != want).sum()) if got.shape == want.shape else 'shape'} differ"


# ---- edge point lists: row_grid of count and scatter, the frame scan -----------------------------------------------------
@pytest.mark.parametrize("source", ["bits", "canny"])
def test_point_lists_past_the_row_cap(hip, source):
    n, h, w = 61703, 17, 8
    p = _plan(hip, "points_rows", n, h, w, units_per_frame=h)
    _plan(hip, "scan_frames", n)
    idx = _cycle(n)
    with hip.Context(0) as ctx, _Dev(ctx) as dev:
        d_src, masks = _source(dev, source, idx, h, w, 11)
        want, w_off = _csr(idx, [np.flatnonzero(m).astype(np.uint32) for m in masks])   # the rule: np.flatnonzero
        total = want.size
        first_trip_ends = int(w_off[p.grid * p.per_group // h + 1])
        assert first_trip_ends < total
        for cap in (total, (first_trip_ends + total) // 2):
            d_pts, d_off = dev.filled(cap, np.uint32(S32)), dev.filled(n + 1, S64)
            if source == "bits":
                ctx.dev_points_from_bits(d_src, h, w, n, d_pts, cap, d_off)
            else:
                ctx.dev_canny_points(d_src, SIGMA, LO, HI, h, w, n, d_pts, cap, d_off)
            what = f"points {source} capacity {cap} of {total}"
            _same(dev.get(d_off, n + 1, np.uint64, S64, what), w_off, what + ": offsets")
            _same(dev.get(d_pts, cap, np.uint32, np.uint32(S32), what), want[:cap], what + ": points")
        dev.report(f"points {source}")


# ---- connected components -------------------------------------------------------------------------------------------------
def _components_case(hip, ctx, dev, source, n, h, w, seed, lattice, cap_of, name):
    idx = _cycle(n)
    d_src, masks = _source(dev, source, idx, h, w, seed, lattice)
    per = [components_rule.components(m, 1) for m in masks]
    w_labels = np.stack([l for l, _ in per])
    w_stats, w_off = _csr(idx, [s for _, s in per])
    total = w_stats.shape[0]
    npx = n * h * w
    for cap in (total, cap_of(w_off, total)):
        assert 0 < cap <= total
        d_labels, d_kept = dev.filled(npx, S32), dev.filled(npx, S8)
        d_stats, d_off = dev.filled(cap * 6, S32), dev.filled(n + 1, S64)
        if source == "bits":
            ctx.dev_components_bits(d_src, h, w, n, 1, d_labels, d_kept, d_stats, cap, d_off)
        else:
            ctx.dev_canny_components(d_src, SIGMA, LO, HI, h, w, n, 1, d_labels, d_kept, d_stats, cap, d_off)
        what = f"{name} {source} capacity {cap} of {total}"
        _same(dev.get(d_off, n + 1, np.uint64, S64, what), w_off, what + ": offsets")
        _same(dev.get(d_stats, cap * 6, np.int32, S32, what).reshape(cap, 6), w_stats[:cap], what + ": stats")
        got = dev.get(d_labels, npx, np.int32, S32, what).reshape(n, h, w)
        for k in range(K):  # frame by frame of the cycle: no batch-sized copy of the expectation
            assert np.all(got[k::K] == w_labels[k]), f"{what}: labels of the frames of kind {k} differ"
        got = dev.get(d_kept, npx, np.uint8, S8, what).reshape(n, h, w)
        for k in range(K):
            assert np.all(got[k::K] == np.where(w_labels[k] != 0, 255, 0)), f"{what}: kept_u8 of kind {k} differs"
        dev.free(d_labels, d_kept, d_stats, d_off)
    dev.report(f"{name} {source}")
    return total


@pytest.mark.parametrize("source", ["bits", "canny"])
def test_components_past_the_row_cap(hip, source):
    """cc_count and cc_number: more than 65 536 x 4 image rows."""
    n, h, w = 40013, 7, 8
    p = _plan(hip, "cc_rows", n, h, w, units_per_frame=h)
    _plan(hip, "scan_frames", n)
    first_trip_frames = p.grid * p.per_group // h + 1
    with hip.Context(0) as ctx, _Dev(ctx) as dev:
        _components_case(hip, ctx, dev, source, n, h, w, 21, False,
                         lambda off, total: (int(off[first_trip_frames]) + total) // 2, "components rows")


@pytest.mark.parametrize("source,w", [("bits", 1), ("canny", 2)])
def test_components_past_the_tile_cap(hip, source, w):
    """init, merge, flatten, area, relabel, write: more than 65 536 x 4 tiles.  At most 65 535 frames make a batch, so a frame
    needs five tiles: 257 rows, one pixel wide from bits (13.5 M pixels) and two behind the detector, which takes no
    narrower frame (26.9 M pixels, 103 MiB per int32 plane: above the 20 M the other cases keep to, as far as the tile
    kernels' strong-plane form can be had)."""
    n, h = 52433, 257
    p = _plan(hip, "cc_tiles", n, h, w, units_per_frame=5)
    _plan(hip, "cc_rows", n, h, w, units_per_frame=h)
    first_trip_frames = p.grid * p.per_group // 5 + 1
    with hip.Context(0) as ctx, _Dev(ctx) as dev:
        _components_case(hip, ctx, dev, source, n, h, w, 22, True,
                         lambda off, total: (int(off[first_trip_frames]) + total) // 2, "components tiles")


def test_component_records_past_the_fixup_cap(hip):
    """cc_fixup: more than 4 096 x 256 records, from stride-2 lattices of isolated pixels."""
    n, h, w = 7211, 32, 32
    with hip.Context(0) as ctx, _Dev(ctx) as dev:
        def cap_of(off, total):
            _plan(hip, "cc_fixup", extra=total)
            cap = 4096 * 256 + 777
            _plan(hip, "cc_fixup", extra=cap)
            assert total > cap
            return cap
        total = _components_case(hip, ctx, dev, "bits", n, h, w, 23, True, cap_of, "components fixup")
        assert total > 4096 * 256


# ---- contours and polygons ------------------------------------------------------------------------------------------------
TOL = (256, 655)  # one pixel plus 1 % of the chain's length


def _chains_of(mask):
    """Per distinct frame: stats, chain lengths, chain points, and per record the polygon's vertices and measures."""
    stats, chains = contours_rule.contours(mask, 1)
    lens = np.array([c.size for c in chains], np.uint64)
    pts = np.concatenate(chains).astype(np.int32) if chains else np.zeros(0, np.int32)
    pg = [polygons_rule.polygon(c, mask.shape[1], *TOL) for c in chains]
    verts = [np.array([int(c[i]) for i in pos], np.int32) for c, (pos, _) in zip(chains, pg)]
    v_lens = np.array([v.size for v in verts], np.uint64)
    v_all = np.concatenate(verts) if verts else np.zeros(0, np.int32)
    meas = np.array([m for _, m in pg], np.int64).reshape(len(pg), 4)
    return stats, lens, pts, v_lens, v_all, meas


@pytest.mark.parametrize("source", ["bits", "canny"])
def test_contours_and_polygons_past_their_caps(hip, source):
    """ct_walk (count, write) and ct_place past 65 536 x 4 rows; from bits also pg_simplify / pg_emit past 65 536 x 4
    records and the scan of the chunk sums past 256 chunks of 2 048 records.  Four runs (three behind canny): room for
    everything; a record capacity that ends inside the second trip of the ROW kernels; from bits one that ends inside the
    second trip of the RECORD kernels (which is still the first trip of the row kernels); and room for every record with
    point and vertex capacities that end inside the second trip of the row kernels."""
    n, h, w = 65003, 7, 8
    p = _plan(hip, "ct_rows", n, h, w, units_per_frame=h)
    assert _plan(hip, "cc_rows", n, h, w, units_per_frame=h) == p
    first_trip_frames = p.grid * p.per_group // h + 1     # every frame with a row in the first trip
    idx = _cycle(n)
    with hip.Context(0) as ctx, _Dev(ctx) as dev:
        d_src, masks = _source(dev, source, idx, h, w, 31, lattice=True)
        per = [_chains_of(m) for m in masks]
        w_stats, w_off = _csr(idx, [p[0] for p in per])
        lens, _ = _csr(idx, [p[1] for p in per])
        w_points, w_poff = _csr(idx, [p[2] for p in per])
        v_lens, _ = _csr(idx, [p[3] for p in per])
        w_verts, _ = _csr(idx, [p[4] for p in per])
        w_meas, _ = _csr(idx, [p[5] for p in per])
        total, P, V = w_stats.shape[0], w_points.size, w_verts.size
        w_chain = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        w_voff = np.concatenate([[0], np.cumsum(v_lens)]).astype(np.uint64)
        r1 = int(w_off[first_trip_frames])                # records of the frames the first trip of the row kernels touches
        row_cap, pcap = (r1 + total) // 2, (int(w_chain[r1]) + P) // 2
        assert r1 < row_cap < total and int(w_chain[r1]) < pcap < P
        cut_at = int(np.searchsorted(w_chain[1:], pcap, side="right"))      # the first record whose chain does not fit
        vcap = (int(w_voff[r1]) + int(w_voff[cut_at])) // 2
        assert r1 < cut_at < total and int(w_voff[r1]) < vcap < int(w_voff[cut_at])
        runs = [(total, P, P), (row_cap, P, P), (total, pcap, vcap)]
        if source == "bits":
            _plan(hip, "pg_records", extra=total)
            _plan(hip, "pg_scan_sums", extra=total)
            _plan(hip, "pg_records", extra=row_cap)
            runs.append((65536 * 4 + 4099, P, P))
            _plan(hip, "pg_records", extra=runs[-1][0])
            assert runs[-1][0] < total
        for cap, pc, vc in runs:
            d_stats, d_off, d_poff = dev.filled(cap * 6, S32), dev.filled(n + 1, S64), dev.filled(n + 1, S64)
            d_chain, d_points = dev.filled(cap + 1, S64), dev.filled(pc, S32)
            d_voff, d_verts, d_meas = dev.filled(cap + 1, S64), dev.filled(vc, S32), dev.filled(cap * 4, M64)
            args = (h, w, n, 1, d_stats, cap, d_off, d_chain, d_points, pc, d_poff, TOL[0], TOL[1], d_voff, d_verts, vc, d_meas)
            if source == "bits":
                ctx.dev_polygons_bits(d_src, *args)
            else:
                ctx.dev_canny_polygons(d_src, SIGMA, LO, HI, *args)
            what = f"polygons {source} capacities {cap} of {total}, {pc} of {P}, {vc} of {V}"
            # the rule for capacities: the first `cap` records; the points below point_capacity; a chain that ends beyond
            # it (they are a suffix of the records) has no vertices and the measures (-1, 0, 0, 0); the vertices below
            # vertex_capacity; every offset is the true count
            fit = int(np.searchsorted(w_chain[1:cap + 1], pc, side="right"))   # records whose chain is complete
            voff, meas = w_voff[:cap + 1].copy(), w_meas[:cap].copy()
            voff[fit + 1:] = w_voff[fit]
            meas[fit:] = (-1, 0, 0, 0)
            n_pts, n_verts = min(pc, int(w_chain[cap])), min(vc, int(w_voff[fit]))
            _same(dev.get(d_off, n + 1, np.uint64, S64, what), w_off, what + ": offsets")
            _same(dev.get(d_poff, n + 1, np.uint64, S64, what), w_poff, what + ": point_offsets")
            _same(dev.get(d_stats, cap * 6, np.int32, S32, what).reshape(cap, 6), w_stats[:cap], what + ": stats")
            _same(dev.get(d_chain, cap + 1, np.uint64, S64, what), w_chain[:cap + 1], what + ": chain_offsets")
            _same(dev.get(d_points, pc, np.int32, S32, what, used=n_pts), w_points[:n_pts], what + ": points")
            _same(dev.get(d_voff, cap + 1, np.uint64, S64, what), voff, what + ": vertex_offsets")
            _same(dev.get(d_verts, vc, np.int32, S32, what, used=n_verts), w_verts[:n_verts], what + ": vertices")
            _same(dev.get(d_meas, cap * 4, np.int64, M64, what).reshape(cap, 4), meas, what + ": measures")
            dev.free(d_stats, d_off, d_poff, d_chain, d_points, d_voff, d_verts, d_meas)
        dev.report(f"polygons {source}")


# ---- Euclidean distance transform -----------------------------------------------------------------------------------------
def _edt_case(hip, ctx, dev, source, n, h, w, seed, name):
    idx = _cycle(n)
    d_src, masks = _source(dev, source, idx, h, w, seed)
    want = [edt_rule.transform(m) for m in masks]
    npx = n * h * w
    d_d2, d_d, d_nn = dev.filled(npx, S32), dev.filled(npx, np.float32(-7.0)), dev.filled(npx, S32)
    if source == "bits":
        ctx.dev_edt_bits(d_src, h, w, n, d_d2, d_d, d_nn)
    else:
        ctx.dev_canny_edt(d_src, SIGMA, LO, HI, h, w, n, d_d2, d_d, d_nn)
    for j, (ptr, dtype, fill, what) in enumerate(((d_d2, np.int32, S32, "dist2"), (d_d, np.float32, np.float32(-7.0), "dist"),
                                                  (d_nn, np.int32, S32, "nearest"))):
        got = dev.get(ptr, npx, dtype, fill, f"{name} {source} {what}").reshape(n, h, w)
        for k in range(K):
            assert np.all(got[k::K] == want[k][j]), f"{name} {source}: {what} of the frames of kind {k} differs"
    dev.report(f"{name} {source}")


@pytest.mark.parametrize("source", ["bits", "canny"])
def test_edt_past_the_row_cap(hip, source):
    """edt_rows with eight rows per wave (the branch from 65 536 rows on) and more than 65 536 x 4 waves."""
    n, h, w = 63563, 33, 8
    p = hip.launch_plan("edt_rows", n, h, w)
    assert p.aux == 8 and p.trips == 2 and p.units % (p.grid * p.per_group) != 0
    assert (p.grid * p.per_group * 8) % (K * h) != 0
    with hip.Context(0) as ctx, _Dev(ctx) as dev:
        _edt_case(hip, ctx, dev, source, n, h, w, 41, "edt rows")


def test_edt_past_the_column_cap(hip):
    """edt_columns: more than 65 536 x 4 strips of 64 columns.  Five strips a frame at no more than 65 535 frames: a frame
    one row high.  From bits only: the column kernel reads the row pass's plane, not the source, so it has one form."""
    n, h, w = 52433, 1, 257
    _plan(hip, "edt_columns", n, h, w, units_per_frame=5)
    with hip.Context(0) as ctx, _Dev(ctx) as dev:
        _edt_case(hip, ctx, dev, "bits", n, h, w, 42, "edt columns")


# ---- Hough lines: the global-atomics vote ----------------------------------------------------------------------------------
def _tall_mask(h, w, band, seed, strides):
    """One frame: bands of `band` rows cycling K distinct patterns (one empty, one with every pixel set).  strides: what
    lies between two items of one wave or lane, in rows, or with the unit "points" in set pixels; none may be a multiple
    of the cycle, or the second item would be the first one's copy."""
    pat = _masks(band, w, seed)
    for stride, unit in strides:
        cycle = band * K if unit == "rows" else int(pat.sum())
        assert stride % cycle != 0, f"a stride of {stride} {unit} covers whole cycles of {cycle}"
    m = pat[_cycle(-(-h // band))].reshape(-1, w)[:h]
    return np.ascontiguousarray(m)


def _hough_case(hip, ctx, dev, call, mask, rho, theta, name):
    h, w = mask.shape
    lm = 32
    numangle, numrho = hip.hough_geometry(h, w, rho, theta)
    assert numrho * 4 > 160 * 1024, "a row of the accumulator must not fit in LDS: the global vote"
    tabs = hip.hough_tables(rho, theta, 0.0, numangle)
    want = hough_rule.accumulate(np.flatnonzero(mask), w, numrho, *tabs)
    thr = int(want.max()) // 2
    wl, wv, wb, wc = hough_rule.lines(want, thr, lm, rho, theta)
    assert wc > 0
    cells = (numangle + 2) * (numrho + 2)
    d_lines, d_votes, d_bases = dev.filled(2 * lm, np.uint32(S32)), dev.filled(lm, S32), dev.filled(lm, np.uint32(S32))
    d_counts, d_acc = dev.filled(1, S32), dev.filled(cells, S32)
    call(rho, theta, thr, lm, 0.0, np.pi, d_lines, d_votes, d_bases, d_counts, d_acc)
    k = min(lm, wc)
    _same(dev.get(d_acc, cells, np.int32, S32, name).reshape(numangle + 2, numrho + 2), want, name + ": accumulator")
    assert dev.get(d_counts, 1, np.int32, S32, name)[0] == wc, name + ": count"
    _same(dev.get(d_bases, lm, np.uint32, np.uint32(S32), name, used=k), wb, name + ": bases")
    _same(dev.get(d_votes, lm, np.int32, S32, name, used=k), wv, name + ": votes")
    assert dev.get(d_lines, 2 * lm, np.uint32, np.uint32(S32), name, used=2 * k).tobytes() == wl.tobytes(), name + ": lines"
    dev.report(name)


def test_hough_global_vote_from_bits_past_the_lane_cap(hip):
    """More plane words in a frame than 4 x (2 048 x 256) lanes: every slot of "four words in flight per lane" is used and
    the outer loop takes a second round."""
    h, w = 2105003, 8
    p = _plan(hip, "hough_vote_bits", 1, h, w, trips=5)
    lanes = p.grid * p.per_group            # a frame 8 pixels wide: one word a row
    mask = _tall_mask(h, w, 61, 51, [(lanes, "rows"), (4 * lanes, "rows")])
    with hip.Context(0) as ctx, _Dev(ctx) as dev:
        d_bits = dev.put(np.packbits(mask, axis=-1))
        _hough_case(hip, ctx, dev, lambda *a: ctx.dev_hough_bits(d_bits, 1, h, w, *a), mask, 1.0, np.pi / 4, "hough bits")


def test_hough_global_vote_from_the_strong_plane_past_the_lane_cap(hip):
    """Behind dev_canny: more words than lanes, so a lane holds a second word in flight (slots j >= 1).  The frame is noise
    with flat bands, not a cycle of patterns: no two stretches of its map are alike."""
    h, w = 600003, 8
    _plan(hip, "hough_vote_strong", 1, h, w)
    rng = np.random.default_rng(52)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    for b in range(0, h, 7 * 509):              # flat bands: stretches of the frame without edge pixels
        img[b:b + 509] = 0
    mask = oracle.canny(img, SIGMA, LO, HI) != 0
    assert 0.05 < mask.mean() < 0.5 and not mask[10:500].any()
    with hip.Context(0) as ctx, _Dev(ctx) as dev:
        d_img = dev.put(img)
        _hough_case(hip, ctx, dev, lambda *a: ctx.dev_canny_hough(d_img, SIGMA, LO, HI, h, w, 1, *a), mask, 1.0, np.pi / 4,
                    "hough strong")


def test_hough_global_vote_from_points_past_the_lane_cap(hip):
    """The point-list source: more points in the frame than the capped grid has lanes."""
    h, w = 1100003, 8
    lanes = 2048 * 256
    mask = _tall_mask(h, w, 61, 53, [(lanes, "points")])
    pts = np.flatnonzero(mask).astype(np.uint32)
    p = _plan(hip, "hough_vote_points", 1, h, w, extra=pts.size)
    assert p.grid * p.per_group == lanes and p.units == pts.size
    with hip.Context(0) as ctx, _Dev(ctx) as dev:
        d_pts, d_off = dev.put(pts), dev.put(np.array([0, pts.size], np.uint64))
        _hough_case(hip, ctx, dev, lambda *a: ctx.dev_hough_points(d_pts, d_off, 1, h, w, *a), mask, 1.0, np.pi / 4,
                    "hough points")


# ---- Hough circles ----------------------------------------------------------------------------------------------------------
def _circles_case(hip, ctx, dev, call, mask, gx, gy, name):
    h, w = mask.shape
    lo, hi, cs, cm = 2, 5, 2, 64
    want = hough_circles_rule.accumulate(mask, gx, gy, lo, hi, cs)
    thr = int(want.max()) // 2
    rec, n_peaks = hough_circles_rule.circles(mask, want, lo, hi, cs, thr, 3, 4, cm)
    assert n_peaks > 0
    d_rec, d_counts, d_peaks = dev.filled(cm * 6, S32), dev.filled(1, S32), dev.filled(1, S32)
    d_acc = dev.filled(want.size, S32)
    call(lo, hi, cs, thr, 3, 4, cm, d_rec, d_counts, d_peaks, d_acc)
    _same(dev.get(d_acc, want.size, np.int32, S32, name).reshape(want.shape), want, name + ": accumulator")
    assert dev.get(d_peaks, 1, np.int32, S32, name)[0] == n_peaks, name + ": peak count"
    assert dev.get(d_counts, 1, np.int32, S32, name)[0] == len(rec), name + ": count"
    _same(dev.get(d_rec, cm * 6, np.int32, S32, name, used=6 * len(rec)).reshape(-1, 6), rec.reshape(-1, 6), name + ": records")
    dev.report(name)


def test_circle_vote_from_bits_past_the_chunk_cap(hip):
    h, w = 140003, 8
    p = _plan(hip, "circles_vote_bits", 1, h, w)
    mask = _tall_mask(h, w, 61, 61, [(p.grid * 64, "rows")])       # a chunk is 64 words, here 64 rows
    rng = np.random.default_rng(62)
    gx, gy = (rng.integers(-1020, 1021, (h, w)).astype(np.int16) for _ in range(2))
    gx[rng.random((h, w)) < 0.1] = 0
    gy[rng.random((h, w)) < 0.1] = 0
    with hip.Context(0) as ctx, _Dev(ctx) as dev:
        d_bits, d_gx, d_gy = dev.put(np.packbits(mask, axis=-1)), dev.put(gx), dev.put(gy)
        _circles_case(hip, ctx, dev, lambda *a: ctx.dev_hough_circles_bits(d_bits, d_gx, d_gy, 1, h, w, *a), mask, gx, gy,
                      "circles bits")


def test_circle_vote_from_the_strong_plane_past_the_chunk_cap(hip):
    """Behind dev_canny; noise with flat bands, as for the Hough vote from the strong plane."""
    h, w = 140003, 8
    _plan(hip, "circles_vote_strong", 1, h, w)
    rng = np.random.default_rng(63)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    for b in range(0, h, 7 * 509):
        img[b:b + 509] = 0
    mask = oracle.canny(img, SIGMA, LO, HI) != 0
    assert 0.05 < mask.mean() < 0.5
    gx, gy = hough_circles_rule.sobel(oracle.gaussian(img, SIGMA))
    with hip.Context(0) as ctx, _Dev(ctx) as dev:
        d_img = dev.put(img)
        _circles_case(hip, ctx, dev, lambda *a: ctx.dev_canny_hough_circles(d_img, SIGMA, LO, HI, h, w, 1, *a), mask, gx, gy,
                      "circles strong")


def test_circle_steps_past_the_grid_cap(hip):
    n = 8192 * 256 + 1003
    _plan(hip, "circles_steps", extra=n)
    rng = np.random.default_rng(64)
    gx, gy = (rng.integers(-32768, 32768, n).astype(np.int16) for _ in range(2))
    gx[::13] = 0
    gy[::17] = 0
    want_x, want_y = hough_circles_rule.step(gx, gy)
    with hip.Context(0) as ctx, _Dev(ctx) as dev:
        d_gx, d_gy, d_sx, d_sy = dev.put(gx), dev.put(gy), dev.filled(n, S32), dev.filled(n, S32)
        ctx.dev_hough_circles_steps(d_gx, d_gy, n, d_sx, d_sy)
        _same(dev.get(d_sx, n, np.int32, S32, "steps"), want_x, "steps: sx")
        _same(dev.get(d_sy, n, np.int32, S32, "steps"), want_y, "steps: sy")
        dev.report("circle steps")


# ---- colour -> gray, the standalone conversion -------------------------------------------------------------------------------
@pytest.mark.parametrize("order,ch", [("bgr", 3), ("rgb", 4)], ids=["bgr8", "rgba8"])
def test_to_gray_past_the_grid_cap(hip, order, ch):
    """One trip covers 8 192 x 256 groups of 16 pixels, 33.5 M pixels: this is the one case above the 20 M pixels the others
    keep to, because the cap cannot be crossed below it (a byte plane: 34 MiB out, 3 or 4 times that in)."""
    n_px = 8192 * 256 * 16 + 16 * 1009 + 5
    _plan(hip, "to_gray", extra=n_px)
    rng = np.random.default_rng(71)
    block = rng.integers(0, 256, (1000003, ch), dtype=np.uint8)       # a prime number of pixels, cycled
    src = np.ascontiguousarray(block[np.arange(n_px) % block.shape[0]])
    with hip.Context(0) as ctx, _Dev(ctx) as dev:
        rgb = src[:, :3] if order == "rgb" else src[:, 2::-1]
        want = gray_rule_of(rgb, ctx.get_option("gray_rule"))
        d_src, d_gray = dev.put(src), dev.filled(n_px, S8)
        ctx.dev_to_gray(d_src, hip.layout_of((1, 1, ch), order), 1, n_px, 1, d_gray)
        _same(dev.get(d_gray, n_px, np.uint8, S8, "to_gray"), want, f"to_gray {order}{ch}")
        dev.report(f"to_gray {order}{ch}")
