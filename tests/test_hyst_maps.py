"""CPU checks of the designed hysteresis maps (tests/hyst_maps.py) that tests/test_gpu_hyst_maps.py runs through the
kernels: the tile model equals the oracle on every map, every slip of the model -- one per line of load_tile /
process_tile_with that can be wrong on its own -- changes a designed frame, every link case hangs on its one link pixel,
and the delay lines and the zigzag hold the sweep counts they were built for.  These are conditions on the inputs and on
the reference, not on the kernels.

The two one-directional fill slips cannot change a map (hyst_maps' docstring says why); they are checked on one
application of fill_runs, where the row atlases catch both, and test_fill_slips_that_cannot_show pins that they stay
invisible in the maps, so that nobody reads their absence from the table below as a hole.
"""
import numpy as np
import pytest

import hyst_maps as hm
import oracle

_memo = {}


def _oracle(batch, lo=hm.LO, hi=hm.HI):
    return np.stack([oracle.hysteresis(f, lo, hi) for f in batch])


def atlases():
    """name -> (batch, names of the frames); built once."""
    if not _memo:
        for shape in hm.LINK_SHAPES:
            batch, metas = hm.link_atlas(shape)
            _memo[f"link{shape[0]}x{shape[1]}"] = (batch, [m["name"] for m in metas])
        for shape in hm.QUIRK_SHAPES:
            batch, metas = hm.quirk_atlas(shape)
            _memo[f"quirk{shape[0]}x{shape[1]}"] = (batch, [m["name"] for m in metas])
        for shape in hm.ISOLATION_SHAPES:
            for name, (batch, _) in hm.isolation_atlas(shape).items():
                _memo[f"isolation_{name}{shape[0]}x{shape[1]}"] = (batch, [f"frame {i}" for i in range(len(batch))])
        batch, names = hm.in_tile_atlas()
        _memo["in_tile"] = (batch, names)
        _memo["zigzag"] = (hm.zigzag(), ["zigzag"])
        for name, batch in (("rows", hm.row_atlas()), ("row_gaps", hm.row_gap_atlas()), ("rows_wide", hm.row_wide_atlas())):
            _memo[name] = (batch, [f"row frame {i}: {''.join('.wS'[int(v >= hm.LO) + int(v >= hm.HI)] for v in f[0])}"
                                   for i, f in enumerate(batch)])
    return _memo


ROW_ATLASES = ("rows", "row_gaps", "rows_wide")


@pytest.fixture(scope="module")
def want():
    return {name: _oracle(batch) for name, (batch, _) in atlases().items()}


def test_the_model_equals_the_oracle_on_every_map(want):
    for name, (batch, names) in atlases().items():
        got, sweeps = hm.model_sweeps(batch)
        bad = np.flatnonzero((got != want[name]).any(axis=(1, 2)))
        assert bad.size == 0, f"{name}: the model differs from the oracle on {names[bad[0]]} ({bad.size} frames)"
        print(f"{name}: {len(batch)} frames of {batch.shape[1]} x {batch.shape[2]}, model sweeps {sweeps}")


def test_frames_that_must_stay_empty_do(want):
    for shape in hm.ISOLATION_SHAPES:
        for name, (batch, empty) in hm.isolation_atlas(shape).items():
            w = want[f"isolation_{name}{shape[0]}x{shape[1]}"]
            for i in empty:
                assert not w[i].any(), (name, shape, i)
            if name == "row_end":
                assert np.array_equal(w[0] != 0, batch[0] >= hm.HI)   # the weak pixels one tile row down are not reached
            if name == "changing_row":
                assert np.count_nonzero(w[0]) == 11 and hm.model_sweeps(batch)[1] == 1


def test_quirk_frames_show_the_quirk(want):
    for shape in hm.QUIRK_SHAPES:
        batch, metas = hm.quirk_atlas(shape)
        w = want[f"quirk{shape[0]}x{shape[1]}"]
        for f, m in enumerate(metas[:12]):
            assert w[f][m["link"]] == 255 and w[f][m["seed"]] == 255
            assert w[f][m["dest"]] == (0 if m["link"] == (1, 0) else 255), m["name"]
        assert w[12][0, 1] == 0 and all(w[12][oy, ox + 1] == 255 for oy, ox in hm.QUIRK_ORIGINS[1:])


SLIP_ATLASES = {"pull": ("link",), "lb_up": ("link",), "push": ("link",), "quirk": ("quirk",),
                "fill": ROW_ATLASES, "frame": ("isolation",)}


@pytest.mark.parametrize("slip", [s for s in hm.SLIPS if s not in hm.INVISIBLE_SLIPS])
def test_every_slip_changes_a_designed_frame(want, slip):
    """The table of DESIGN.md section 22: which frame catches which slip."""
    kinds = SLIP_ATLASES[slip.split("_")[0] if not slip.startswith("lb_up") else "lb_up"]
    caught = []
    for name, (batch, names) in atlases().items():
        if not name.startswith(kinds):
            continue
        got, _ = hm.model_sweeps(batch, slip=slip)
        bad = np.flatnonzero((got != want[name]).any(axis=(1, 2)))
        if bad.size:
            caught.append(f"{name}: {bad.size} frames, first {names[bad[0]]}")
    print(f"{slip}: " + ("; ".join(caught) if caught else "NOT CAUGHT"))
    assert caught, f"no designed frame notices the slip {slip}"
    if kinds == ("link",):   # both geometries have to notice
        assert len(caught) == len(hm.LINK_SHAPES), caught


def test_fill_slips_that_cannot_show(want):
    """One-directional fills: wrong on one application of fill_runs for thousands of atlas rows, and yet the same maps,
    because the next round's 3x3 pull adds the horizontal neighbours the fill left out."""
    for name in ("rows", "row_gaps"):   # the 64-pixel rows: one word each
        batch, _ = atlases()[name]
        p, g = batch >= hm.LO, batch >= hm.HI
        assert np.array_equal(hm.fill_runs(p, g) * 255, want[name]), name   # one application IS the row's flood
        for slip in hm.INVISIBLE_SLIPS:
            short = int((hm.fill_runs(p, g, slip) != hm.fill_runs(p, g)).any(axis=(1, 2)).sum())
            print(f"{name}: one application of fill_runs with {slip} falls short on {short} of {len(batch)} frames")
            assert short > len(batch) // 4
            assert np.array_equal(hm.model_sweeps(batch, slip=slip)[0], want[name])


def test_the_row_atlas_is_complete():
    rows = hm.row_atlas()
    assert rows.shape == (6049, 1, 64)
    keys = {(f[0] >= hm.LO).tobytes() + (f[0] >= hm.HI).tobytes() for f in rows}
    assert len(keys) == 6049
    full = [f[0] for f in rows if (f[0] >= hm.LO).all()]
    assert {int(np.flatnonzero(f >= hm.HI)[0]) for f in full} >= {0, 63}


@pytest.mark.parametrize("shape", hm.LINK_SHAPES)
def test_every_link_case_hangs_on_its_link_pixel(shape):
    batch, metas = hm.link_atlas(shape)
    assert len(batch) == 44
    pairs = set()
    for frame, m in zip(batch, metas):
        (ly, lx), (dy, dx) = m["link"], m["dest"]
        assert (ly // 64, lx // 64) != (1, 1) and (dy // 64, dx // 64) == (1, 1) and max(abs(ly - dy), abs(lx - dx)) == 1
        pairs.add(((ly // 64, lx // 64), dy % 64 if lx in (63, 128) else dx % 64, (dy - ly, dx - lx)))
        whole = oracle.hysteresis(frame, hm.LO, hm.HI)
        assert np.array_equal(whole != 0, frame != 0), m["name"]   # the whole path is reached ...
        cut = frame.copy()
        cut[m["link"]] = 0
        lost = oracle.hysteresis(cut, hm.LO, hm.HI)
        assert all(lost[p] == 0 for p in m["far"]) and lost[m["seed"]] == 255, m["name"]   # ... and only through the link
        # the delay line: no order of the tiles sets the link pixel before sweep 2, by when the centre tile has run twice
        early = hm.earliest_sweep(frame)
        assert early[m["link"]] >= 2 and early[m["dest"]] >= early[m["link"]], (m["name"], early[m["link"]])
    sources = {p[0] for p in pairs}
    assert sources == {(a, b) for a in range(3) for b in range(3)} - {(1, 1)}
    for side in ((0, 1), (2, 1), (1, 0), (1, 2)):   # straight and both diagonals at lanes 0, 31, 63 (and 32)
        got = {(lane, step) for src, lane, step in pairs if src == side}
        assert len(got) == 10 and {lane for lane, _ in got} == set(hm.LINK_LANES), (side, sorted(got))


def test_the_zigzag_needs_two_chunks_of_sweeps():
    z = hm.zigzag()
    floor = hm.reported_iterations_floor(z)
    _, sweeps = hm.model_sweeps(z)
    print(f"zigzag: at least {floor} reported iterations (16 re-entries of the start tile), model sweeps {sweeps}")
    assert floor >= 12 and floor == 17 and floor <= sweeps + 1


def test_value_atlas_expectations():
    """Which calls the value atlas expects to be refused, and that every accepted batch has a non-trivial answer
    somewhere."""
    refused, kept = [], 0
    for lo, hi in hm.VALUE_PAIRS:
        for width in hm.VALUE_WIDTHS:
            batches = [hm.value_frames(lo, hi, width), hm.value_random(lo, hi, (24 if width == 64 else 23, width))]
            if lo <= 0:
                batches += list(hm.value_in_domain(lo, hi, width))
            for b in batches:
                if hm.value_status(b, lo, hi):
                    refused.append((lo, hi, width, len(b)))
                else:
                    kept += int(_oracle(b, lo, hi).any())
    print("refused:", refused)
    assert {(lo, hi) for lo, hi, _, _ in refused} == {(0, 255), (-3, 1), (300, 200)}
    ok, bad = hm.value_in_domain(0, 255, 64)
    assert hm.value_status(ok, 0, 255) == 0 and hm.value_status(bad, 0, 255) == hm.ERR_DOMAIN
    assert (bad < 0).sum() == 1 and bad[-1, -1, -1] < 0
    assert kept >= 10
