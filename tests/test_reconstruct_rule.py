"""Reconstruction, host side: canny_hip_reconstruct_bits (plain C++, no device) against
tests/reconstruct_rule.py byte for byte, the two Python restatements against each other and against scipy, the documented facts
of the rule, the named slips on their designed maps, the model of the tile flood's launches, the hysteresis identity, the
refused calls, the header and the bindings, and the host file and the word steps under the host compiler's sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage as ndi

import binarize_rule
import reconstruct_rule as R
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (3, 5), (33, 257), (64, 512), (65, 513), (130, 1030))
DENSITIES = (0.3, 0.45, 0.6, 0.8)
STRUCT = {4: ndi.generate_binary_structure(2, 1), 8: np.ones((3, 3), bool)}


def both(marker, mask, op, c, dirty=True):
    """The host C++ and the numpy rule on bool [n, h, w] (dirty pad bits in), compared; -> (unpacked output, info)."""
    mask = np.asarray(mask, bool)
    w = mask.shape[-1]
    rng = np.random.default_rng(mask.size + op)
    pk = (lambda a: R.pack_dirty(a, rng)) if dirty else R.pack
    mb, kb = pk(mask), None if marker is None else pk(np.asarray(marker, bool))
    want, want_info = R.reconstruct(kb, mb, w, op, c)
    got, info = capi.reconstruct_bits(kb, mb, w, op, c)
    assert np.array_equal(got, want), f"op {op} c {c}: the host's bytes differ from the rule"
    assert np.array_equal(info, want_info), (op, c, info.tolist(), want_info.tolist())
    return R.unpack(got, w), info


def random_case(h, w, density, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random((h, w)) < density
    return rng.random((h, w)) < 0.02, mask


def clear_border_by_labels(mask, c):
    lab, _ = ndi.label(mask, STRUCT[c])
    touching = np.unique(lab[R.border(*mask.shape)])
    return mask & ~np.isin(lab, touching[touching > 0])


# ---- the two restatements, scipy and the host -----------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CONNECTIVITIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_the_rule_equals_scipy_and_the_host_equals_the_rule(shape, c):
    h, w = shape
    for i, density in enumerate(DENSITIES):
        marker, mask = random_case(h, w, density, 38 * h + w + i)
        out, info = both(marker[None], mask[None], R.SEEDED, c)
        assert np.array_equal(out[0], ndi.binary_propagation(marker & mask, STRUCT[c], mask=mask))
        assert info[0].tolist() == [out.sum(), mask.sum(), (marker & mask).sum()]
        out, info = both(None, mask[None], R.FILL_HOLES, c)
        assert np.array_equal(out[0], ndi.binary_fill_holes(mask, STRUCT[12 - c]))
        assert info[0].tolist() == [out.sum(), mask.sum(), (R.border(h, w) & ~mask).sum()]
        out, info = both(None, mask[None], R.CLEAR_BORDER, c)
        assert np.array_equal(out[0], clear_border_by_labels(mask, c))
        assert info[0].tolist() == [out.sum(), mask.sum(), (R.border(h, w) & mask).sum()]


@pytest.mark.parametrize("c", R.CONNECTIVITIES)
def test_the_stack_flood_equals_the_iterated_dilation(c):
    for seed in range(12):
        rng = np.random.default_rng(seed)
        h, w = int(rng.integers(1, 14)), int(rng.integers(1, 20))
        marker, mask = rng.random((h, w)) < 0.1, rng.random((h, w)) < (0.3 + 0.05 * seed)
        for op in R.OPS:
            k = marker if op == R.SEEDED else None
            assert np.array_equal(R.flood_px(k, mask, op, c), R.reconstruct_px(k, mask, op, c)[0]), (seed, op)


# ---- the documented facts -------------------------------------------------------------------------------------------------
def test_subsets_idempotence_and_monotony():
    for seed in range(6):
        marker, mask = random_case(40, 77, 0.35 + 0.08 * seed, seed)
        more = marker | (np.random.default_rng(100 + seed).random(mask.shape) < 0.02)
        for c in R.CONNECTIVITIES:
            seeded = both(marker[None], mask[None], R.SEEDED, c)[0][0]
            assert not (seeded & ~mask).any()
            assert np.array_equal(both(seeded[None], mask[None], R.SEEDED, c)[0][0], seeded)
            assert np.array_equal(both(marker[None], seeded[None], R.SEEDED, c)[0][0], seeded)
            assert not (seeded & ~both(more[None], mask[None], R.SEEDED, c)[0][0]).any(), "monotone in the marker"
            assert np.array_equal(both(mask[None], mask[None], R.SEEDED, c)[0][0], mask)
            filled = both(None, mask[None], R.FILL_HOLES, c)[0][0]
            assert not (mask & ~filled).any()
            assert np.array_equal(both(None, filled[None], R.FILL_HOLES, c)[0][0], filled)
            cleared = both(None, mask[None], R.CLEAR_BORDER, c)[0][0]
            assert not (cleared & ~mask).any()
            assert np.array_equal(both(None, cleared[None], R.CLEAR_BORDER, c)[0][0], cleared)


def test_the_demonstration_scene():
    s = R.demo_scene()
    assert s.shape == (96, 160) and s.sum() == 1735
    assert ndi.label(~s, STRUCT[4])[1] == 2
    filled, info = both(None, s[None], R.FILL_HOLES, 8)
    assert info[0, 0] == 3248 and info[0, 0] - info[0, 1] == 1513 and ndi.label(~filled[0], STRUCT[4])[1] == 1
    assert both(R.first_pixel(s)[None], s[None], R.SEEDED, 8)[1][0].tolist() == [427, 1735, 1]
    assert both(None, s[None], R.CLEAR_BORDER, 8)[1][0].tolist() == [1735, 1735, 0]
    moved = np.roll(s, -10, axis=1)                       # the ring (columns 10 .. 70) now touches column 0, the bar nothing
    lab, n = ndi.label(moved, STRUCT[8])
    assert n == 2
    cleared = both(None, moved[None], R.CLEAR_BORDER, 8)[0][0]
    kept = [i for i in (1, 2) if (cleared & (lab == i)).any()]
    assert len(kept) == 1 and np.array_equal(cleared, lab == kept[0]), "clears the component that touches, and only it"


def test_the_diamond_ring_separates_the_connectivities():
    d = np.zeros((9, 9), bool)
    d[1:8, 1:8] = R.diamond()
    assert {(y, x) for y, x in np.argwhere(R.diamond())} == ({(3 - i, i) for i in range(4)} | {(3 + i, i) for i in range(4)} |
                                                            {(3 - i, 6 - i) for i in range(4)} | {(3 + i, 6 - i) for i in range(4)})
    for c, want in ((8, 13), (4, 0)):
        info = both(None, d[None], R.FILL_HOLES, c)[1]
        assert info[0, 0] - info[0, 1] == want


def test_the_zigzag():
    z = R.zigzag(65, 40)
    assert z.sum() == 1319 and ndi.label(z, STRUCT[4])[1] == 1 and ndi.label(z, STRUCT[8])[1] == 1
    crossings = int((z[63] & z[64]).sum())
    assert crossings == 20, "the path crosses the tile border between rows 63 and 64 twenty times"
    for c in R.CONNECTIVITIES:
        state, launches = R.tile_model(R.first_pixel(z), z, c)
        assert np.array_equal(state, z) and launches == 22
    # a launch runs each tile once: a path that alternates between two tiles advances at most two crossings a launch
    assert -(-crossings // 2) == 10 > 4


# ---- the slips ------------------------------------------------------------------------------------------------------------
def packed(d):
    pk = R.pack_dirty if d["dirty"] else R.pack
    return None if d["marker"] is None else pk(d["marker"]), pk(d["mask"])


@pytest.mark.parametrize("name", R.DESIGNED)
def test_every_slip_changes_its_designed_map_and_the_host_does_not_slip(name):
    d = R.designed(name)
    assert d["slip"] in R.MUTANTS
    w = d["mask"].shape[-1]
    kb, mb = packed(d)
    want, want_info = R.reconstruct(kb, mb, w, d["op"], d["c"])
    got, info = capi.reconstruct_bits(kb, mb, w, d["op"], d["c"])
    assert np.array_equal(got, want) and np.array_equal(info, want_info)
    if d["slip"] in ("no_tile_carry", "halo_wrong_row", "first_chunk_only"):
        args = (d["marker"][0], d["mask"][0], d["c"])
        assert np.array_equal(R.tile_model(*args)[0], R.unpack(want, w)[0]), "the tile scheme reaches the global fixed point"
        assert not np.array_equal(R.tile_model(*args, mutant=d["slip"])[0], R.unpack(want, w)[0])
    else:
        assert not np.array_equal(R.reconstruct(kb, mb, w, d["op"], d["c"], mutant=d["slip"])[0], want)


@pytest.mark.parametrize("c", R.CONNECTIVITIES)
def test_the_tile_model_reaches_the_global_fixed_point(c):
    for seed in range(4):
        mask = R.blobs(70, 150, seed, 5, 0.48)
        marker = np.random.default_rng(seed).random(mask.shape) < 0.003
        state, launches = R.tile_model(marker, mask, c, tile=(16, 64))
        assert np.array_equal(state, R.reconstruct_px(marker, mask, R.SEEDED, c)[0]) and launches >= 1


# ---- pad bits -------------------------------------------------------------------------------------------------------------
def test_pad_bits_are_ignored_on_input_and_zero_on_output():
    for w in (1, 7, 9, 13, 61):
        marker, mask = random_case(20, w, 0.7, w)
        for op in R.OPS:
            k = marker[None] if op == R.SEEDED else None
            clean = capi.reconstruct_bits(None if k is None else R.pack(k), R.pack(mask[None]), w, op, 8)
            dirty = capi.reconstruct_bits(None if k is None else R.pack_dirty(k), R.pack_dirty(mask[None]), w, op, 8)
            assert np.array_equal(clean[0], dirty[0]) and np.array_equal(clean[1], dirty[1])
            assert np.array_equal(R.pack(R.unpack(dirty[0], w)), dirty[0]), "pad bits of the output"


# ---- hysteresis thresholding of any plane -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CONNECTIVITIES)
def test_two_binarizations_and_seeded_are_hysteresis_thresholding(c):
    frame = synth_frame(120, 200, 7)[None]
    lo, hi = 90, 170
    low = binarize_rule.binarize(frame, binarize_rule.FIXED, lo)[0]
    high = binarize_rule.binarize(frame, binarize_rule.FIXED, hi)[0]
    out = capi.reconstruct_bits(high, low, 200, R.SEEDED, c)[0]
    lab, _ = ndi.label(frame[0] > lo, STRUCT[c])
    keep = np.unique(lab[frame[0] > hi])
    want = np.isin(lab, keep[keep > 0])
    assert want.any() and not want.all() and np.array_equal(R.unpack(out, 200)[0], want)


# ---- refused calls --------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing_and_info_may_be_null():
    L = capi.load()
    n, h, w, rb = 2, 6, 9, 2
    rng = np.random.default_rng(3)
    mask, marker = R.pack(rng.random((n, h, w)) < 0.6), R.pack(rng.random((n, h, w)) < 0.1)
    vp = capi.C.c_void_p
    n_out = n * h * rb
    S8 = 0x5A5A5A5A5A5A5A5A

    def call(mk=1, ms=1, n=n, h=h, w=w, op=R.SEEDED, c=8, out=1, info=1, off=0):
        o, inf = np.full(n_out + 8, 0x5A, np.uint8), np.full(3 * 2 + 4, S8, np.int64)
        st = L.canny_hip_reconstruct_bits(capi._hp(marker) if mk else None, capi._hp(mask) if ms else None, n, h, w, op, c,
                                          capi._hp(o) if out else None, vp(inf.ctypes.data + off) if info else None)
        if st:
            assert (o == 0x5A).all() and (inf == S8).all(), "a refused call wrote something"
        else:
            assert (o[n_out:] == 0x5A).all() and (inf[6:] == S8).all() and (info or (inf == S8).all())
        return st

    assert call() == 0 and call(info=0) == 0 and call(c=4) == 0
    assert call(mk=0, op=R.FILL_HOLES) == 0 and call(mk=0, op=R.CLEAR_BORDER, c=4, info=0) == 0
    for kw in (dict(mk=0), dict(ms=0), dict(out=0), dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(op=-1), dict(op=3),
               dict(c=0), dict(c=6), dict(c=12), dict(op=R.FILL_HOLES), dict(op=R.CLEAR_BORDER), dict(off=4), dict(off=1)):
        assert call(**kw) == 1, kw
    for kw in (dict(h=32769), dict(w=32769), dict(n=65536), dict(h=32768, w=32768 * 2)):
        assert call(**kw) == 2, kw
    # buffers that overlap: maps 24 B, info 48 B
    buf = np.full(400, 0x5A, np.uint8)
    at = lambda o: vp(buf.ctypes.data + o)
    for k_at, m_at, o_at, f_at in ((0, 30, 0, 200), (0, 30, 23, 200), (0, 30, 53, 200), (0, 30, 40, 200), (0, 30, 100, 16),
                                   (0, 30, 100, 120), (0, 30, 100, 56), (0, 30, 100, 0)):
        st = L.canny_hip_reconstruct_bits(at(k_at), at(m_at), n, h, w, R.SEEDED, 8, at(o_at), at(f_at))
        assert st == 1 and (buf == 0x5A).all(), (k_at, m_at, o_at, f_at)
    buf[:60] = 0
    assert L.canny_hip_reconstruct_bits(at(0), at(30), n, h, w, R.SEEDED, 8, at(64), at(96)) == 0 and (buf[144:] == 0x5A).all()


# ---- header and bindings --------------------------------------------------------------------------------------------------
def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 2700
    assert capi.load().canny_hip_version() >= 2700
    for word in ("0.27.0: + morphological reconstruction of packed bit maps", "0.26.0: + thinning of packed bit maps",
                 "THE PAD BITS OF THE INPUTS ARE IGNORED", "EVERYTHING OUTSIDE THE\n *     FRAME IS NOT PART OF ANY SET",
                 "THE BACKGROUND TAKES THE DUAL\n *     CONNECTIVITY", "c' = 12 - c", "binary_propagation", "binary_fill_holes",
                 "clear_border", "apply_hysteresis_threshold", "\"reconstruct_route\"", "\"last_reconstruct_launches\"",
                 "SYNCHRONISE THE STREAM", "NO launch or sweep count", "3248 pixels (1513", "keeps 427", "13 pixels at c = 8",
                 "grey-level reconstruction", "per-tile dirty stamps", "a label-based route", "an asynchronous form"):
        assert word in header, word
    for name in ("canny_hip_dev_reconstruct_bits", "canny_hip_dev_canny_reconstruct", "canny_hip_reconstruct_batch",
                 "canny_hip_reconstruct_bits", "canny_hip_selftest_reconstruct_plan"):
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
        getattr(capi.load(), name)
    for method in ("dev_reconstruct_bits", "dev_canny_reconstruct", "reconstruct_batch"):
        assert hasattr(capi.Context, method), method
    assert callable(capi.reconstruct_bits) and callable(capi.reconstruct_plan)
    assert (capi.RECON_SEEDED, capi.RECON_FILL_HOLES, capi.RECON_CLEAR_BORDER) == R.OPS == (0, 1, 2)
    assert (capi.RECON_ROUTE_AUTO, capi.RECON_ROUTE_STEPWISE, capi.RECON_ROUTE_TILES) == (0, 1, 2)
    assert capi.RECON_INFO == R.INFO == 3 and re.search(r"#define CANNY_HIP_RECON_INFO 3\b", header)
    for i, m in enumerate(("SEEDED", "FILL_HOLES", "CLEAR_BORDER")):
        assert re.search(rf"CANNY_HIP_RECON_{m} = {i}\b", header), m
    for i, part in enumerate(capi.RECON_PARTS):
        assert re.search(rf"CANNY_HIP_RECON_PART_{part.upper()} = {i}\b", header), part
    assert re.search(r"CANNY_HIP_RECON_PARTS = 2\b", header) and len(capi.RECON_PARTS) == 2


def test_the_profile_parts_are_refused_before_the_device_is_touched():
    fn = capi.load().canny_hip_profile_part_get
    D, Lg = capi.C.c_double, capi.C.c_long
    for part in (0, 1, 2, -1):
        ms, n = D(-1.0), Lg(-1)
        assert fn(None, b"reconstruct", part, capi.C.byref(ms), capi.C.byref(n)) == 1 and (ms.value, n.value) == (-1.0, -1)


# ---- the host rule and the word steps under the host compiler's sanitizers --------------------------------------------------
def run_sanitized(tmp_path, name, sources, token):
    exe = tmp_path / name
    csrc = os.path.join(ROOT, "canny_edge_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "cpp", name + ".cpp")] +
                          [os.path.join(csrc, s) for s in sources] + ["-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and token in r.stdout, r.stdout + r.stderr


def test_host_rule_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_reconstruct_host.cpp has its own main and is compiled together with csrc/canny_reconstruct_host.cpp
    alone: nothing of it is loaded into this interpreter, and no device is involved."""
    run_sanitized(tmp_path, "test_reconstruct_host", ["canny_reconstruct_host.cpp"], "reconstruct ok")


def test_the_word_steps_of_the_kernels_equal_the_bit_by_bit_loop(tmp_path):
    """csrc/canny_recon_words.h is what the kernels of canny_reconstruct.hip run per 64-bit word; it is plain C++ apart from
    its qualifiers, so tests/cpp/test_recon_words.cpp (own main) runs the fill on the host against the bit-by-bit loop on every
    single-run mask with every seed position, carries in from both sides and random words, and the dilation step against a
    per-pixel restatement."""
    run_sanitized(tmp_path, "test_recon_words", [], "recon words ok")
