"""The edge-curve rule (include/canny_hip.h) without a GPU: what follows from the rule, asserted on
every map through the plain-Python restatement of tests/curves_rule.py, and canny_hip_curves_from_bits -- the rule in plain
C++ on one host bit map -- against that restatement word for word, at exact, halved and zero capacities.

The oracle's maps of synth_frame are open curves without a junction, so they alone prove little: the designed and the
random maps carry the weight."""
import os
import subprocess

import numpy as np
import pytest

import components_rule as cr
import contours_rule
import curves_rule as rule
import oracle
from canny_edge_amd import capi
from canny_edge_amd.synth import synth_frame

MIN_LENGTHS = (1, 3, 10)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maps():
    maps = dict(rule.designed_maps())
    maps.update(rule.random_maps())
    maps.update({f"directed64x72_{k}": v for k, v in cr.directed_masks(64, 72).items()})
    maps.update({f"directed9x2_{k}": v for k, v in cr.directed_masks(9, 2).items()})
    return maps


MAPS = _maps()
_oracle_cache = {}


def _oracle_map(h, w, seed):
    if (h, w, seed) not in _oracle_cache:
        _oracle_cache[(h, w, seed)] = oracle.canny(synth_frame(h, w, seed), 1.4, 50, 150) != 0
    return _oracle_cache[(h, w, seed)]


@pytest.mark.parametrize("name", sorted(MAPS))
def test_what_follows_from_the_rule(name):
    rule.check_invariants(MAPS[name])


def test_the_designed_maps_give_the_curves_they_were_drawn_for():
    d = rule.designed_maps()

    def recs(name, min_length=1):
        return rule.curves(d[name], min_length)[0]

    for ring in ("square_ring", "diamond_ring"):
        r = recs(ring)
        assert r.shape[0] == 1 and r[0, rule.POINTS] == 16 and r[0, rule.FLAGS] & 0xF == rule.CLOSED, ring
    links = rule.link_sets(d["diamond_ring"])
    assert all(dd & 1 for ds in links.values() for dd in ds), "the diamond has diagonal links only"
    saw_links = rule.link_sets(d["sawtooth_ring"])
    assert sum(1 for ds in saw_links.values() if len(ds) == 2 and ds[1] <= 3) > 1, "several closed-curve candidates"
    r = recs("sawtooth_ring")
    assert r.shape[0] == 1 and r[0, rule.FLAGS] & 0xF == rule.CLOSED and r[0, rule.POINTS] == int(d["sawtooth_ring"].sum())
    for name, arms in (("plus", 4), ("x", 4), ("t", 3)):
        r = recs(name)
        assert r.shape[0] == arms, name
        assert all(bool(f & rule.START_JUNCTION) != bool(f & rule.END_JUNCTION) for f in r[:, rule.FLAGS]), name
        assert int(r[:, rule.POINTS].sum()) == int(d[name].sum()) + arms - 1, f"{name}: the junction ends every arm"
    r = recs("lollipop")
    loops = [x for x in r if x[rule.START] == x[rule.END]]
    assert r.shape[0] == 2 and len(loops) == 1, "a loop hanging on a junction, and the stem"
    assert loops[0][rule.FLAGS] & 0xF == rule.START_JUNCTION | rule.END_JUNCTION
    r = recs("figure_eight")
    assert r.shape[0] == 2 and all(x[rule.START] == x[rule.END] and x[rule.POINTS] == 5 for x in r)
    r = recs("two_nodes")
    assert r.tolist() == [[6, 7, 2, 0]], "a curve between two adjacent nodes has two points"
    assert recs("two_nodes", 3).shape[0] == 0
    r = recs("checkerboard")
    assert r.shape[0] == 20 and np.all(r[:, rule.FLAGS] == rule.ISOLATED) and np.all(r[:, rule.START] == r[:, rule.END])
    assert recs("checkerboard", 2).shape[0] == 0
    r = recs("staircase")
    assert r.shape[0] == 1 and r[0, rule.POINTS] == int(d["staircase"].sum()), "bridged diagonals are no links"
    for name, n in (("1x1", 1), ("1x70", 70), ("70x1", 70), ("serpentine", int(d["serpentine"].sum()))):
        r = recs(name)
        assert r.shape[0] == 1 and r[0, rule.POINTS] == n, name
    # min_length drops the spur of the T without re-linking the bar across the junction
    t = np.zeros((8, 11), bool)
    t[1, 1:10] = t[1:4, 5] = True
    r3, r4 = rule.curves(t, 1)[0], rule.curves(t, 4)[0]
    assert r3.shape[0] == 3 and r4.shape[0] == 2 and np.all(r4[:, rule.POINTS] == 5)


def _from_bits(mask, min_length, **kw):
    h, w = mask.shape
    return capi.curves_from_bits(np.packbits(mask, axis=-1), h, w, min_length, **kw)


@pytest.mark.parametrize("min_length", MIN_LENGTHS)
@pytest.mark.parametrize("name", sorted(MAPS))
def test_curves_from_bits_equals_the_rule(name, min_length):
    mask = MAPS[name]
    w_rec, chains = rule.curves(mask, min_length)
    K, P = len(chains), sum(c.size for c in chains)
    w_chain = np.concatenate([[0], np.cumsum([c.size for c in chains])]).astype(np.uint64)
    w_points = np.concatenate(chains) if chains else np.zeros(0, np.int32)
    what = f"{name} min_length={min_length}"
    rec, chain, pts, k, p = _from_bits(mask, min_length)                       # sized by a counts-only call
    assert (k, p) == (K, P), f"{what}: counts"
    assert np.array_equal(rec, w_rec), f"{what}: records"
    assert np.array_equal(chain, w_chain), f"{what}: chain_offsets"
    assert pts.dtype == np.int32 and np.array_equal(pts, w_points), f"{what}: points"
    rec, chain, pts, k, p = _from_bits(mask, min_length, capacity=K, point_capacity=P)   # exact-size buffers
    assert (k, p) == (K, P) and np.array_equal(rec, w_rec) and np.array_equal(chain, w_chain)
    assert np.array_equal(pts, w_points), f"{what}: exact-size buffers"
    # halved capacities: the records that fit, a chain cut midway, the counts still true
    cap, pcap = K // 2, P // 2
    rec, chain, pts, k, p = _from_bits(mask, min_length, capacity=cap, point_capacity=pcap)
    assert (k, p) == (K, P), f"{what}: halved capacities change the counts"
    assert np.array_equal(rec, w_rec[:cap]) and np.array_equal(chain, w_chain[:cap + 1]), f"{what}: halved records"
    assert np.array_equal(pts, w_points[:min(pcap, int(w_chain[cap]))]), f"{what}: halved points"
    rec, chain, pts, k, p = _from_bits(mask, min_length, capacity=K, point_capacity=pcap)
    assert np.array_equal(rec, w_rec) and np.array_equal(pts, w_points[:pcap]), f"{what}: a chain cut midway"
    # counts only
    rec, chain, pts, k, p = _from_bits(mask, min_length, want_records=False, capacity=0, point_capacity=0)
    assert rec is None and chain.tolist() == [0] and pts.size == 0 and (k, p) == (K, P), f"{what}: counts only"


def test_curves_from_bits_writes_nothing_past_its_capacities_and_checks_its_arguments():
    import ctypes as C
    mask = MAPS["random_0.35_1"]
    h, w = mask.shape
    bits = np.packbits(mask, axis=-1)
    w_rec, chains = rule.curves(mask, 1)
    K, P = len(chains), sum(c.size for c in chains)
    L = capi.load()
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    for cap, pcap in ((K, P), (K // 2, P), (K, P // 3), (0, 0)):
        rec = np.full((cap + 8) * 4, 0x5A5A5A5A, np.int32)
        chain = np.full(cap + 1 + 8, 0xEEEEEEEEEEEEEEEE, np.uint64)
        pts = np.full(pcap + 8, 0x5A5A5A5A, np.int32)
        k, p = C.c_ulonglong(0), C.c_ulonglong(0)
        assert L.canny_hip_curves_from_bits(hp(bits), h, w, 1, hp(rec), cap, C.byref(k), hp(chain), hp(pts), pcap,
                                            C.byref(p)) == 0
        assert (k.value, p.value) == (K, P)
        assert np.all(rec[cap * 4:] == 0x5A5A5A5A) and np.all(chain[cap + 1:] == 0xEEEEEEEEEEEEEEEE)
        fit = int(np.cumsum([0] + [c.size for c in chains])[min(cap, K)])
        assert np.all(pts[min(pcap, fit):] == 0x5A5A5A5A), "points past a capacity"
    k, p = C.c_ulonglong(0), C.c_ulonglong(0)
    call = L.canny_hip_curves_from_bits
    assert call(None, h, w, 1, None, 0, C.byref(k), None, None, 0, C.byref(p)) == 1
    assert call(hp(bits), h, w, 1, None, 0, None, None, None, 0, C.byref(p)) == 1
    assert call(hp(bits), h, w, 1, None, 0, C.byref(k), None, None, 0, None) == 1
    assert call(hp(bits), h, w, 1, None, 4, C.byref(k), None, None, 0, C.byref(p)) == 1      # capacity without chain_offsets
    assert call(hp(bits), h, w, 1, None, 0, C.byref(k), None, None, 4, C.byref(p)) == 1      # point_capacity without points
    assert call(hp(bits), 0, w, 1, None, 0, C.byref(k), None, None, 0, C.byref(p)) == 1
    assert call(hp(bits), 1 << 15, (1 << 13) + 1, 1, None, 0, C.byref(k), None, None, 0, C.byref(p)) == 2   # > 2^28 pixels
    # the padding bits of a row are ignored
    padded = bits.copy()
    padded[:, -1] |= np.uint8((1 << (8 - w % 8)) - 1)
    got = capi.curves_from_bits(padded, h, w, 1)
    assert np.array_equal(got[0], w_rec) and got[3:] == (K, P)


@pytest.mark.parametrize("shape", [(37, 53), (120, 1001), (270, 480)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_oracles_maps_are_open_curves(shape):
    h, w = shape
    for seed in (1, 2, 3):
        mask = _oracle_map(h, w, seed)
        rule.check_invariants(mask)
        rec, chains = rule.curves(mask, 1)
        assert not (rec[:, rule.FLAGS] & (rule.CLOSED | rule.START_JUNCTION | rule.END_JUNCTION)).any(), \
            "synth_frame maps hold no junction and no closed curve"
        assert sum(c.size for c in chains) == int(mask.sum()), "so every pixel is listed exactly once"
        got = _from_bits(mask, 1)
        assert np.array_equal(got[0], rec) and np.array_equal(got[2], rule.csr([mask], 1)[3])


def test_curves_list_fewer_points_than_the_contour_chains():
    """The point of the feature: a contour chain walks a one-pixel curve out and back, a curve lists it once."""
    mask = _oracle_map(270, 480, 3)
    curve_points = sum(c.size for c in rule.curves(mask, 1)[1])
    contour_points = sum(c.size for c in contours_rule.contours(mask, 1)[1])
    print(f"270x480 seed 3: {int(mask.sum())} edge pixels, {curve_points} curve points, {contour_points} contour points")
    assert curve_points == int(mask.sum()) == 1032
    assert curve_points < contour_points


def test_abi_version_and_exports():
    assert capi.load().canny_hip_version() >= 1800
    for name in ("canny_hip_dev_canny_curves", "canny_hip_dev_curves_bits", "canny_hip_canny_curves",
                 "canny_hip_curves_from_bits", "canny_hip_curves_profile_get", "canny_hip_selftest_curves_plan"):
        assert name in capi.EXPORTS


# ---- the host rule under the host compiler's sanitizers -----------------------------------------------------------------
def test_host_rule_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_curves_host.cpp has its own main and is compiled together with csrc/canny_curves_host.cpp alone:
    nothing of it is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_curves_host"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_curves_host.cpp"),
                           os.path.join(ROOT, "canny_edge_amd", "csrc", "canny_curves_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_curves_host: ok" in r.stdout, r.stdout + r.stderr
