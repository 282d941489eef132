"""Thinning, host side: canny_hip_thin_bits (plain C++, no device) against tests/thin_rule.py byte for
byte, the two Python restatements against each other, the documented facts of the rule, the named mutants, the model of the
fused route (a halo of 2 F reproduces F global iterations, a halo of F does not), the demonstration scene through the curve
linker, the refused calls, the header and the bindings, and the host file under the host compiler's sanitizers."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import curves_rule
import thin_rule as R
from canny_edge_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_THICKNESSES = (1, 2, 3, 4, 5, 8, 9, 16)


def both(px, method, k=0):
    """The host C++ and the numpy rule on bool [n, h, w] (dirty pad bits in), compared; -> (unpacked output, info)."""
    px = np.asarray(px, bool)
    w = px.shape[-1]
    bits = R.pack_dirty(px, np.random.default_rng(px.size))
    want, want_info = R.thin(bits, w, method, k)
    got, info = capi.thin_bits(bits, w, method, k)
    assert np.array_equal(got, want), f"method {method} k {k}: the host's bytes differ from the rule"
    assert np.array_equal(info, want_info), (method, k, info.tolist(), want_info.tolist())
    return R.unpack(got, w), info


def designed_maps():
    yy, xx = np.mgrid[:20, :27]
    return {
        "scene": R.demo_scene(), "square2": R.square2(), "diagonal2": R.diagonal2(), "allset": np.ones((33, 47), bool),
        "empty": np.zeros((5, 9), bool), "checker": ((yy + xx) & 1).astype(bool), "bar_at_border": R.bar(9, 30, 0, 4),
        "one_pixel": np.ones((1, 1), bool), "one_row": np.ones((1, 13), bool), "one_column": np.ones((11, 1), bool),
        "blobs": R.blobs(50, 61, 3),
    }


# ---- the two restatements and the host ------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", R.METHODS)
def test_both_restatements_and_the_host_agree_on_tiny_maps(method):
    rng = np.random.default_rng(37 + method)
    maps = [R.square2(), R.diagonal2(6, 1), np.ones((5, 7), bool), np.ones((1, 1), bool), np.zeros((3, 4), bool)]
    maps += [rng.random((int(rng.integers(1, 12)), int(rng.integers(1, 14)))) < d for d in (0.3, 0.5, 0.7, 0.9) for _ in range(3)]
    maps += [R.blobs(12, 14, s, 3) for s in range(3)]
    for a, k in itertools.product(maps, (0, 1, 2)):
        out, it, conv = R.thin_px(a, method, k)
        out2, it2, conv2 = R.thin_loop(a, method, k)
        assert np.array_equal(out, out2) and (it, conv) == (it2, conv2)
        got, info = both(a[None], method, k)
        assert np.array_equal(got[0], out) and info[0].tolist() == [out.sum(), it, a.sum() - out.sum(), conv]


# ---- the documented facts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("t", BAR_THICKNESSES)
def test_a_bar_of_thickness_t_takes_t_half_iterations_and_leaves_one_row(method, t):
    out, info = both(R.bar(t + 8, 40, 4, t)[None], method)
    assert info[0, 1] == t // 2 and info[0, 3] == 1
    assert out[0].any(axis=1).sum() == 1


@pytest.mark.parametrize("method", R.METHODS)
def test_an_all_set_33_by_47_frame_takes_16_iterations(method):
    assert both(np.ones((1, 33, 47), bool), method)[1][0, 1] == 16


def test_zhangsuen_erases_the_square_and_guohall_keeps_components():
    assert both(R.square2()[None], R.ZHANGSUEN)[0].sum() == 0
    assert both(R.square2()[None], R.GUOHALL)[0].sum() == 1
    d = R.diagonal2()
    assert d.sum() == 23
    assert both(d[None], R.ZHANGSUEN)[0].sum() == 1
    assert both(d[None], R.GUOHALL)[0].sum() == 13


def test_guohall_keeps_the_components_of_sixty_blob_maps():
    maps = np.stack([R.blobs(50, 61, seed) for seed in range(60)])
    out, _ = both(maps, R.GUOHALL)
    for a, o in zip(maps, out):
        assert R.components8(a) == R.components8(o)


@pytest.mark.parametrize("method", R.METHODS)
def test_the_output_is_a_subset_of_the_input_and_idempotent(method):
    maps = list(designed_maps().values()) + [np.random.default_rng(s).random((23, 37)) < (0.2 + 0.04 * s) for s in range(18)]
    for a in maps:
        out, info = both(a[None], method)
        assert not (out[0] & ~a).any()
        again, info2 = both(out, method)
        assert np.array_equal(again, out) and info2[0].tolist() == [out.sum(), 0, 0, 1]
        cut, info_cut = both(a[None], method, max(1, int(info[0, 1])))   # a run cut at exactly D proves nothing
        assert np.array_equal(cut, out) and info_cut[0, 3] == (1 if info[0, 1] == 0 else 0)


def test_max_iterations_cuts_the_run():
    a = R.bar(30, 40, 5, 16)
    for method in R.METHODS:
        d = 8
        for k, want_it, want_conv in ((1, 1, 0), (d - 1, d - 1, 0), (d, d, 0), (d + 1, d, 1), (0, d, 1), (16384, d, 1)):
            out, info = both(a[None], method, k)
            assert info[0, 1] == want_it and info[0, 3] == want_conv
            assert (out[0].any(axis=1).sum() == 1) == (want_it == d)


# ---- the mutants ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant,method,name", [
    ("swapped_subs", R.ZHANGSUEN, "scene"), ("swapped_subs", R.GUOHALL, "square2"), ("b_le_7", R.ZHANGSUEN, "blobs"),
    ("no_wrap", R.ZHANGSUEN, "diagonal2"), ("replicate", R.ZHANGSUEN, "bar_at_border"), ("replicate", R.GUOHALL, "allset"),
    ("gh_max", R.GUOHALL, "diagonal2")])
def test_every_mutant_changes_a_named_map(mutant, method, name):
    assert mutant in R.MUTANTS
    a = designed_maps()[name]
    assert not np.array_equal(R.thin_px(a, method, 0, mutant)[0], R.thin_px(a, method)[0])


# ---- the fused route's model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("fuse", (1, 2, 8))
def test_tiles_with_a_halo_of_2f_reproduce_f_global_iterations(method, fuse):
    for seed in range(3):
        a = R.blobs(50, 61, seed)
        for k in (0, 3):
            want = R.thin_px(a, method, k)
            got = R.fused_model(a, method, k, (16, 16), fuse)
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (seed, k)


@pytest.mark.parametrize("method", R.METHODS)
def test_a_smaller_halo_does_not(method):
    a = R.blobs(50, 61, 0)
    want = R.thin_px(a, method)[0]
    assert not np.array_equal(R.fused_model(a, method, 0, (16, 16), 2, halo=2)[0], want), "a halo of F"
    assert not np.array_equal(R.fused_model(a, method, 0, (16, 16), 1, halo=1)[0], want), "a halo of 2 F - 1 at F = 1"


# ---- pad bits -------------------------------------------------------------------------------------------------------------
def test_pad_bits_are_ignored_on_input_and_zero_on_output():
    for w in (1, 7, 9, 13, 61):
        a = R.blobs(20, w, w) if w > 5 else np.ones((20, w), bool)
        clean, dirty = R.pack(a[None]), R.pack_dirty(a[None])
        assert w % 8 == 0 or not np.array_equal(clean, dirty)
        for method in R.METHODS:
            out_c, info_c = capi.thin_bits(clean, w, method)
            out_d, info_d = capi.thin_bits(dirty, w, method)
            assert np.array_equal(out_c, out_d) and np.array_equal(info_c, info_d)
            assert np.array_equal(R.pack(R.unpack(out_d, w)), out_d), "pad bits of the output"
            assert info_d[0, 2] == a.sum() - info_d[0, 0], "deleted counts pixels inside the frame only"


# ---- the demonstration scene ----------------------------------------------------------------------------------------------
def test_the_demonstration_scene_links_into_two_curves():
    s = R.demo_scene()
    assert s.shape == (96, 160) and s.sum() == 1735
    assert curves_rule.curves(s)[0].shape[0] == 3078
    for method, iterations, left, lengths in ((R.GUOHALL, 5, 203, {(148, 1), (55, 0)}), (R.ZHANGSUEN, 4, 218, {(164, 1), (54, 0)})):
        out, info = both(s[None], method)
        assert info[0].tolist() == [left, iterations, 1735 - left, 1]
        records, _ = curves_rule.curves(out[0])
        assert {(int(r[curves_rule.POINTS]), int(r[curves_rule.FLAGS]) & curves_rule.CLOSED) for r in records} == lengths
        assert records.shape[0] == 2


# ---- refused calls --------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing_and_info_may_be_null():
    L = capi.load()
    n, h, w, rb = 2, 6, 9, 2
    a = R.pack(np.random.default_rng(3).random((n, h, w)) < 0.6)
    vp = capi.C.c_void_p
    n_out = n * h * rb
    S8 = 0x5A5A5A5A5A5A5A5A

    def call(src=1, n=n, h=h, w=w, method=R.GUOHALL, k=0, out=1, info=1, off=0):
        o, inf = np.full(n_out + 8, 0x5A, np.uint8), np.full(4 * 2 + 4, S8, np.int64)
        st = L.canny_hip_thin_bits(capi._hp(a) if src else None, n, h, w, method, k, capi._hp(o) if out else None,
                                   vp(inf.ctypes.data + off) if info else None)
        if st:
            assert (o == 0x5A).all() and (inf == S8).all(), "a refused call wrote something"
        else:
            assert (o[n_out:] == 0x5A).all() and (inf[8:] == S8).all() and (info or (inf == S8).all())
        return st

    assert call() == 0 and call(info=0) == 0 and call(method=R.ZHANGSUEN, k=16384) == 0 and call(k=1) == 0
    for kw in (dict(src=0), dict(out=0), dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(method=-1), dict(method=2), dict(k=-1),
               dict(k=16385), dict(off=4), dict(off=1)):
        assert call(**kw) == 1, kw
    for kw in (dict(h=32769), dict(w=32769), dict(n=65536), dict(h=32768, w=32768 * 2)):
        assert call(**kw) == 2, kw
    # buffers that overlap: maps 24 B, info 64 B
    buf = np.full(400, 0x5A, np.uint8)
    at = lambda o: vp(buf.ctypes.data + o)
    for i_at, o_at, f_at in ((0, 0, 200), (0, 23, 200), (10, 0, 200), (0, 100, 16), (0, 100, 120), (0, 100, 96), (0, 100, 40)):
        st = L.canny_hip_thin_bits(at(i_at), n, h, w, R.GUOHALL, 0, at(o_at), at(f_at))
        assert st == 1 and (buf == 0x5A).all(), (i_at, o_at, f_at)
    assert L.canny_hip_thin_bits(at(0), n, h, w, R.GUOHALL, 0, at(24), at(48)) == 0 and (buf[112:] == 0x5A).all()


# ---- header and bindings --------------------------------------------------------------------------------------------------
def test_header_describes_the_feature():
    header = open(os.path.join(ROOT, "include", "canny_hip.h")).read()
    assert int(re.search(r"#define CANNY_HIP_VERSION (\d+)", header).group(1)) >= 2600
    assert capi.load().canny_hip_version() >= 2600
    for word in ("0.26.0: + thinning of packed bit maps", "0.25.0: + binarization", "0.24.0: + binary morphology on packed bit maps",
                 "THE PAD BITS OF THE INPUT ARE IGNORED", "EVERYTHING OUTSIDE THE FRAME READS 0", "P9 = (y-1, x-1)",
                 "P2 P4 P6 = 0 and P4 P6 P8 = 0", "P2 P4 P8 = 0 and P2 P6 P8 = 0", "2 <= min(N1, N2) <= 3",
                 "m = (P6 | P7 | !P9) & P8", "m = (P2 | P3 | !P5) & P4", "ZHANGSUEN DOES NOT PRESERVE COMPONENTS",
                 "\"thin_route\"", "\"thin_fuse\"", "SYNCHRONISES THE STREAM", "no in-place form",
                 "CANNY_HIP_THIN_MAX_ITERATIONS %d" % capi.THIN_MAX_ITERATIONS, "hit-or-miss", "spur pruning", "medial-axis radii",
                 "grey-level thinning"):
        assert word in header, word
    morph_follow_ups = re.search(r"Not covered -- follow-ups: grey-level morphology.*?\*/", header, re.S).group(0)
    assert "hit-or-miss" in morph_follow_ups and "and thinning" not in morph_follow_ups
    for name in ("canny_hip_dev_thin_bits", "canny_hip_dev_canny_thin", "canny_hip_thin_batch", "canny_hip_thin_bits",
                 "canny_hip_selftest_thin_plan"):
        assert name in capi.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
        getattr(capi.load(), name)
    assert "canny_hip_thin_profile_get" not in capi.EXPORTS and "canny_hip_thin_profile_get" not in header
    for method in ("dev_thin_bits", "dev_canny_thin", "thin_batch"):
        assert hasattr(capi.Context, method), method
    assert callable(capi.thin_bits) and callable(capi.thin_plan)
    assert (capi.THIN_ZHANGSUEN, capi.THIN_GUOHALL) == R.METHODS == (0, 1) and capi.THIN_MAX_ITERATIONS == R.MAX_ITERATIONS
    assert (capi.THIN_ROUTE_AUTO, capi.THIN_ROUTE_STEPWISE, capi.THIN_ROUTE_FUSED) == (0, 1, 2)
    for i, m in enumerate(("ZHANGSUEN", "GUOHALL")):
        assert re.search(rf"CANNY_HIP_THIN_{m} = {i}\b", header), m
    for i, part in enumerate(capi.THIN_PARTS):
        assert re.search(rf"CANNY_HIP_THIN_PART_{part.upper()} = {i}\b", header), part
    assert re.search(r"CANNY_HIP_THIN_PARTS = 2\b", header) and len(capi.THIN_PARTS) == 2


def test_the_profile_parts_are_refused_before_the_device_is_touched():
    fn = capi.load().canny_hip_profile_part_get
    D, Lg = capi.C.c_double, capi.C.c_long
    for part in (0, 1, 2, -1):
        ms, n = D(-1.0), Lg(-1)
        assert fn(None, b"thin", part, capi.C.byref(ms), capi.C.byref(n)) == 1 and (ms.value, n.value) == (-1.0, -1)


# ---- the host rule under the host compiler's sanitizers -------------------------------------------------------------------
def test_host_rule_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/test_thin_host.cpp has its own main and is compiled together with csrc/canny_thin_host.cpp alone: nothing of it
    is loaded into this interpreter, and no device is involved."""
    exe = tmp_path / "test_thin_host"
    csrc = os.path.join(ROOT, "canny_edge_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                           os.path.join(ROOT, "tests", "cpp", "test_thin_host.cpp"),
                           os.path.join(csrc, "canny_thin_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "thin ok" in r.stdout, r.stdout + r.stderr


def test_the_bit_sliced_sub_iteration_of_the_kernels_equals_the_per_pixel_rule(tmp_path):
    """csrc/canny_thin_words.h is what the kernels of canny_thin.hip run per 64-bit word; it is plain C++ apart from its
    qualifiers, so tests/cpp/test_thin_words.cpp (own main) runs it on the host over all 512 neighbourhoods at every bit
    position and over random words, both methods, both sub-iterations."""
    exe = tmp_path / "test_thin_words"
    csrc = os.path.join(ROOT, "canny_edge_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(ROOT, "tests", "cpp", "test_thin_words.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "thin words ok" in r.stdout, r.stdout + r.stderr
