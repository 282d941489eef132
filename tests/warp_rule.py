"""The frame-alignment rules of include/canny_hip.h restated in numpy and plain Python ints: the chain of
the motion records (compose) and the warp of u8 frames by transform records (NEAREST and BILINEAR, constant border, valid
bits).  Written from the rule's text, independently of csrc/canny_warp_host.cpp and csrc/canny_warp.hip; the tests compare
both with this file byte for byte."""
import numpy as np

XFORM_WORDS, MOTION_WORDS = 8, 16
NEAREST, BILINEAR = 0, 1
LIM_A, LIM_T = 1 << 24, 1 << 36
ONE = 65536
IDENTITY = (ONE, 0, 0, 0, ONE, 0)


def record(coef, src=0, flags=1):
    """One transform record: flags, source frame, a11, a12, tx, a21, a22, ty (Q16)."""
    return np.array([flags, src, *coef], np.int64)


def within_limits(c):
    a11, a12, tx, a21, a22, ty = (int(v) for v in c)
    return all(abs(a) <= LIM_A for a in (a11, a12, a21, a22)) and abs(tx) <= LIM_T and abs(ty) <= LIM_T


def usable(rec, n_src):
    return bool(int(rec[0]) & 1) and within_limits(rec[2:8]) and 0 <= int(rec[1]) < n_src


def motion_record(coef, flags=3):
    """A 16-word motion record that carries the six coefficients in words 4..9."""
    m = np.zeros(MOTION_WORDS, np.int64)
    m[0] = flags
    m[4:10] = coef
    return m


def compose_pair(m, p):
    """M o T in Python ints: apply p (the chain so far) first, then m."""
    m11, m12, mtx, m21, m22, mty = (int(v) for v in m)
    p11, p12, ptx, p21, p22, pty = (int(v) for v in p)
    return ((m11 * p11 + m12 * p21) >> 16, (m11 * p12 + m12 * p22) >> 16, ((m11 * ptx + m12 * pty) >> 16) + mtx,
            (m21 * p11 + m22 * p21) >> 16, (m21 * p12 + m22 * p22) >> 16, ((m21 * ptx + m22 * pty) >> 16) + mty)


def compose(motion, first_frame=0):
    """int64 [n_pairs, 16] motion records of the pairs (f, f + 1) -> int64 [n_pairs + 1, 8] transform records."""
    motion = np.asarray(motion, np.int64).reshape(-1, MOTION_WORDS)
    out = np.zeros((len(motion) + 1, XFORM_WORDS), np.int64)
    out[:, 1] = first_frame + np.arange(len(motion) + 1)
    p, ok = IDENTITY, True
    out[0, 0], out[0, 2:] = 1, p
    for k, m in enumerate(motion):
        ok = ok and (int(m[0]) & 3) == 3 and within_limits(m[4:10])
        if ok:
            c = compose_pair(m[4:10], p)
            ok = within_limits(c)
            if ok:
                p = c
                out[k + 1, 0], out[k + 1, 2:] = 1, p
    return out


def warp(src, xforms, out_h, out_w, interp, border):
    """src uint8 [n_src, h, w], xforms int64 [n_out, 8] -> (uint8 [n_out, out_h, out_w], valid bit maps uint8
    [n_out, out_h, ceil(out_w / 8)], rows MSB-first with zero pad bits)."""
    src = np.asarray(src, np.uint8)
    n_src, sh, sw = src.shape
    xforms = np.asarray(xforms, np.int64).reshape(-1, XFORM_WORDS)
    out = np.full((len(xforms), out_h, out_w), border, np.uint8)
    valid = np.zeros((len(xforms), out_h, out_w), bool)
    y, x = np.mgrid[0:out_h, 0:out_w].astype(np.int64)
    for o, rec in enumerate(xforms):
        if not usable(rec, n_src):
            continue
        plane = src[int(rec[1])].astype(np.int64)
        a11, a12, tx, a21, a22, ty = (int(v) for v in rec[2:8])
        X, Y = a11 * x + a12 * y + tx, a21 * x + a22 * y + ty

        def tap(sy, sx):
            inside = (sx >= 0) & (sx < sw) & (sy >= 0) & (sy < sh)
            return np.where(inside, plane[np.clip(sy, 0, sh - 1), np.clip(sx, 0, sw - 1)], border), inside

        if interp == NEAREST:
            px, ok = tap((Y + 32768) >> 16, (X + 32768) >> 16)
        else:
            X8, Y8 = (X + 128) >> 8, (Y + 128) >> 8
            ix, fx, iy, fy = X8 >> 8, X8 & 255, Y8 >> 8, Y8 & 255
            (p00, i00), (p01, i01), (p10, i10), (p11, i11) = tap(iy, ix), tap(iy, ix + 1), tap(iy + 1, ix), tap(iy + 1, ix + 1)
            px = ((256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p01 + (256 - fx) * fy * p10 + fx * fy * p11 + 32768) >> 16
            ok = i00 & (i01 | (fx == 0)) & (i10 | (fy == 0)) & (i11 | (fx == 0) | (fy == 0))
        out[o], valid[o] = px.astype(np.uint8), ok
    return out, np.packbits(valid, axis=2)


def unpack_valid(bits, out_w):
    return np.unpackbits(bits, axis=-1)[..., :out_w].astype(bool)


# ---- transforms the tests share -----------------------------------------------------------------------------------------
def shift(dx, dy):
    """Output (x, y) reads the source at (x + dx, y + dy); dx, dy in pixels (fractions allowed: they are rounded to Q16)."""
    return (ONE, 0, int(round(dx * ONE)), 0, ONE, int(round(dy * ONE)))


def quarter_turn(w):
    """(x, y) -> (y, w - 1 - x): the relation of tests/test_descriptors_rule.py's turned view, R = np.rot90(A): an output of
    A's geometry read from R."""
    return (0, ONE, 0, -ONE, 0, (w - 1) * ONE)


def about_centre(a11, a12, a21, a22, cx, cy):
    """The linear part given in Q16, the translation chosen so that (cx, cy) stays where it is."""
    return (a11, a12, int(round(cx * ONE - a11 * cx - a12 * cy)), a21, a22, int(round(cy * ONE - a21 * cx - a22 * cy)))


def small_turn(w, h, degrees=1.0, scale=1.01):
    c, s = np.cos(np.radians(degrees)) * scale, np.sin(np.radians(degrees)) * scale
    return about_centre(int(round(c * ONE)), int(round(-s * ONE)), int(round(s * ONE)), int(round(c * ONE)),
                        (w - 1) / 2, (h - 1) / 2)
