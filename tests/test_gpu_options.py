"""The two registries of a context from outside: the int options and the workspace list.

The options that are a bounded store or load of one int member are answered from a table in the runtime (kOptions in
canny_capi.hip); the workspaces that canny_hip_selftest_workspace lists and canny_hip_ctx_destroy releases come from another
(kWorkspaces).  What is expected here was written down from the two `if` chains of canny_hip_ctx_get_option /
canny_hip_ctx_set_option and from collect_workspaces as they stood before the tables, not from the tables: a row that
drifts from the old behaviour fails here.  The process-wide names (tune_sobel_*, tune_plane_stores, gaussian_fma_div,
tune_finalize_mode, tune_gaussian_*) are not written: they would outlive the context."""
import pytest

pytestmark = pytest.mark.gpu

ERR_INVALID = 1

# name, min, max, readable, the value a fresh context holds (what a set-only name is put back to)
OPTIONS = [
    ("gaussian_path", 0, 2, True, 0),
    ("sobel_nms_path", 0, 2, True, 0),
    ("tune_sobel_seg", 0, 4096, False, 0),
    ("fuse_classify", 0, 1, True, 1),
    ("smoothed_u8", 0, 1, True, 1),
    ("gray_rule", 0, 1, True, 0),
    ("fuse_gray", 0, 1, True, 1),
    ("hysteresis_tail", 0, 1, True, 1),
    ("tune_hyst_tail_after", 1, 4, False, 2),
    ("overlap_hysteresis", 0, 1, False, 0),
    ("tune_batch_workers", 0, 16, False, 0),
    ("tune_batch_chunk_mb", 0, 1024, False, 0),
    ("tune_batch_chunk_frames", 0, 65535, False, 0),
    ("tune_batch_pipe_mode", 0, 2, False, 0),
    ("tune_batch_compact", 0, 1, True, 0),
    ("hough_path", 0, 2, True, 0),
    ("tune_hough_lds_kb", 0, 160, True, 0),
    ("chamfer_route", 0, 2, True, 0),
    ("warp_route", 0, 2, True, 0),
    ("fuse_route", 0, 2, True, 0),
    ("morph_route", 0, 2, True, 0),
    ("binarize_route", 0, 2, True, 0),
    ("thin_route", 0, 2, True, 0),
    ("thin_fuse", 0, 8, True, 0),
    ("tune_chamfer_chunk_mb", 0, 4096, True, 0),
]
READ_ONLY = ["last_canny_smoothed_u8", "last_canny_fused_gray", "batch_expand_threads"]

D, I, CACHE = 0, 1, 2
WORKSPACES = [
    ("tmp_f32", D), ("smoothed", D), ("edges16", D), ("gray", D), ("hist", D), ("thr", D), ("points", I),
    ("hough_accum", D), ("hough_ws", I), ("hough_tab", CACHE), ("cc_parent", I), ("cc_ws", I), ("ct_ws", I), ("pg_ws", I),
    ("pg_points", I), ("sh_ws", I), ("edt_cols", I), ("edt_stack", I), ("seg_ws", I), ("seg_lines", I), ("seg_work", D),
    ("circ_accum", D), ("circ_ws", I), ("circ_recs", I), ("chamfer_cost", D), ("chamfer_scores", D), ("chamfer_ws", I),
    ("chamfer_dist2", I), ("corners_ws", I), ("desc_ws", I), ("motion_ws", I), ("morph_ws", D), ("binarize_ws", D),
    ("thin_ws", D), ("plane_s", D), ("plane_c", D), ("stamps", I), ("flags", D), ("io0", I), ("io1", I), ("io2", I),
    ("io3", I),
]


def _set(hip, ctx, name, value):
    """The status of set_option, 0 for success."""
    try:
        ctx.set_option(name, value)
    except hip.CannyHipError as e:
        return e.status
    return 0


def _get(hip, ctx, name):
    """(status, value) of get_option."""
    try:
        return 0, ctx.get_option(name)
    except hip.CannyHipError as e:
        return e.status, None


def test_option_bounds_and_directions(hip):
    with hip.Context(0) as ctx:
        for name, lo, hi, readable, fresh in OPTIONS:
            st, before = _get(hip, ctx, name)
            if readable:
                assert (st, before) == (0, fresh), name
            else:
                assert st == ERR_INVALID, f"{name} can only be set"
            try:
                for good in (hi, lo):
                    assert _set(hip, ctx, name, good) == 0, (name, good)
                    if readable:
                        assert _get(hip, ctx, name) == (0, good), (name, good)
                assert _set(hip, ctx, name, hi) == 0, name
                bad = [hi + 1, -1] + ([lo - 1] if lo > 0 else [])
                for value in bad:
                    assert _set(hip, ctx, name, value) == ERR_INVALID, (name, value)
                    if readable:
                        assert _get(hip, ctx, name) == (0, hi), f"{name}: a rejected {value} changed the value"
            finally:
                assert _set(hip, ctx, name, fresh) == 0, name
            if readable:
                assert _get(hip, ctx, name) == (0, fresh), name


def test_read_only_and_unknown_names(hip):
    with hip.Context(0) as ctx:
        for name in READ_ONLY:
            assert _get(hip, ctx, name) == (0, 0), name   # a fresh context: no canny call yet, no expand pool
            for value in (0, 1):
                assert _set(hip, ctx, name, value) == ERR_INVALID, (name, value)
            assert _get(hip, ctx, name) == (0, 0), name
        for name in ("no_such_option", "", "gaussian_pat", "gaussian_path "):
            assert _set(hip, ctx, name, 0) == ERR_INVALID, name
            assert _get(hip, ctx, name)[0] == ERR_INVALID, name


def test_workspace_list_of_a_fresh_context(hip):
    with hip.Context(0) as ctx:
        listed = ctx.selftest_workspaces()
    assert [(name, kind) for name, _, _, kind in listed] == WORKSPACES
    assert all(ptr == 0 and size == 0 for _, ptr, size, _ in listed), "a fresh context owns no device memory"
