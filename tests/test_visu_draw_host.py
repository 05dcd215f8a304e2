"""tests/visu_draw_ref.py -- the definition of the vector primitives -- held to what it restates: PIL.ImageDraw on RGB images, and
matplotlib for the colour table of plot_graph_result.  "Equals PIL" is the definition: every comparison is zero differing pixels.
Also the parts of the draw path that need no GPU: the closed forms the kernel uses against the loop forms, and the argument checks of
the C entry point and of ops.draw."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest
import torch

import visu_draw_ref as DR
from wild_visual_navigation_amd import _lib, ops
from wild_visual_navigation_amd.visu.colormaps import graph_result_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((64, 48), (53, 37))   # (W, H)
COL = (10, 200, 30)


def _pil(W, H):
    Image = pytest.importorskip("PIL.Image")
    ImageDraw = pytest.importorskip("PIL.ImageDraw")
    im = Image.new("RGB", (W, H))
    return im, ImageDraw.Draw(im)


def _ref(W, H, kind, pts):
    canvas = np.zeros((1, H, W, 3), np.uint8)
    n = len(pts)
    skipped = DR.draw(canvas, [kind] * n, np.asarray(pts, np.float32).reshape(n, 4), [COL] * n, [0] * n, [0] * n, W)
    assert skipped == 0
    return canvas[0]


def _special_segments(W, H, rng):
    """Zero-length, exactly horizontal and vertical segments (inside, across and outside the borders), slopes of exactly 1 and 1/2."""
    out = []
    for _ in range(300):
        x, y = rng.randint(-6, W + 5), rng.randint(-6, H + 5)
        f = rng.random()
        out += [(x, y, x, y), (x + f, y + f, x + f, y + f), (x, y, rng.randint(-6, W + 5), y), (x, y, x, rng.randint(-6, H + 5)),
                (x, y + f, rng.uniform(-16, W + 16), y + f * 0.5), (x + f, y, x + f * 0.5, rng.uniform(-16, H + 16))]
        d = rng.randint(-20, 20)
        out += [(x, y, x + d, y + d), (x, y, x + d, y - d), (x, y, x + 2 * d, y + d), (x, y, x + d, y - 2 * d)]
    return out


@pytest.mark.parametrize("kind, width", [(DR.LINE, 1), (DR.LINE, 0), (DR.LINE2, 2)])
def test_lines_equal_pil(kind, width):
    rng = random.Random(20 + width)
    total = 0
    for W, H in SIZES:
        segs = [tuple(rng.uniform(-16, s + 16) for s in (W, H, W, H)) for _ in range(2600)] + _special_segments(W, H, rng)
        total += len(segs)
        for seg in segs:
            seg = tuple(float(np.float32(c)) for c in seg)   # what a record can hold
            im, dr = _pil(W, H)
            dr.line(list(seg), fill=COL, width=width)
            want, got = np.array(im), _ref(W, H, kind, [seg])
            assert np.array_equal(want, got), (seg, int((want != got).any(2).sum()))
    assert total >= 5000


def test_lines_are_drawn_from_truncated_coordinates():
    """A float segment draws exactly what its truncation toward zero draws (both widths), for negative coordinates as well."""
    rng = random.Random(3)
    W, H = SIZES[1]
    for _ in range(500):
        seg = [rng.uniform(-16, s + 16) for s in (W, H, W, H)]
        for width in (1, 2):
            a, da = _pil(W, H)
            b, db = _pil(W, H)
            da.line(seg, fill=COL, width=width)
            db.line([float(math.trunc(c)) for c in seg], fill=COL, width=width)
            assert np.array_equal(np.array(a), np.array(b)), seg


def _centres(W, H, rng):
    out = [(rng.uniform(-16, W + 16), rng.uniform(-16, H + 16)) for _ in range(1500)]
    for _ in range(150):   # within 5 of each border, below 5 (the 9-wide boxes), exactly on integers and halves
        t = rng.uniform(-16, max(W, H) + 16)
        out += [(rng.uniform(-6, 6), t), (rng.uniform(W - 7, W + 6), t), (t, rng.uniform(-6, 6)), (t, rng.uniform(H - 7, H + 6)),
                (rng.uniform(0, 5), rng.uniform(0, 5)), (float(rng.randint(-8, W + 8)), rng.randint(-8, H + 8) + 0.5)]
    out += [(1e-10, 1e-10), (1e-10, 20.0), (20.0, -1e-10), (5.0, 5.0), (4.9999995, 5.0000005), (-1e-10, 5 + 1e-6), (W - 1e-4, H - 1e-4)]
    return out


def test_discs_equal_pil():
    rng = random.Random(7)
    total = 0
    for W, H in SIZES:
        cs = _centres(W, H, rng)
        total += len(cs)
        for k, (cx, cy) in enumerate(cs):
            cx, cy = np.float32(cx), np.float32(cy)   # the centres are fp32, as center[i].tolist() of a float tensor gives them
            im, dr = _pil(W, H)
            params = [float(cx), float(cy)]
            dr.ellipse([p - 5 for p in params] + [p + 5 for p in params], width=(10, 1)[k % 2], fill=COL)
            want, got = np.array(im), _ref(W, H, DR.DISC, [(cx, cy, 0, 0)])
            assert np.array_equal(want, got), ((cx, cy), int((want != got).any(2).sum()))
    assert total >= 3000


def test_an_fp32_subtraction_would_move_the_box():
    """c - 5 is a double on the fp32 centre: for c = 1e-10 the box starts at (int)(-4.9999999999) = -4; fp32 gives -5.0 -> -5."""
    c = np.float32(1e-10)
    assert math.trunc(float(c) - 5) == -4 and math.trunc(float(np.float32(c - np.float32(5)))) == -5
    assert [DR.truncate(v) for v in DR.disc_box(c, c)] == [-4, -4, 5, 5]


def test_painters_order_panel_clip_and_skip_rule():
    """The statement's own bookkeeping: later primitives overrule earlier ones, a primitive stays inside its panel, and a primitive
    with a bad coordinate, frame or panel is skipped, counted and changes nothing."""
    W, H = 40, 30
    canvas = np.zeros((2, H, 2 * W, 3), np.uint8)
    kinds = [DR.DISC, DR.DISC, DR.LINE, DR.LINE2, DR.DISC, DR.LINE, DR.LINE, 7, DR.LINE, DR.DISC]
    pts = [(W - 2, 10, 0, 0), (W - 2, 12, 0, 0), (-5, 3, W + 5, 3), (0, 0, float("nan"), 3), (float("inf"), 1, 0, 0), (0, 0, 1e12, 5),
           (0, 0, 5, 5), (0, 0, 5, 5), (0, 0, 5, 5), (10, 32768 + 5, 0, 0)]
    cols = [(i + 1, 0, 0) for i in range(len(kinds))]
    frame = [0, 0, 1, 0, 0, 0, 2, 0, 0, 0]
    panel = [0, 0, 1, 0, 0, 0, 0, 0, 2, 0]
    assert DR.draw(canvas, kinds, np.asarray(pts, np.float32), cols, frame, panel, W) == 7
    assert (canvas[0, :, W:] == 0).all() and (canvas[1, :, :W] == 0).all()           # nothing bleeds into the neighbouring panel
    assert canvas[0, 11, W - 2, 0] == 2 and canvas[0, 6, W - 2, 0] == 1               # the later disc wins where both cover
    assert (canvas[1, 3, W:, 0] == 3).all() and (canvas[1, :3] == 0).all() and (canvas[1, 4:] == 0).all()
    assert set(np.unique(canvas[..., 0])) == {0, 1, 2, 3}
    # a double that does not fit an fp32 record travels as its truncation
    assert DR._pretruncate(100.99999994) == 100.0 and np.float32(100.99999994) == 101.0 and math.isnan(DR._pretruncate(float("nan")))


def test_closed_forms_equal_the_loops():
    """csrc/draw.hip tests a pixel in closed form: Bresenham's minor coordinate after i major steps, and the integer form of the
    2-pixel line's offsets.  Every (dx, dy) with both <= 64 in all four sign pairs, against the loop and against hypot."""
    for dx in range(65):
        for dy in range(65):
            for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                x1, y1 = 70 + sx * dx, 70 + sy * dy
                painted = set(DR.thin_line_pixels(70, 70, x1, y1))
                lo_x, hi_x, lo_y, hi_y = min(70, x1) - 1, max(70, x1) + 1, min(70, y1) - 1, max(70, y1) + 1
                covered = {(x, y) for x in range(lo_x, hi_x + 1) for y in range(lo_y, hi_y + 1) if DR.thin_line_covers(x, y, 70, 70, x1, y1)}
                assert painted == covered, (dx, dy, sx, sy)
                if dx or dy:
                    assert DR.wide_line_offsets(sx * dx, sy * dy) == DR.wide_line_offsets_integer(sx * dx, sy * dy), (dx, dy, sx, sy)
    rng = random.Random(5)
    for _ in range(20000):   # the whole coordinate range, and vectors close to the 30 / 60 degree thresholds
        dx, dy = rng.randint(-65535, 65535), rng.randint(-65535, 65535)
        if rng.random() < 0.5:
            dy = int(round(dx * math.sqrt(3) ** rng.choice((-1, 1)))) + rng.randint(-1, 1)
        if (dx or dy) and abs(dx) <= 65535 and abs(dy) <= 65535:
            assert DR.wide_line_offsets(dx, dy) == DR.wide_line_offsets_integer(dx, dy), (dx, dy)
    for major in (1, 2, 3, 1000, 32767, 32768, 65535):   # the 32-bit and 64-bit branches of the kernel's division
        for minor in {0, 1, major // 2, major - 1, major}:
            e, c = 2 * minor - major, 0
            for i in range(min(major, 3000) + 1):
                assert DR.bresenham_minor(minor, major, i) == c
                if e >= 0:
                    c += 1
                    e -= 2 * major
                e += 2 * minor


def test_graph_result_table_is_the_matplotlib_construction():
    pytest.importorskip("matplotlib")
    want = DR.graph_result_table("RdYlBu")
    assert want.shape == (256, 3) and want.dtype == np.uint8
    assert np.array_equal(graph_result_table("RdYlBu").numpy(), want)                      # the packaged file
    assert np.array_equal(graph_result_table("viridis").numpy(), DR.graph_result_table("viridis"))   # any other name: matplotlib
    with pytest.raises(_lib.WvnError, match="matplotlib does not know"):
        graph_result_table("no_such_colour_map")


def test_method_lists_follow_the_reference_arithmetic():
    """plot_optical_flow: u, v over int(k * s); the far end is (v + fp32(flow[1] + W), u + flow[0]) summed in double."""
    flow = np.zeros((2, 23, 31), np.float32)
    # 1 - 2^-24: fp32(flow[1] + 31) is 32.0 (a double sum would truncate to 31); 4 + flow[0] is 4.99999994 in double -> 4 (fp32: 5.0)
    flow[0, 4, 8], flow[1, 4, 8] = 0.99999994, 0.99999994
    kinds, pts, cols, frame, panel = DR.optical_flow_list(flow, s=4)
    assert len(kinds) == int(23 / 4) * int(31 / 4) and (kinds == DR.LINE2).all() and (cols == (0, 255, 0)).all()
    i = 1 * int(31 / 4) + 2
    assert pts[i].tolist() == [8.0, 4.0, 40.0, 4.0]
    assert pts[0].tolist() == [0.0, 0.0, 31.0, 0.0]
    k2 = DR.sparse_optical_flow_list([[1.25, 2.5]], [[0.75, 7.0]], 31)[1]
    assert k2[0].tolist() == [1.25, 2.5, 31.75, 7.0]
    k, p, c, _, pan = DR.graph_result_list(np.array([[0, 1], [1, 1]]), [[3.5, 4.5], [9, 9]], [0.0, 1.0], [2.0, -1.0],
                                           DR.graph_result_table() if _has_matplotlib() else np.arange(768).reshape(256, 3) % 256, use_seg=True)
    assert k.tolist() == [DR.LINE, DR.LINE, DR.DISC, DR.DISC] * 3 and pan.tolist() == [0] * 4 + [1] * 4 + [2] * 4
    assert p[0].tolist() == [3.5, 4.5, 9.0, 9.0] and p[1].tolist() == [9.0, 9.0, 9.0, 9.0] and (c[:2] == (255, 0, 0)).all()
    assert (c[2] == c[7]).all() and (c[3] == c[6]).all()          # prediction clipped to 1 and 0: the colours of y = 1 and y = 0


def _has_matplotlib():
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return False
    return True


# ---- the C entry point and ops.draw without a GPU -------------------------------------------------------------------------------------
def _desc(**kw):
    words = (C.c_longlong * 8)()
    p = C.addressof(words)   # (never dereferenced: every call below is refused before a launch)
    d = _lib.DrawDesc()
    d.canvas = d.kinds = d.points = d.colours = d.frame = d.panel = p
    d.B, d.H, d.P, d.Wp, d.N = 2, 8, 2, 8, 4
    d.row_bytes, d.frame_bytes = 48, 384
    for k, v in kw.items():
        setattr(d, k, v)
    return d, words


def test_c_entry_point_refuses_bad_arguments_before_any_launch():
    h = _lib.lib()
    assert "wvn_draw" in _lib.EXPORTED_SYMBOLS and hasattr(h, "wvn_draw")
    bad = [dict(canvas=None), dict(kinds=None), dict(points=None), dict(colours=None), dict(frame=None), dict(panel=None), dict(N=-1),
           dict(N=_lib.DRAW_MAX_PRIMITIVES + 1), dict(B=0), dict(B=65536), dict(P=0), dict(P=6), dict(H=0), dict(Wp=0), dict(row_bytes=47),
           dict(frame_bytes=383), dict(frame_bytes=-1), dict(Wp=1 << 30)]
    for kw in bad:
        d, words = _desc(**kw)
        assert h.wvn_draw(C.byref(d), None) == _lib.ERR_ARG, kw
        assert all(w == 0 for w in words)
    assert h.wvn_draw(None, None) == _lib.ERR_ARG
    d, _ = _desc(N=0, kinds=None, points=None, colours=None, frame=None, panel=None)
    assert h.wvn_draw(C.byref(d), None) == 0                       # an empty list: nothing to launch
    assert C.sizeof(_lib.DrawDesc) == 7 * 8 + 2 * 8 + 5 * 4 + 4
    with open(os.path.join(ROOT, "include", "wvn_hip.h")) as f:
        hdr = f.read()
    for name, val in (("WVN_DRAW_MAX_PRIMITIVES", _lib.DRAW_MAX_PRIMITIVES), ("WVN_DRAW_LINE", _lib.DRAW_LINE),
                      ("WVN_DRAW_LINE2", _lib.DRAW_LINE2), ("WVN_DRAW_DISC", _lib.DRAW_DISC)):
        assert f"#define {name} {val}\n" in hdr
    assert (DR.LINE, DR.LINE2, DR.DISC) == (_lib.DRAW_LINE, _lib.DRAW_LINE2, _lib.DRAW_DISC)


def test_ops_draw_refuses_cpu_tensors():
    with pytest.raises(_lib.WvnError, match="GPU"):                # no CPU fallback
        ops.draw(torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 4),
                 torch.zeros(1, 3, dtype=torch.uint8))
