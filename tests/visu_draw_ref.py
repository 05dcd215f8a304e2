"""The vector primitives of wild_visual_navigation_amd (csrc/draw.hip, ops.draw, the graph and flow views of visu/) stated in plain
Python and numpy: what PIL.ImageDraw draws for ``line(width=1)``, ``line(width=2)`` and ``ellipse`` on the box of +-5, the painter's
order, the panel clip, the skip rule, and the primitive lists of plot_traversability_graph, plot_graph_result, plot_optical_flow and
plot_sparse_optical_flow of the reference (visu/visualizer.py:251-309, :425-484, :541-613).  No PIL import: tests/test_visu_draw_host.py
holds this file to PIL itself, tests/test_gpu_visu_draw.py holds the kernel to this file.

Pillow's rules, as src/libImaging/Draw.c and src/_imaging.c state them and test_visu_draw_host.py confirms on Pillow 12.2:
  * every coordinate is a double truncated toward zero by a C ``(int)`` cast;
  * a thin line is line8 / line32's Bresenham over n = max(|dx|, |dy|) pixels from the FIRST end, then the last point on its own;
  * a line of width 2 is polygon_generic on four integer vertices, edge slopes held as C floats;
  * a filled ellipse depends only on its truncated box."""
import math

import numpy as np

LINE, LINE2, DISC = 0, 1, 2
COORD_MIN, COORD_MAX = -32768, 32767
f32 = np.float32


# ---- the three primitives as loops: each returns the list of (x, y) it paints, unclipped --------------------------------------
def thin_line_pixels(x0, y0, x1, y1):
    """line8 of Draw.c, plus the last point ImageDraw.line adds (``draw last point``)."""
    px = []
    last = (x1, y1)
    dx, dy = x1 - x0, y1 - y0
    xs = -1 if dx < 0 else 1
    ys = -1 if dy < 0 else 1
    dx, dy = abs(dx), abs(dy)
    if dx == 0:
        for _ in range(dy):
            px.append((x0, y0))
            y0 += ys
    elif dy == 0:
        lo, hi = min(x0, x1), max(x0, x1)
        px += [(x, y0) for x in range(lo, hi + 1)]
    elif dx > dy:
        n = dx
        dy += dy
        e = dy - dx
        dx += dx
        for _ in range(n):
            px.append((x0, y0))
            if e >= 0:
                y0 += ys
                e -= dx
            e += dy
            x0 += xs
    else:
        n = dy
        dx += dx
        e = dx - dy
        dy += dy
        for _ in range(n):
            px.append((x0, y0))
            if e >= 0:
                x0 += xs
                e -= dy
            e += dx
            y0 += ys
    px.append(last)
    return px


def bresenham_minor(minor, major, i):
    """The closed form the kernel uses: minor-axis steps after i major steps = floor(minor * i / major + 1/2)."""
    return (2 * minor * i + major) // (2 * major)


def thin_line_covers(x, y, x0, y0, x1, y1):
    """dr_cover_thin of csrc/draw.hip."""
    dx, dy = x1 - x0, y1 - y0
    xs = -1 if dx < 0 else 1
    ys = -1 if dy < 0 else 1
    dx, dy = abs(dx), abs(dy)
    if dx > dy:
        i = (x - x0) * xs
        return 0 <= i <= dx and y == y0 + ys * bresenham_minor(dy, dx, i)
    i = (y - y0) * ys
    return 0 <= i <= dy and x == x0 + (0 if dy == 0 else xs * bresenham_minor(dx, dy, i))


def round_up(f):
    """ROUND_UP of Draw.c on a C float: half away from zero, symmetric about zero."""
    f = f32(f)
    return int(math.floor(f32(f + f32(0.5)))) if f >= 0 else -int(math.floor(f32(abs(f) + f32(0.5))))


def round_down(f):
    """ROUND_DOWN of Draw.c on a C float: half toward zero, symmetric about zero."""
    f = f32(f)
    return int(math.ceil(f32(f - f32(0.5)))) if f >= 0 else -int(math.ceil(f32(abs(f) - f32(0.5))))


def wide_line_offsets(dx, dy):
    """ImagingDrawWideLine at width 2: (ex, ey) = (ROUND_DOWN(dy / hypot), ROUND_DOWN(dx / hypot)), in doubles."""
    ratio = 1.0 / math.hypot(dx, dy)

    def rd(v):
        return int(math.ceil(v - 0.5)) if v >= 0 else -int(math.ceil(abs(v) - 0.5))

    return rd(ratio * dy), rd(ratio * dx)


def wide_line_offsets_integer(dx, dy):
    """The form the kernel uses: |dy| / hypot > 1/2 <=> 3 dy^2 > dx^2 (no tie for integers)."""
    sign = lambda v: (v > 0) - (v < 0)   # noqa: E731
    return (sign(dy) if 3 * dy * dy > dx * dx else 0), (sign(dx) if 3 * dx * dx > dy * dy else 0)


def wide_line_spans(x0, y0, x1, y1, rows):
    """line(width=2) -> [(xa, y, xb)] inclusive spans on the rows of ``rows`` (a range), unclipped in x: polygon_generic of Draw.c
    on (x0, y0 + ey), (x1, y1 + ey), (x1 + ex, y1), (x0 + ex, y0).  Horizontal edges are spans of their own; on a row every other
    edge with ymin <= y <= ymax gives x = (y - ya) * slope + xa in C floats (a: the edge's first vertex), twice when y is the edge's
    last row and not the polygon's; the sorted values are taken in pairs, each filling [ROUND_UP(a), ROUND_DOWN(b)]."""
    if x0 == x1 and y0 == y1:
        return [(x0, y0, x0)] if y0 in rows else []
    ex, ey = wide_line_offsets(x1 - x0, y1 - y0)
    v = [(x0, y0 + ey), (x1, y1 + ey), (x1 + ex, y1), (x0 + ex, y0)]
    spans, edges = [], []
    for k in range(4):
        (xa, ya), (xb, yb) = v[k], v[(k + 1) % 4]
        if ya == yb:
            if ya in rows:
                spans.append((min(xa, xb), ya, max(xa, xb)))
        else:
            edges.append((xa, ya, min(ya, yb), max(ya, yb), f32(f32(xb - xa) / f32(yb - ya))))
    top = max(p[1] for p in v)
    for y in rows:
        xx = []
        for xa, ya, ymin, ymax, slope in edges:
            if ymin <= y <= ymax:
                xv = f32(f32(f32(y - ya) * slope) + f32(xa))
                xx.append(xv)
                if y == ymax and y < top:
                    xx.append(xv)
        xx.sort()
        for i in range(1, len(xx), 2):
            a, b = round_up(xx[i - 1]), round_down(xx[i])
            if a <= b:
                spans.append((a, y, b))
    return spans


def disc_box(cx, cy):
    """The truncated box of ellipse([c - 5 for c in centre] + [c + 5 for c in centre]): Python floats (doubles) of the fp32 centre."""
    cx, cy = float(f32(cx)), float(f32(cy))
    return [cx - 5, cy - 5, cx + 5, cy + 5]


def disc_covers(u, v, w, h):
    """Pixel (u, v) of a truncated box w wide and h high (each 9 or 10): the four stamps of PIL's ellipse."""
    return 0 <= u <= w and 0 <= v <= h and min(u, w - u) + min(v, h - v) >= 3


# ---- the draw call ------------------------------------------------------------------------------------------------------------
def truncate(v):
    """(int) of a double, or None where the primitive is skipped: not finite, or the truncation outside [-32768, 32767]."""
    v = float(v)
    if not math.isfinite(v):
        return None
    t = math.trunc(v)
    return t if COORD_MIN <= t <= COORD_MAX else None


def draw(canvas, kinds, points, colours, frame, panel, panel_width):
    """ops.draw on a numpy uint8 canvas [B, H, P * Wp, 3], in place -> the number of skipped primitives.  Primitives are painted in
    index order, so a pixel ends with the colour of the highest-index primitive covering it; each paints only inside its own panel."""
    B, H, Wc, _ = canvas.shape
    Wp = int(panel_width)
    P = Wc // Wp
    assert P * Wp == Wc
    skipped = 0
    for i in range(len(kinds)):
        k, b, p = int(kinds[i]), int(frame[i]), int(panel[i])
        if k not in (LINE, LINE2, DISC) or not 0 <= b < B or not 0 <= p < P:
            skipped += 1
            continue
        pt = [f32(c) for c in points[i]]
        box = disc_box(pt[0], pt[1]) if k == DISC else [float(c) for c in pt]
        t = [truncate(c) for c in box]
        if any(c is None for c in t):
            skipped += 1
            continue
        col = np.asarray(colours[i], dtype=np.uint8)
        view = canvas[b, :, p * Wp:(p + 1) * Wp]
        if k == LINE:
            for x, y in thin_line_pixels(*t):
                if 0 <= x < Wp and 0 <= y < H:
                    view[y, x] = col
        elif k == LINE2:
            for xa, y, xb in wide_line_spans(*t, range(max(0, min(t[1], t[3]) - 1), min(H, max(t[1], t[3]) + 2))):
                xa, xb = max(xa, 0), min(xb, Wp - 1)
                if xa <= xb:
                    view[y, xa:xb + 1] = col
        else:
            w, h = t[2] - t[0], t[3] - t[1]
            for v in range(h + 1):
                for u in range(w + 1):
                    x, y = t[0] + u, t[1] + v
                    if disc_covers(u, v, w, h) and 0 <= x < Wp and 0 <= y < H:
                        view[y, x] = col
    return skipped


# ---- the primitive lists of the four methods (B = 1) -----------------------------------------------------------------------------
def _lists(recs):
    kinds = np.array([r[0] for r in recs], dtype=np.int32).reshape(-1)
    points = np.array([r[1] for r in recs], dtype=np.float32).reshape(-1, 4)
    colours = np.array([r[2] for r in recs], dtype=np.uint8).reshape(-1, 3)
    panel = np.array([r[3] for r in recs], dtype=np.int32).reshape(-1)
    return kinds, points, colours, np.zeros(len(recs), dtype=np.int32), panel


def graph_list(edge_index, center, node_colours, edge_colour, panels=(0,)):
    """Edges in edge order, then discs in node order, per panel: node_colours[k] is the [N, 3] table of panel panels[k]."""
    center = np.asarray(center, dtype=np.float32)
    recs = []
    for k, p in enumerate(panels):
        for i in range(edge_index.shape[1]):
            a, b = int(edge_index[0, i]), int(edge_index[1, i])
            recs.append((LINE, [center[a, 0], center[a, 1], center[b, 0], center[b, 1]], edge_colour, p))
        for i in range(center.shape[0]):
            recs.append((DISC, [center[i, 0], center[i, 1], 0, 0], node_colours[k][i], p))
    return _lists(recs)


def traversability_graph_list(prediction, edge_index, center, table, valid=None, colorize_invalid_centers=False):
    """plot_traversability_graph: grey edges, discs of table[uint8(prediction * 255)], grey where the node is invalid."""
    index = (np.asarray(prediction, dtype=np.float32) * f32(255)).astype(np.uint8)
    cols = np.asarray(table, dtype=np.uint8)[index]
    if valid is not None and not colorize_invalid_centers:
        cols = np.where(np.asarray(valid, dtype=bool)[:, None], cols, np.uint8(127))
    return graph_list(edge_index, center, [cols], (127, 127, 127))


def graph_result_list(edge_index, center, y, res, table, use_seg=False):
    """plot_graph_result: [prediction | ground truth | (segmentation)], red edges, discs of table[uint8(value * 255)]."""
    table = np.asarray(table, dtype=np.uint8)
    c_y = table[(np.asarray(y, dtype=np.float32) / f32(1.0) * f32(255)).astype(np.uint8)]
    c_pred = table[(np.clip(np.asarray(res, dtype=np.float32), 0, 1) / f32(1.0) * f32(255)).astype(np.uint8)]
    return graph_list(edge_index, center, [c_pred, c_y] + ([c_y] if use_seg else []), (255, 0, 0), panels=range(3 if use_seg else 2))


def optical_flow_list(flow, s=10):
    """plot_optical_flow: from (v, u) to (v + dv, u + du) for every s-th pixel; du = flow[0, u, v], dv = fp32(flow[1, u, v] + W); the
    sums with the integer sample position are doubles, truncated as such (and exact as the fp32 coordinates of a record)."""
    flow = np.asarray(flow, dtype=np.float32)
    _, H, W = flow.shape
    recs = []
    for ku in range(int(H / s)):
        u = int(ku * s)
        for kv in range(int(W / s)):
            v = int(kv * s)
            du = float(flow[0, u, v])
            dv = float(f32(flow[1, u, v] + f32(W)))
            recs.append((LINE2, [v, u, _pretruncate(v + dv), _pretruncate(u + du)], (0, 255, 0), 0))
    return _lists(recs)


def _pretruncate(v):
    """A double sum as an fp32 coordinate that truncates alike: its truncation where that is exact in fp32, else the value itself
    (not finite, or far outside the drawable range: skipped either way)."""
    return float(math.trunc(v)) if math.isfinite(v) and abs(v) < 2 ** 24 else v


def sparse_optical_flow_list(pre_pos, cur_pos, W):
    """plot_sparse_optical_flow: (p0, p1) -> (fp32(W + c0), c1)."""
    pre, cur = np.asarray(pre_pos, dtype=np.float32), np.asarray(cur_pos, dtype=np.float32)
    recs = [(LINE2, [p[0], p[1], f32(f32(W) + c[0]), c[1]], (0, 255, 0), 0) for p, c in zip(pre, cur)]
    return _lists(recs)


def graph_result_table(name="RdYlBu"):
    """``np.uint8(cm.get_cmap(name, 255)(np.linspace(0, 1, 256))[:, :3] * 255)`` of plot_graph_result, on today's matplotlib."""
    import matplotlib

    return np.uint8(matplotlib.colormaps[name].resampled(255)(np.linspace(0, 1, 256))[:, :3] * 255)
