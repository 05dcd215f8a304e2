"""csrc/draw.hip through ops.draw and the graph / flow views of LearningVisualizer, against tests/visu_draw_ref.py (the primitives as
plain loops, held to PIL.ImageDraw by tests/test_visu_draw_host.py) and against PIL itself.  Every comparison is equality of bytes."""
import random
import sys
import types

import numpy as np
import pytest
import torch

import visu_draw_ref as DR
from wild_visual_navigation_amd import ops
from wild_visual_navigation_amd.visu import LearningVisualizer, colour_table
from wild_visual_navigation_amd.visu.colormaps import graph_result_table

pytestmark = pytest.mark.gpu
SIZES = ((64, 48), (53, 37))   # (W, H): three and four tiles of 16 with a tail


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _both(dev, canvas, kinds, pts, cols, frame, panel, Wp, view=None):
    """canvas: numpy uint8 [B,H,Wc,3]; view: (c0, c1) = the columns drawn on (a slice of a wider image).  Runs the statement on a
    copy and the kernel on the device, compares the whole images and the skip counts, returns the picture."""
    kinds, pts = np.asarray(kinds, np.int32).reshape(-1), np.asarray(pts, np.float32).reshape(-1, 4)
    cols, frame, panel = np.asarray(cols, np.uint8).reshape(-1, 3), np.asarray(frame, np.int32).reshape(-1), np.asarray(panel, np.int32).reshape(-1)
    c0, c1 = view if view is not None else (0, canvas.shape[2])
    want = canvas.copy()
    n_skip = DR.draw(want[:, :, c0:c1], kinds, pts, cols, frame, panel, Wp)
    got = torch.from_numpy(canvas).to(dev)
    skipped = torch.zeros(1, dtype=torch.int32, device=dev)
    ret = ops.draw(got[:, :, c0:c1], *(torch.from_numpy(a).to(dev) for a in (kinds, pts, cols, frame, panel)), Wp, skipped=skipped)
    assert ret.data_ptr() == got[:, :, c0:c1].data_ptr()
    diff = (got.cpu().numpy() != want).any(-1)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5].tolist())
    assert int(skipped) == n_skip
    return want


def _noise(B, H, Wc, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (B, H, Wc, 3)).astype(np.uint8)


def _random_prims(rng, n, kind, W, H, B, P):
    kinds = [rng.choice((DR.LINE, DR.LINE2, DR.DISC)) if kind is None else kind for _ in range(n)]
    pts = [[rng.uniform(-16, W + 16), rng.uniform(-16, H + 16), rng.uniform(-16, W + 16), rng.uniform(-16, H + 16)] for _ in range(n)]
    cols = [[rng.randint(0, 255) for _ in range(3)] for _ in range(n)]
    return kinds, pts, cols, [rng.randrange(B) for _ in range(n)], [rng.randrange(P) for _ in range(n)]


@pytest.mark.parametrize("kind", [DR.LINE, DR.LINE2, DR.DISC, None])
@pytest.mark.parametrize("size, P", [(SIZES[0], 1), (SIZES[1], 3), (SIZES[1], 2)])
def test_random_primitives(dev, kind, size, P):
    """Each kind alone and all mixed, B = 2, one to three panels; float coordinates in [-16, size + 16]: clipped at every border."""
    W, H = size
    rng = random.Random(100 * P + W + (7 if kind is None else kind))
    prims = _random_prims(rng, 120, kind, W, H, 2, P)
    out = _both(dev, _noise(2, H, P * W), *prims, W)
    assert (out != _noise(2, H, P * W)).any()


@pytest.mark.parametrize("kind", [DR.LINE, DR.LINE2, DR.DISC])
def test_borders_and_off_canvas(dev, kind):
    """Primitives crossing each of the four borders, touching the corners, and entirely outside (which change nothing)."""
    W, H = SIZES[1]
    base = _noise(1, H, W, 3)
    across = [(-9, 10, 9, 14), (W - 6, 10, W + 9, 3), (10, -9, 14, 9), (10, H - 4, 3, H + 9), (-3, -3, 4, 4), (W + 2, H + 2, W - 4, H - 5),
              (-8, H // 2, W + 8, H // 2 + 1), (W // 2, -8, W // 2 + 1, H + 8), (0, 0, 0, 0), (W - 1, H - 1, W - 1, H - 1), (2.5, 2.5, 0, 0),
              (W - 2.5, H - 2.5, W, H), (0, H - 1, W - 1, H - 1), (W - 1, 0, W - 1, H - 1), (-5.5, -5.5, -5.5, -5.5), (W + 4.5, H + 4.5, 0, 0)]
    outside = [(-12, -12, -7, 40), (W + 7, 0, W + 12, H), (0, -12, W, -7), (0, H + 7, W, H + 12), (-100, -100, -50, -60), (W, H, W, H),
               (-1, -1, -1, -1), (W + 5.5, 10, W + 5.5, 10), (10, -6.5, 10, -6.5)]
    n = len(across)
    out = _both(dev, base, [kind] * n, across, [(255, i, 0) for i in range(n)], [0] * n, [0] * n, W)
    assert (out != base).any()
    outside = [outside[i] for i in (0, 1, 2, 3, 4, 7, 8)] if kind == DR.DISC else outside[:7]   # (a disc reaches 5 beyond its centre)
    m = len(outside)
    out = _both(dev, base, [kind] * m, outside, [(0, 255, i) for i in range(m)], [0] * m, [0] * m, W)
    assert (out == base).all()


def test_overlapping_discs_in_both_orders_and_a_disc_on_a_panel_boundary(dev):
    W, H = SIZES[1]
    base = np.zeros((1, H, 2 * W, 3), np.uint8)
    pts = [(20, 15, 0, 0), (24, 17, 0, 0)]
    a = _both(dev, base, [DR.DISC] * 2, pts, [(255, 0, 0), (0, 0, 255)], [0, 0], [0, 0], W)
    b = _both(dev, base, [DR.DISC] * 2, pts[::-1], [(0, 0, 255), (255, 0, 0)], [0, 0], [0, 0], W)
    assert (a != b).any() and ((a != 0).any(-1) == (b != 0).any(-1)).all()
    assert a[0, 16, 22].tolist() == [0, 0, 255] and b[0, 16, 22].tolist() == [255, 0, 0]       # the higher index wins
    # PIL draws on separate images: a disc at a panel's edge does not bleed into the neighbour
    pts = [(W - 2, 10, 0, 0), (1.5, 20, 0, 0), (W - 0.5, 30, 0, 0)]
    out = _both(dev, base, [DR.DISC] * 3, pts, [(9, 9, 9)] * 3, [0] * 3, [0, 1, 1], W)
    assert (out[0, 5:15, W:] == 0).all() and (out[0, 16:26, :W] == 0).all() and (out[0, 25:36, :W] == 0).all()
    assert (out[0, 10, W - 7:W] == 9).all() and (out[0, 20, W:W + 7] == 9).all() and (out[0, 30, 2 * W - 5:] == 9).all()


def test_column_slice_of_a_wider_image(dev):
    """The canvas is columns 7 .. 7 + 2 * 20 of a 64-wide image (an odd byte address, pitched rows): nothing outside is touched."""
    rng = random.Random(11)
    prims = _random_prims(rng, 90, None, 20, 37, 2, 2)
    base = _noise(2, 37, 64, 5)
    out = _both(dev, base, *prims, 20, view=(7, 47))
    assert (out[:, :, :7] == base[:, :, :7]).all() and (out[:, :, 47:] == base[:, :, 47:]).all() and (out != base).any()


def test_three_hundred_lines_on_one_tile(dev):
    """More records meet one tile than a chunk of the list loop holds: the order survives the chunk boundary."""
    W, H = SIZES[0]
    rng = random.Random(12)
    n = 300
    pts = [[rng.uniform(16, 32), rng.uniform(16, 32), rng.uniform(16, 32), rng.uniform(16, 32)] for _ in range(n)]
    kinds = [rng.choice((DR.LINE, DR.LINE2)) for _ in range(n)]
    cols = [(i % 256, i // 256, 77) for i in range(n)]
    out = _both(dev, np.zeros((1, H, W, 3), np.uint8), kinds, pts, cols, [0] * n, [0] * n, W)
    assert (out[0, :, :, 1] == 1).any() and (out[0, :, :, 1][out[0, :, :, 2] == 77] <= 1).all()   # records 256.. are visible
    # the last record overrules everything before it, wherever the chunks fall
    pts[-1] = [16, 24, 32, 24]
    kinds[-1] = DR.LINE
    out = _both(dev, np.zeros((1, H, W, 3), np.uint8), kinds, pts, cols, [0] * n, [0] * n, W)
    assert (out[0, 24, 16:33] == np.array(cols[-1], np.uint8)).all()


def test_empty_list_and_skipped_records(dev):
    W, H = SIZES[1]
    base = _noise(2, H, 2 * W, 8)
    e = np.zeros
    out = _both(dev, base, e(0, np.int32), e((0, 4), np.float32), e((0, 3), np.uint8), e(0, np.int32), e(0, np.int32), W)
    assert (out == base).all()
    got = torch.from_numpy(base).to(dev)
    ops.draw(got, torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, 4, device=dev), torch.zeros(0, 3, dtype=torch.uint8, device=dev),
             panel_width=W)
    assert torch.equal(got.cpu(), torch.from_numpy(base))
    # NaN, inf, 1e12, a disc whose box leaves the range, frame / panel outside the canvas, an unknown kind: skipped and counted; the
    # good records around them are drawn as if the bad ones were not there
    nan, inf = float("nan"), float("inf")
    good = [(DR.LINE, (3, 3, 40, 30)), (DR.DISC, (20, 20, 0, 0)), (DR.LINE2, (50, 2, 5, 33))]
    bad = [(DR.LINE, (nan, 3, 40, 30)), (DR.LINE, (3, 3, 40, inf)), (DR.LINE2, (3, -inf, 40, 30)), (DR.LINE2, (3, 3, 1e12, 30)),
           (DR.DISC, (nan, 20, 0, 0)), (DR.DISC, (20, 1e12, 0, 0)), (DR.DISC, (32763.5, 20, 0, 0)), (DR.LINE, (-32769, 3, 40, 30)),
           (7, (3, 3, 40, 30)), (-1, (3, 3, 40, 30))]
    recs = [good[0]] + bad[:4] + [good[1]] + bad[4:] + [good[2]]
    n = len(recs)
    frame, panel = [0] * n, [1] * n
    mixed = _both(dev, base, [r[0] for r in recs], [r[1] for r in recs], [(1, 2, 3 + i) for i in range(n)], frame, panel, W)
    idx = [0, 5, n - 1]
    alone = _both(dev, base, [recs[i][0] for i in idx], [recs[i][1] for i in idx], [(1, 2, 3 + i) for i in idx], [0] * 3, [1] * 3, W)
    assert (mixed == alone).all() and (mixed != base).any()
    # a disc reads its centre only: the unused second point may hold anything
    _both(dev, base, [DR.DISC], [(20, 20, nan, 1e30)], [(5, 5, 5)], [0], [0], W)
    # frame and panel outside the canvas
    out = _both(dev, base, [DR.LINE] * 4, [(3, 3, 40, 30)] * 4, [(9, 9, 9)] * 4, [2, -1, 0, 0], [0, 0, 2, -1], W)
    assert (out == base).all()
    # the extreme drawable coordinates (the 64-bit branch of the Bresenham division, a 65535-long 2-pixel line)
    far = [(-32768, -32768, 32767, 32767), (32767, -32768, -32768, 32767), (-32768, 10, 32767, 30), (20, 32767, 30, -32768)]
    for kind in (DR.LINE, DR.LINE2):
        out = _both(dev, base, [kind] * 4, far, [(200, 100, i) for i in range(4)], [0, 1, 0, 1], [0, 1, 1, 0], W)
        assert (out != base).any()


# ---- the visualizer ------------------------------------------------------------------------------------------------------------------
def _graph(g, N=10, W=64, H=48):
    """A 10-node graph with self-loops, y_valid mixed, centres on and beyond the borders."""
    center = torch.rand(N, 2, generator=g) * torch.tensor([W + 8.0, H + 8.0]) - 4
    center[0] = torch.tensor([1e-10, 2.5])
    src = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0, 3, 3, 9, 5, 2])
    dst = torch.tensor([1, 2, 3, 4, 5, 6, 7, 8, 9, 0, 5, 3, 8, 9, 1, 7])
    graph = types.SimpleNamespace(edge_index=torch.stack([src, dst]), y_valid=torch.tensor([1, 1, 0, 1, 0, 1, 1, 1, 0, 1], dtype=torch.bool),
                                  y=torch.rand(N, generator=g))
    return graph, center, torch.rand(N, generator=g)


def _to(graph, dev):
    return types.SimpleNamespace(**{k: v.to(dev) for k, v in vars(graph).items()})


def _pil_traversability_graph(prediction, graph, center, img, table, colorize_invalid_centers=False):
    """visualizer.py:273-309 of the reference, restated: the PIL loop."""
    from PIL import Image, ImageDraw

    prediction = (prediction.type(torch.float32) * 255).type(torch.uint8)
    img_pil = Image.fromarray(np.uint8((img.permute(1, 2, 0) * 255).cpu().numpy()))
    img_draw = ImageDraw.Draw(img_pil)
    adjacency_list = graph.edge_index
    try:
        node_validity = graph.y_valid
    except Exception:
        node_validity = [True] * center.shape[0]
    for i in range(adjacency_list.shape[1]):
        a, b = adjacency_list[0, i], adjacency_list[1, i]
        img_draw.line(center[a].tolist() + center[b].tolist(), fill=(127, 127, 127))
    for i in range(center.shape[0]):
        params = center[i].tolist()
        params = [p - 5 for p in params] + [p + 5 for p in params]
        if node_validity[i] or colorize_invalid_centers:
            img_draw.ellipse(params, width=10, fill=tuple(table[prediction[i]].tolist()))
        else:
            img_draw.ellipse(params, width=1, fill=(127, 127, 127))
    return np.array(img_pil)


@pytest.fixture(scope="module")
def scene():
    g = _gen(3)
    graph, center, pred = _graph(g)
    return graph, center, pred, torch.rand(3, 48, 64, generator=g)


def test_plot_traversability_graph_equals_the_pil_loop(dev, scene):
    pytest.importorskip("PIL")
    graph, center, pred, img = scene
    table = colour_table("RdYlBu", 256).numpy()
    vis = LearningVisualizer()
    for colorize in (False, True):
        want = _pil_traversability_graph(pred, graph, center, img, table, colorize)
        got = vis.plot_traversability_graph(pred.to(dev), _to(graph, dev), center.to(dev), img.to(dev), colorize_invalid_centers=colorize)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
        assert np.array_equal(vis.plot_traversability_graph(pred, graph, center, img, colorize_invalid_centers=colorize), want)   # host inputs
    # no y_valid: every node valid; the statement's list gives the same picture
    bare = types.SimpleNamespace(edge_index=graph.edge_index)
    want = _pil_traversability_graph(pred, bare, center, img, table)
    got = vis.plot_traversability_graph(pred.to(dev), _to(bare, dev), center.to(dev), img.to(dev), as_tensor=True)
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    ref = np.uint8((img.permute(1, 2, 0) * 255).numpy())[None].copy()
    DR.draw(ref, *DR.traversability_graph_list(pred.numpy(), graph.edge_index.numpy(), center.numpy(), table), 64)
    assert np.array_equal(ref[0], want)
    again = vis.plot_traversability_graph(pred.to(dev), _to(bare, dev), center.to(dev), img.to(dev), as_tensor=True)
    assert torch.equal(got, again)                                                                     # two runs: identical bytes
    with pytest.raises(AssertionError, match="Pred out of Bounds"):
        vis.plot_traversability_graph((pred + 1).to(dev), _to(graph, dev), center.to(dev), img.to(dev))
    # a batch sharing one graph: frame b is the single-frame picture of its own centres and predictions
    g = _gen(4)
    imgs = torch.rand(2, 3, 48, 64, generator=g)
    centers = torch.stack([center, center.flip(0)])
    preds = torch.stack([pred, torch.rand(10, generator=g)])
    both = vis.plot_traversability_graph(preds.to(dev), _to(graph, dev), centers.to(dev), imgs.to(dev))
    for b in range(2):
        assert np.array_equal(both[b], _pil_traversability_graph(preds[b], graph, centers[b], imgs[b], table))


def test_plot_traversability_graph_without_pil(dev, scene, monkeypatch):
    """The graph view needs no PIL at run time (before: ImportError from the method's own import)."""
    graph, center, pred, img = scene
    vis = LearningVisualizer()
    want = vis.plot_traversability_graph(pred.to(dev), _to(graph, dev), center.to(dev), img.to(dev))
    for name in [m for m in sys.modules if m == "PIL" or m.startswith("PIL.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(ImportError):
        import PIL  # noqa: F401
    got = LearningVisualizer().plot_traversability_graph(pred.to(dev), _to(graph, dev), center.to(dev), img.to(dev))
    assert np.array_equal(got, want) and (got != np.uint8((img.permute(1, 2, 0) * 255).numpy())).any()


@pytest.mark.parametrize("use_seg", [False, True])
def test_plot_graph_result(dev, scene, use_seg):
    Image = pytest.importorskip("PIL.Image")
    ImageDraw = pytest.importorskip("PIL.ImageDraw")
    graph, center, _, img = scene
    res = torch.rand(10, generator=_gen(9)) * 1.4 - 0.2                                               # clipped to [0, 1]
    seg = (torch.arange(48 * 64).reshape(48, 64) * 10 // (48 * 64))
    table = graph_result_table("RdYlBu").numpy()
    vis = LearningVisualizer()
    got = vis.plot_graph_result(_to(graph, dev), center.to(dev), img.to(dev), seg.to(dev), res.to(dev), use_seg=use_seg)
    # visualizer.py:439-484 of the reference, restated
    y = (graph.y.type(torch.float32) / 1.0 * 255).type(torch.uint8)
    y_pred = (res.clip(0, 1.0) / 1.0 * 255).type(torch.uint8)
    frame = np.uint8((img.permute(1, 2, 0) * 255).numpy())
    pils = [Image.fromarray(frame.copy()), Image.fromarray(frame.copy())]
    cols = [y_pred, y]
    if use_seg:
        pils.append(Image.fromarray(vis.plot_segmentation(seg.to(dev), max_seg=100)))
        cols.append(y)
    for pil, c in zip(pils, cols):
        d = ImageDraw.Draw(pil)
        for i in range(graph.edge_index.shape[1]):
            a, b = graph.edge_index[0, i], graph.edge_index[1, i]
            d.line(center[a].tolist() + center[b].tolist(), fill=(255, 0, 0))
        for i in range(10):
            params = center[i].tolist()
            d.ellipse([p - 5 for p in params] + [p + 5 for p in params], width=10, fill=tuple(table[c[i]].tolist()))
    want = np.concatenate([np.array(p) for p in pils], axis=1)
    assert got.shape == (48, 64 * (3 if use_seg else 2), 3) and np.array_equal(got, want)
    # the statement's list, and a device result
    if not use_seg:
        ref = np.concatenate([frame, frame], axis=1)[None].copy()
        DR.draw(ref, *DR.graph_result_list(graph.edge_index.numpy(), center.numpy(), graph.y.numpy(), res.numpy(), table), 64)
        assert np.array_equal(ref[0], want)
    t = vis.plot_graph_result(_to(graph, dev), center.to(dev), img.to(dev), seg.to(dev), res.to(dev), use_seg=use_seg, as_tensor=True)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), want)


def test_flow_plots(dev):
    Image = pytest.importorskip("PIL.Image")
    ImageDraw = pytest.importorskip("PIL.ImageDraw")
    g = _gen(21)
    H = W = 64
    img1, img2 = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g) * 255             # both ranges of plot_image
    flow = torch.randn(2, H, W, generator=g) * 12
    flow[0, 4, 8], flow[1, 4, 8] = 0.99999994, 0.99999994                                           # the fp32 / double sums of the far end
    flow[:, 8, 8] = float("nan")                                                                      # defined beyond PIL: skipped
    flow[1, 12, 8] = float("inf")
    vis = LearningVisualizer()
    got = vis.plot_optical_flow(flow.to(dev), img1.to(dev), img2.to(dev), s=4)
    i1, i2 = np.uint8((img1.permute(1, 2, 0) * 255).numpy()), np.uint8(img2.permute(1, 2, 0).numpy())
    base = np.concatenate([i1, i2], axis=1)
    pil = Image.fromarray(base.copy())
    draw = ImageDraw.Draw(pil)
    s = 4
    for u in range(int(flow.shape[1] / s)):                                                           # visualizer.py:560-569, restated
        u = int(u * s)
        for v in range(int(flow.shape[2] / s)):
            v = int(v * s)
            du = (flow[0, u, v]).item()
            dv = (flow[1, u, v] + i2.shape[1]).item()
            if not (np.isfinite(du) and np.isfinite(dv)):
                continue
            draw.line([(v, u), (v + dv, u + du)], fill=(0, 255, 0), width=2)
    want = np.array(pil).astype(np.uint8)
    assert got.shape == (H, 2 * W, 3) and np.array_equal(got, want) and (want != base).any()
    ref = base[None].copy()
    assert DR.draw(ref, *DR.optical_flow_list(flow.numpy(), s=4), 2 * W) == 2
    assert np.array_equal(ref[0], want)
    t = vis.plot_optical_flow(flow.to(dev), img1.to(dev), img2.to(dev), s=4, as_tensor=True)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), want)
    assert np.array_equal(vis.plot_optical_flow(flow.to(dev), img1.to(dev), img2.to(dev), s=4), want)   # two runs: identical bytes
    # sparse: tracked points, some leaving the picture
    pre = torch.rand(40, 2, generator=g) * torch.tensor([W + 10.0, H + 10.0]) - 5
    cur = pre + torch.randn(40, 2, generator=g) * 6
    got = vis.plot_sparse_optical_flow(pre.to(dev), cur.to(dev), img1.to(dev), img2.to(dev))
    pil = Image.fromarray(base.copy())
    draw = ImageDraw.Draw(pil)
    for p, c in zip(pre, cur):                                                                        # visualizer.py:601-612, restated
        draw.line([(p[0].item(), p[1].item()), ((i2.shape[1] + c[0]).item(), c[1].item())], fill=(0, 255, 0), width=2)
    want = np.array(pil).astype(np.uint8)
    assert np.array_equal(got, want) and (want != base).any()
    ref = base[None].copy()
    DR.draw(ref, *DR.sparse_optical_flow_list(pre.numpy(), cur.numpy(), W), 2 * W)
    assert np.array_equal(ref[0], want)
    t = vis.plot_sparse_optical_flow(pre.to(dev), cur.to(dev), img1.to(dev), img2.to(dev), as_tensor=True)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), want)


def test_graph_on_seg_draws_the_graph_on_the_overlay(dev, scene):
    """draw_graph=True: the overlay bytes with the graph of plot_traversability_graph on top; the default picture is unchanged."""
    graph, center, pred, img = scene
    seg = (torch.arange(48 * 64).reshape(48, 64) * 10 // (48 * 64))
    vis = LearningVisualizer()
    plain = vis.plot_traversability_graph_on_seg(pred.to(dev), seg.to(dev), None, None, img.to(dev))
    same = vis.plot_traversability_graph_on_seg(pred.to(dev), seg.to(dev), _to(graph, dev), center.to(dev), img.to(dev), draw_graph=False)
    assert np.array_equal(plain, same)
    got = vis.plot_traversability_graph_on_seg(pred.to(dev), seg.to(dev), _to(graph, dev), center.to(dev), img.to(dev), draw_graph=True)
    want = plain[None].copy()
    DR.draw(want, *DR.traversability_graph_list(pred.numpy(), graph.edge_index.numpy(), center.numpy(), colour_table("RdYlBu", 256).numpy(),
                                                graph.y_valid.numpy()), 64)
    assert np.array_equal(got, want[0]) and (got != plain).any()
