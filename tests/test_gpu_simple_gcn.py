"""SimpleGCN on the GPU (csrc/simple_gcn.hip, model/simple_gcn.py) against the float64 statement of the definition
(tests/simple_gcn_ref.py).

Accuracy rule ("within bound"): max abs error against the float64 statement <= max(8 x the error of the same statement run in
float32 on the CPU on the same inputs, 2^-16 x max|float64 output|).  Inputs are x = 2 randn with glorot weights.  Every case
prints (error, bound, float32-statement error).

Measured on an MI355X (error / bound): definition cases at most 7.7e-08 / 7.5e-06; widths and row counts at most 1.4e-06 / 3.9e-05
(D = 768, N = 801; the float32 statement itself errs by 7.6e-07 there); the 300-edge star 3.1e-06 / 1.3e-04 at max|out| 8.3, THE
WORST (float32 statement 3.1e-06); the chain behind a NaN row 6.3e-07 / 2.4e-05; the per-segment table (trav, loss, conf) at most
3.0e-07 / 1.4e-05; one Adam step of the estimator 3.8e-08 against a parameter change of 5.0e-02 (7.6e-07 of it; the bar is
1.5e-05); the HIP forward on the trained weights 9.0e-09 / 8.4e-06.

Reading of "bit-identical to a per-frame statement" for predict_per_segment: the traversability map equals, bit for bit,
``model.forward(Data(x=feat[b], edge_index=edges_b))[:, 0][seg[b]]`` with ``edges_b`` from ``SegmentExtractor.adjacency_list``;
the confidence and loss maps equal, bit for bit, the single-frame ``forward_per_segment(feat[b], seg[b], edges=edges_b)`` (the
kernel's own row loss: torch's ``mean`` has another summation order, so a torch-side confidence cannot be bit-identical), and all
three are within bound of the float64 statement's table."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_gcn_ref as REF  # noqa: E402

from wild_visual_navigation_amd import _lib, ops  # noqa: E402
from wild_visual_navigation_amd.cfg import ExperimentParams  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import FeatureExtractor  # noqa: E402
from wild_visual_navigation_amd.feature_extractor.segment_extractor import SegmentExtractor  # noqa: E402
from wild_visual_navigation_amd.model import SimpleGCN  # noqa: E402
from wild_visual_navigation_amd.traversability_estimator import MissionNode, TraversabilityEstimator  # noqa: E402
from wild_visual_navigation_amd.utils import Batch, ConfidenceGenerator, Data  # noqa: E402

pytestmark = pytest.mark.gpu

MEAN, STD, FAC = 0.9, 0.25, 0.5
WIDE = [256, 128, 1]


def g(seed):
    return torch.Generator().manual_seed(seed)


def _model(dev, D, hidden, seed=7):
    sd = REF.glorot_state_dict(D, hidden, seed)
    m = SimpleGCN(D, True, hidden)
    m.load_state_dict(sd)
    return m.to(dev).eval(), sd


def _run(m, x, ei, dev):
    return m(Data(x=x.to(dev), edge_index=ei.to(dev)))


def _within_bound(what, got, ref64, ref32):
    err, bnd, err32 = REF.rule(got, ref64, ref32)
    print(f"{what}: err {err:.3e} bound {bnd:.3e} (float32 statement {err32:.3e}, max|ref| {ref64.abs().max().item():.3f})")
    assert err <= bnd, (what, err, bnd)


def _check(what, m, sd, x, ei, dev):
    out = _run(m, x, ei, dev)
    assert out.shape == (x.shape[0], 1 + x.shape[1]) and out.dtype == torch.float32
    _within_bound(what, out, REF.forward(sd, x, ei), REF.forward(sd, x, ei, torch.float32))
    return out


def _random_edges(N, mean_in_degree, seed):
    return torch.randint(0, N, (2, mean_in_degree * N), generator=g(seed))


# ---- definition cases ------------------------------------------------------------------------------------------------------------
DEFINITION = {
    "single node": (1, []),
    "path": (3, [(0, 1), (1, 2)]),
    "path and back": (3, [(0, 1), (1, 2), (1, 0), (2, 1)]),
    "duplicate and self loop": (3, [(0, 1), (0, 1), (1, 1), (2, 1)]),
    "isolated node": (4, [(0, 1), (1, 2)]),
}


@pytest.mark.parametrize("name", list(DEFINITION))
def test_definition_cases(dev, name):
    N, edges = DEFINITION[name]
    m, sd = _model(dev, 5, [7, 3, 1])
    x = 2 * torch.randn(N, 5, generator=g(N))
    ei = torch.tensor(edges, dtype=torch.long).reshape(-1, 2).t().contiguous()
    out = _check(name, m, sd, x, ei, dev)
    if N == 1:   # no neighbours: every layer is x W^T + b
        h = x.double()
        for l in range(3):
            h = h @ sd[f"layers.{l}.lin.weight"].double().t() + sd[f"layers.{l}.bias"].double()
            h = torch.relu(h) if l < 2 else torch.cat([torch.sigmoid(h[:, :1]), h[:, 1:]], 1)
        assert (out.cpu().double() - h).abs().max().item() <= 2.0 ** -16 * h.abs().max().item()


# ---- widths and ragged row counts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [17, 100, 801])
@pytest.mark.parametrize("D,hidden", [(90, WIDE), (384, WIDE), (768, WIDE), (384, [64, 32, 1])])
def test_widths_and_ragged_rows(dev, D, hidden, N):
    m, sd = _model(dev, D, hidden)
    x = 2 * torch.randn(N, D, generator=g(D + N))
    out = _check(f"D={D} hidden={hidden} N={N}", m, sd, x, _random_edges(N, 6, N), dev)
    assert ((out[:, 0] > 0) & (out[:, 0] < 1)).all()


def test_high_degree_row(dev):
    """edges k -> 0 and 0 -> k for k = 1 .. 300: row 0 has 301 neighbours, far beyond any tile."""
    N, D = 301, 384
    k = torch.arange(1, N)
    ei = torch.cat([torch.stack([k, torch.zeros_like(k)]), torch.stack([torch.zeros_like(k), k])], dim=1)
    m, sd = _model(dev, D, WIDE)
    _check("star", m, sd, 2 * torch.randn(N, D, generator=g(1)), ei, dev)


# ---- order and position -----------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_edge_order_run_or_batch_position(dev):
    D = 90
    m, _ = _model(dev, D, WIDE)
    graphs = []
    for N, seed in ((37, 1), (50, 2)):
        graphs.append(Data(x=(2 * torch.randn(N, D, generator=g(seed))).to(dev), edge_index=_random_edges(N, 6, seed + 10).to(dev)))
    alone = [m(d).clone() for d in graphs]
    assert torch.equal(m(graphs[0]), alone[0])                                     # a second run
    perm = torch.randperm(graphs[0].edge_index.shape[1], generator=g(3)).to(dev)
    assert torch.equal(m(Data(x=graphs[0].x, edge_index=graphs[0].edge_index[:, perm])), alone[0])
    batch = Batch.from_data_list(graphs)
    both = m(batch)
    assert batch.edge_index[:, -1].min().item() >= 37                               # the second graph's edges were offset
    assert torch.equal(both[:37], alone[0]) and torch.equal(both[37:], alone[1])
    assert int(m.bad_edges.item()) == 0


def test_nan_row_reaches_three_hops(dev):
    N, D = 10, 90
    m, sd = _model(dev, D, WIDE)
    x = 2 * torch.randn(N, D, generator=g(4))
    x[0] = float("nan")
    ei = torch.stack([torch.arange(0, N - 1), torch.arange(1, N)])
    out = _run(m, x, ei, dev).cpu()
    assert torch.isnan(out[:4]).all() and torch.isfinite(out[4:]).all()
    ref64, ref32 = REF.forward(sd, x, ei), REF.forward(sd, x, ei, torch.float32)
    assert torch.isnan(ref64[:4]).all() and torch.isfinite(ref64[4:]).all()
    _within_bound("chain behind a NaN row", out[4:], ref64[4:], ref32[4:])


def test_bad_edges_are_dropped_and_counted(dev):
    N, D = 23, 90
    m, _ = _model(dev, D, WIDE)
    x = (2 * torch.randn(N, D, generator=g(5))).to(dev)
    ei = _random_edges(N, 4, 6)
    clean = m(Data(x=x, edge_index=ei.to(dev))).clone()
    assert int(m.bad_edges.item()) == 0
    bad = torch.cat([ei[:, :10], torch.tensor([[3, -1], [N, 5]]), ei[:, 10:]], dim=1)   # 3 -> N and -1 -> 5
    out = m(Data(x=x, edge_index=bad.to(dev)))
    assert torch.equal(out, clean)
    assert int(m.bad_edges.item()) == 2


# ---- adjacency bitmaps ------------------------------------------------------------------------------------------------------------
def _assert_bitmaps_equal_adjacency_lists(seg, S):
    adj = ops.seg_adjacency_batched(seg, S)
    assert adj.shape == (seg.shape[0], S, S) and adj.dtype == torch.uint8
    for b in range(seg.shape[0]):
        want = SegmentExtractor().adjacency_list(seg[b][None, None].long())
        nz = adj[b].nonzero()                                      # (l, r) pairs
        nz = nz[torch.argsort(nz[:, 0] + nz[:, 1] * S)]
        assert torch.equal(nz, want), (b, nz.shape, want.shape)
        assert int(adj[b].max()) <= 1


def test_adjacency_bitmaps_hand_made(dev):
    S = 6
    a = torch.zeros(16, 16, dtype=torch.int32)
    a[:8, 8:], a[8:, :5], a[8:, 5:11], a[8:, 11:] = 1, 2, 3, 5      # id 4 is absent
    a[3:5, 3:5] = 5
    b = (torch.arange(256).reshape(16, 16) // 43).to(torch.int32)  # ids 0 .. 5 in row-major runs
    _assert_bitmaps_equal_adjacency_lists(torch.stack([a, b]).to(dev), S)


def test_adjacency_bitmap_of_a_slic_map(dev, golden):
    u8 = golden("graph_img_448.pt")["frame_u8"]
    seg = ops.slic(u8.to(dev), 100, 10.0)
    _assert_bitmaps_equal_adjacency_lists(seg[None], ops.slic_num_clusters(448, 448, 100))


# ---- per-segment prediction ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_type,kwargs", [("grid", {"cell_size": 16}), ("slic", {})])
def test_predict_per_segment(dev, seg_type, kwargs):
    fe = FeatureExtractor(dev, segmentation_type=seg_type, feature_type="dino", input_size=64, allow_synthetic=True)
    D = fe.feature_dim
    m, sd = _model(dev, D, WIDE, seed=11)
    cg = ConfidenceGenerator(method="latest_measurement", std_factor=FAC).to(dev)
    cg.mean[0], cg.std[0] = MEAN, STD
    img = torch.rand(2, 3, 64, 64, generator=g(0)).to(dev)
    trav, conf, loss, feat, seg, nseg = fe.predict_per_segment(img, m, cg, want_loss=True, **kwargs)
    assert trav.shape == conf.shape == loss.shape == (2, 64, 64)
    for o in (trav, conf, loss):
        assert torch.isfinite(o).all()                              # an id absent from a frame gives NaN nowhere on the map
    S = feat.shape[1]
    for b in range(2):
        edges = SegmentExtractor().adjacency_list(seg[b][None, None].long()).t()
        present = torch.zeros(S, dtype=torch.bool)
        present[seg[b].unique().long().cpu()] = True
        assert torch.equal(~torch.isnan(feat[b]).any(1).cpu(), present)
        out = m(Data(x=feat[b], edge_index=edges))
        assert torch.equal(trav[b], out[:, 0][seg[b].long()])
        t1, c1, l1 = m.forward_per_segment(feat[b], seg[b], MEAN, STD, FAC, want_loss=True, edges=edges)
        assert torch.equal(trav[b], t1) and torch.equal(conf[b], c1) and torch.equal(loss[b], l1)
        # the table against the float64 statement, on the rows the frame has
        x = feat[b].cpu()
        rows = [REF.table(REF.forward(sd, x, edges, dt), x, MEAN, STD, FAC) for dt in (torch.float64, torch.float32)]
        first = torch.stack([(seg[b].cpu() == s).reshape(-1).int().argmax() for s in range(S)])       # a pixel of every present id
        for name, got, r64, r32 in zip(("trav", "loss", "conf"), (trav, loss, conf), *rows):
            _within_bound(f"{seg_type} frame {b} {name}", got[b].reshape(-1).cpu()[first][present], r64[present], r32[present])


def test_conf_state_from_device_memory_and_absent_id(dev):
    B, S, D = 2, 20, 90
    MEAN, STD = 4.0, 1.5                                            # x = 2 randn: reconstruction losses around 4
    m, _ = _model(dev, D, WIDE)
    feat = (2 * torch.randn(B, S, D, generator=g(3)))
    feat[1, 7] = float("nan")                                       # id 7 is absent from frame 1: a NaN row nobody borders
    seg = torch.randint(0, S, (B, 24, 40), generator=g(4), dtype=torch.int32)
    seg[1][seg[1] == 7] = 8
    feat, seg = feat.to(dev), seg.to(dev)
    adj = ops.seg_adjacency_batched(seg, S)
    a = m.forward_per_segment(feat, seg, MEAN, STD, FAC, want_loss=True, adjacency=adj)
    for o in a:
        assert torch.isfinite(o).all()
    assert ((a[1] > 0) & (a[1] < 1)).any()                          # losses inside the confidence window
    state = torch.tensor([MEAN, STD, FAC], dtype=torch.float32, device=dev)
    b = m.forward_per_segment(feat, seg, 123.0, 456.0, 7.0, want_loss=True, conf_state=state, adjacency=adj)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    c = m.forward_per_segment(feat, seg, MEAN, 2 * STD, FAC, adjacency=adj)
    assert c[2] is None and torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    # a frame inside the batch equals the frame alone, through the bitmaps and through its edge list
    for f in range(B):
        alone = m.forward_per_segment(feat[f], seg[f], MEAN, STD, FAC, want_loss=True, adjacency=adj[f:f + 1])
        edges = SegmentExtractor().adjacency_list(seg[f][None, None].long()).t()
        listed = m.forward_per_segment(feat[f], seg[f], MEAN, STD, FAC, want_loss=True, edges=edges)
        for x, y, z in zip(a, alone, listed):
            assert torch.equal(x[f], y) and torch.equal(y, z)


def test_refusals(dev):
    fe = FeatureExtractor(dev, segmentation_type="grid", feature_type="dino", input_size=64, allow_synthetic=True)
    m, _ = _model(dev, fe.feature_dim, WIDE)
    img = torch.rand(1, 3, 64, 64, generator=g(0))
    with pytest.raises(_lib.WvnError, match="SimpleGCN"):
        fe.predict_per_pixel(img, m)
    with pytest.raises(_lib.WvnError, match="SimpleGCN"):
        fe.predict_and_extract(img, m)
    fr = FeatureExtractor(dev, segmentation_type="random", feature_type="dino", input_size=64, allow_synthetic=True)
    with pytest.raises(_lib.WvnError, match="random"):
        fr.predict_per_segment(img, m)
    feat = torch.randn(1, 4, fe.feature_dim, device=dev)
    seg = torch.zeros(1, 8, 8, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.WvnError, match="graph"):
        m.forward_per_segment(feat, seg)
    with pytest.raises(_lib.WvnError):
        m.forward_per_segment(feat, seg, adjacency=torch.zeros(1, 4, 5, dtype=torch.uint8, device=dev))
    with pytest.raises(_lib.WvnError):
        m.forward_per_segment(feat.expand(2, 4, -1), seg.expand(2, 8, 8), edges=torch.zeros(2, 0, dtype=torch.long, device=dev))


# ---- TraversabilityEstimator ------------------------------------------------------------------------------------------------------
def _estimator(dev, D):
    """The configuration keeps the one-step comparison well conditioned.  Adam's first step moves a parameter by
    lr g / (|g| + 1e-8): (a) a stored fp32 parameter of magnitude 0.5 carries a rounding of 2^-26, which is 2^-16 x lr already at
    the default lr = 1e-3, so lr = 0.05 puts the rounding at 3e-7 x lr; (b) the step's sensitivity to a gradient error dg is
    1e-8 dg / (|g| + 1e-8)^2, large only for gradients near zero, so unit loss weights (gradients 30 x the default w_trav's)
    and a small model (205 parameters) leave no such element.  On the CPU the fp32 statement sits at 4e-7 to 2e-6 x lr here."""
    p = ExperimentParams()
    p.model.name = "SimpleGCN"
    p.model.simple_gcn_cfg.input_size = D
    p.model.simple_gcn_cfg.hidden_sizes = [8, 4, 1]
    p.optimizer.lr, p.loss.w_trav, p.loss.w_reco = 0.05, 1.0, 1.0
    return p, TraversabilityEstimator(p, device=dev, min_samples_for_training=2)


def _loss64(out, x, y, yv, p):
    """TraversabilityLoss (utils/loss.py, latest_measurement, anomaly_balanced) on float64 tensors."""
    loss_reco = ((out[:, 1:] - x) ** 2).mean(1)
    with torch.no_grad():
        pos = loss_reco[yv]
        conf = REF.table(out, x, pos.mean().item(), pos.std().item(), p.loss.confidence_std_factor)[2]
    raw = (out[:, 0] - y) ** 2
    trav = torch.where(yv, raw, raw * (1 - conf)).sum() / y.shape[0]
    return p.loss.w_trav * trav + p.loss.w_reco * loss_reco[yv].mean(), raw.mean(), loss_reco[yv].mean()


def test_estimator_trains_and_checkpoints(dev, tmp_path):
    D, S, H = 12, 12, 48
    p, te = _estimator(dev, D)
    assert isinstance(te._model, SimpleGCN) and p.loss.method == "latest_measurement" and p.loss.anomaly_balanced
    gen = g(0)
    for i in range(4):
        n = MissionNode(timestamp=float(i))
        n.features = (2 * torch.randn(S, D, generator=gen)).to(dev)
        n.feature_edges = _random_edges(S, 3, 20 + i).to(dev)
        n.feature_segments = (torch.arange(H * H).reshape(H, H) * S // (H * H)).to(dev)
        mask = torch.full((3, H, H), float("nan"))
        mask[:, : H // 2] = 0.5 + 0.5 * torch.rand(3, H // 2, H, generator=gen)
        assert te.add_mission_node(n)
        te.update_supervision(n, mask.to(dev))
    sd0 = {k: v.detach().cpu().clone() for k, v in te._model.state_dict().items()}
    batches, make = [], te.make_batch
    te.make_batch = lambda bs: batches.append(make(bs)) or batches[-1]
    res = te.train()
    assert te.step == 1 and all(np.isfinite(res[k]) for k in ("loss_total", "loss_trav", "loss_reco")) and res["loss_total"] > 0
    # one float64 Adam step on the reference statement's gradients
    gr = batches[0]
    x, ei, y, yv = gr.x.cpu().double(), gr.edge_index.cpu(), gr.y.cpu().double(), gr.y_valid.cpu()
    sd64 = {k: v.double().requires_grad_() for k, v in sd0.items()}
    total, l_trav, l_reco = _loss64(REF.forward(sd64, x, ei), x, y, yv, p)
    total.backward()
    want = REF.adam_step({k: v.detach() for k, v in sd64.items()}, {k: v.grad for k, v in sd64.items()}, p.optimizer.lr)
    for name, a, b in (("loss_total", res["loss_total"], total), ("loss_trav", res["loss_trav"], l_trav), ("loss_reco", res["loss_reco"], l_reco)):
        assert abs(a - b.item()) <= 2.0 ** -16 * abs(b.item()), (name, a, b.item())
    change = max((want[k] - sd0[k].double()).abs().max().item() for k in sd0)
    err = max((te._model.state_dict()[k].cpu().double() - want[k]).abs().max().item() for k in sd0)
    print(f"one Adam step: err {err:.3e}, max|param change| {change:.3e}")
    assert change > 0 and err <= 2.0 ** -16 * change
    # the HIP forward (no grad) and the grad-enabled statement on the trained weights
    te.make_batch = make
    for _ in range(3):
        te.train()
    assert te.step == 4
    sd = {k: v.detach().cpu() for k, v in te._model.state_dict().items()}
    data = Data(x=gr.x, edge_index=gr.edge_index)
    with torch.no_grad():
        hip = te._model(data)
    stmt = te._model(data).detach()
    ref64, ref32 = REF.forward(sd, gr.x, gr.edge_index), REF.forward(sd, gr.x, gr.edge_index, torch.float32)
    _within_bound("HIP forward on trained weights", hip, ref64, ref32)
    _within_bound("torch statement on trained weights", stmt, ref64, ref32)
    # update_node_confidence, as for the other models
    node = te._mission_graph.get_nodes()[0]
    node.prediction = te._model(Data(x=node.features, edge_index=node.feature_edges)).detach()
    te._traversability_loss.update_node_confidence(node)
    assert node.confidence.shape == (S,) and torch.isfinite(node.confidence).all()
    # checkpoint round trip
    f = te.save_checkpoint(str(tmp_path))
    ck = torch.load(f, weights_only=False)
    assert list(ck["model_state_dict"]) == REF.KEYS
    _, te2 = _estimator(dev, D)
    te2.load_checkpoint(f)
    assert te2.step == 4
    for k, v in te._model.state_dict().items():
        assert torch.equal(v, te2._model.state_dict()[k]), k
