"""Exact dense CRF (csrc/dense_crf.hip, ops.dense_crf, StegoInterface(run_crf=True, crf="exact")) against the float64 statement of the
definition in DESIGN.md "Dense CRF" (the public STEGO crf.py / pydensecrf DenseCRF2D recipe with every pixel pair evaluated).

The fp64 reference below lives here and nowhere else; the CPU tests pin it to a literal O(N^2 K) loop, the GPU tests hold the kernels to it."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from wild_visual_navigation_amd import _lib

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
DEFAULTS = dict(pos_w=3.0, pos_xy_std=1.0, bi_w=4.0, bi_xy_std=67.0, bi_rgb_std=3.0)


def g(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------- fp64 reference -----------------------------------------------------
def _features(H, W, image, dev):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    pos = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)                       # [N, 2]
    col = image.reshape(-1, 3).to(dev, torch.float64)                             # [N, 3]
    return pos, col


def kernel_apply(pos, col, V, xy_std, rgb_std=None, rows=None, chunk=512):
    """sum_j k(i, j) V_j (j == i included) for the query rows ``rows`` (default: all), tiled; V [N, M] float64."""
    N = pos.shape[0]
    idx = torch.arange(N, device=pos.device) if rows is None else rows
    out = torch.empty(idx.numel(), V.shape[1], dtype=torch.float64, device=pos.device)
    for s in range(0, idx.numel(), chunk):
        r = idx[s:s + chunk]
        e = -((pos[r, None, :] - pos[None]).square().sum(-1)) / (2 * xy_std ** 2)
        if rgb_std is not None:
            e = e - (col[r, None, :] - col[None]).square().sum(-1) / (2 * rgb_std ** 2)
        out[s:s + chunk] = torch.exp(e) @ V
    return out


def unary64(logits):
    """logits [K, N] -> -U = log(clip(softmax(L), 1e-5, 1)) [N, K] float64."""
    p = torch.softmax(logits.double(), 0)
    return torch.log(p.clamp(1e-5, 1.0)).T.contiguous()


def crf_ref(logits, image, iterations=10, pos_w=3.0, pos_xy_std=1.0, bi_w=4.0, bi_xy_std=67.0, bi_rgb_std=3.0, parts=False):
    """logits [K, H, W], image u8 [H, W, 3] -> Q^T [K, H, W] float64 (and, with ``parts``, the first iteration's pieces)."""
    K, H, W = logits.shape
    dev = logits.device
    pos, col = _features(H, W, image, dev)
    N = H * W
    ones = torch.ones(N, 1, dtype=torch.float64, device=dev)
    n_g = (kernel_apply(pos, col, ones, pos_xy_std)[:, 0] + 1e-20).rsqrt()
    n_b = (kernel_apply(pos, col, ones, bi_xy_std, bi_rgb_std)[:, 0] + 1e-20).rsqrt()
    negU = unary64(logits.reshape(K, N))
    Q = torch.softmax(negU, 1)
    first = None
    for t in range(iterations):
        mg = n_g[:, None] * kernel_apply(pos, col, n_g[:, None] * Q, pos_xy_std)
        mb = n_b[:, None] * kernel_apply(pos, col, n_b[:, None] * Q, bi_xy_std, bi_rgb_std)
        if first is None:
            first = dict(n_g=n_g, n_b=n_b, msg_g=mg, msg_b=mb, Q0=Q)
        Q = torch.softmax(negU + pos_w * mg + bi_w * mb, 1)
    Q = Q.T.reshape(K, H, W)
    return (Q, first) if parts else Q


def crf_literal(logits, image, iterations, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std):
    """The definition as a literal O(N^2 K) loop in Python floats (tiny images only)."""
    K, H, W = logits.shape
    N = H * W
    px = [(i % W, i // W) for i in range(N)]
    rgb = [[float(image[i // W, i % W, c]) for c in range(3)] for i in range(N)]

    def kg(i, j):
        return math.exp(-((px[i][0] - px[j][0]) ** 2 + (px[i][1] - px[j][1]) ** 2) / (2 * pos_xy_std ** 2))

    def kb(i, j):
        d = (px[i][0] - px[j][0]) ** 2 + (px[i][1] - px[j][1]) ** 2
        c = sum((rgb[i][k] - rgb[j][k]) ** 2 for k in range(3))
        return math.exp(-d / (2 * bi_xy_std ** 2) - c / (2 * bi_rgb_std ** 2))

    def softmax(v):
        m = max(v)
        e = [math.exp(x - m) for x in v]
        s = sum(e)
        return [x / s for x in e]

    ng = [1 / math.sqrt(sum(kg(i, j) for j in range(N)) + 1e-20) for i in range(N)]
    nb = [1 / math.sqrt(sum(kb(i, j) for j in range(N)) + 1e-20) for i in range(N)]
    L = logits.reshape(K, N)
    negU = []
    for i in range(N):
        p = softmax([float(L[k, i]) for k in range(K)])
        negU.append([math.log(min(max(x, 1e-5), 1.0)) for x in p])
    Q = [softmax(u) for u in negU]
    for _ in range(iterations):
        new = []
        for i in range(N):
            v = []
            for k in range(K):
                mg = ng[i] * sum(kg(i, j) * ng[j] * Q[j][k] for j in range(N))
                mb = nb[i] * sum(kb(i, j) * nb[j] * Q[j][k] for j in range(N))
                v.append(negU[i][k] + pos_w * mg + bi_w * mb)
            new.append(softmax(v))
        Q = new
    return torch.tensor(Q, dtype=torch.float64).T.reshape(K, H, W)


def crf_image_ref(frame, size=None):
    """torch fp32 restatement of STEGO dense_crf's image: to_pil_image(UnNormalize(Normalize(x))) on the resized, cropped frame."""
    from wild_visual_navigation_amd.feature_extractor.transforms import resize_nearest_center_crop

    x = frame.float() / 255 if frame.dtype == torch.uint8 else frame.float()
    if size is not None:
        x = resize_nearest_center_crop(x, size)
    m = torch.tensor(MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.tensor(STD, dtype=torch.float32).view(1, 3, 1, 1)
    n = (x - m) / s
    r = n * s
    r = r + m
    return (r * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def blocky_image(H, W, seed, levels=4, noise=4):
    """piecewise-constant colour regions plus noise: the bilateral term matters."""
    gen = g(seed)
    by, bx = max(1, H // 3), max(1, W // 4)
    base = torch.randint(0, 256, (levels, 3), generator=gen)
    ids = torch.randint(0, levels, ((H + by - 1) // by, (W + bx - 1) // bx), generator=gen)
    ids = ids.repeat_interleave(by, 0).repeat_interleave(bx, 1)[:H, :W]
    img = base[ids] + torch.randint(-noise, noise + 1, (H, W, 3), generator=gen)
    return img.clamp(0, 255).to(torch.uint8)


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_dense_crf_symbols_are_exported_and_bound():
    for name in ("wvn_dense_crf", "wvn_dense_crf_workspace_bytes", "wvn_crf_image"):
        assert name in _lib.EXPORTED_SYMBOLS
    h = _lib.lib()
    assert h.wvn_dense_crf_workspace_bytes(2, 40, 56, 27) > 0
    assert h.wvn_dense_crf_workspace_bytes(1, 40, 56, 0) == 0
    assert h.wvn_dense_crf_workspace_bytes(1, 40, 56, 65) == 0


def test_dense_crf_rejects_bad_arguments_without_the_gpu():
    h = _lib.lib()
    buf = C.create_string_buffer(1 << 16)
    p = C.addressof(buf)
    ws = h.wvn_dense_crf_workspace_bytes(1, 8, 8, 4)

    def call(l1=p, K1=4, l2=0, K2=0, img=p, B=1, H=8, W=8, T=10, pos_std=1.0, bi_std=67.0, rgb_std=3.0, labels=p, nseg=0, probs=0,
             work=p, nbytes=ws, pos_w=3.0):
        return h.wvn_dense_crf(l1, K1, 64 * K1, 64, 1, l2, K2, 64 * max(K2, 1), 64, 1, img, B, H, W, T, pos_w, pos_std, 4.0, bi_std, rgb_std,
                               labels, nseg, probs, 0, work, nbytes, None)

    ARG = 1001
    assert call(K1=0) == ARG
    assert call(K1=65) == ARG
    assert call(K1=40, l2=p, K2=30) == ARG                    # 70 columns in all
    assert call(K2=3) == ARG                                   # K2 without its logits
    assert call(l2=p) == ARG                                   # logits without columns
    assert call(l1=0) == ARG
    assert call(img=0) == ARG
    assert call(work=0) == ARG
    assert call(labels=0) == ARG                               # nothing to write
    assert call(labels=0, nseg=p, probs=p) == ARG              # relabel needs labels
    assert call(B=0) == ARG and call(H=0) == ARG and call(W=-3) == ARG and call(H=4096) == ARG
    assert call(T=0) == ARG
    assert call(pos_std=0.0) == ARG and call(pos_std=5.0) == ARG and call(rgb_std=-1.0) == ARG and call(bi_std=float("inf")) == ARG
    assert call(pos_w=float("nan")) == ARG
    assert call(nbytes=ws - 1) == 1002                         # WVN_ERR_WORKSPACE
    assert h.wvn_crf_image(0, 1, 1, 8, 8, 0, 0, 8, 8, p, None) == ARG
    assert h.wvn_crf_image(p, 1, 1, 8, 8, 0, 0, 4, 4, p, None) == ARG   # resizing needs the tables
    assert h.wvn_crf_image(p, 1, 1, 8, 8, p, 0, 8, 8, p, None) == ARG


def test_fp64_reference_matches_the_literal_loop():
    H, W, K = 8, 8, 3
    logits = torch.randn(K, H, W, generator=g(0), dtype=torch.float64) * 2
    image = blocky_image(H, W, 1)
    params = dict(pos_w=3.0, pos_xy_std=1.0, bi_w=4.0, bi_xy_std=3.0, bi_rgb_std=20.0)   # a short appearance range: both kernels matter on 8x8
    want = crf_literal(logits, image, 2, **params)
    got = crf_ref(logits, image, 2, **params)
    assert (got - want).abs().max().item() < 1e-12
    # the definition's defaults as well
    assert (crf_ref(logits, image, 2, **DEFAULTS) - crf_literal(logits, image, 2, **DEFAULTS)).abs().max().item() < 1e-12


def test_stego_interface_crf_refusals():
    from wild_visual_navigation_amd.feature_extractor.stego_interface import StegoInterface

    with pytest.raises(_lib.WvnError, match="skip_crf"):
        StegoInterface("cpu", input_size=64, run_crf=True, crf="exact", skip_crf=True, allow_synthetic=True)
    with pytest.raises(_lib.WvnError, match="cluster_resolution"):
        StegoInterface("cpu", input_size=64, run_crf=True, crf="exact", cluster_resolution="patch", allow_synthetic=True)
    with pytest.raises(_lib.WvnError, match="code_align_corners"):
        StegoInterface("cpu", input_size=64, run_crf=True, crf="exact", code_align_corners=False, allow_synthetic=True)
    with pytest.raises(_lib.WvnError, match="crf"):
        StegoInterface("cpu", input_size=64, run_crf=True, crf="lattice", allow_synthetic=True)
    with pytest.raises(_lib.WvnError, match="skip_crf"):                      # unchanged: run_crf=True without crf= still refuses
        StegoInterface("cpu", input_size=64, run_crf=True, skip_crf=False, allow_synthetic=True)


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _rel_message_error(got, want, scale):
    """|got - want| / the message of unit values (the scale every column of the message lives on)."""
    return ((got - want).abs() / scale[:, None]).max().item()


@pytest.mark.gpu
def test_crf_image_is_bit_identical(dev, golden):
    from wild_visual_navigation_amd import ops

    frames = golden("demo_frames_224.pt")["frames_u8"]
    assert torch.equal(ops.crf_image(frames.to(dev)).cpu(), crf_image_ref(frames))
    assert torch.equal(ops.crf_image(frames.to(dev), 160).cpu(), crf_image_ref(frames, 160))
    # fp32 frames, every level k / 255 (255 x integral) and random values, camera-sized through the resize / crop tables
    lv = (torch.arange(256, dtype=torch.float32) / 255).repeat(3 * 90 * 120 // 256 + 1)[: 3 * 90 * 120].reshape(1, 3, 90, 120)
    rnd = torch.rand(2, 3, 90, 120, generator=g(5))
    fr = torch.cat([lv, rnd])
    assert torch.equal(ops.crf_image(fr.to(dev), 64).cpu(), crf_image_ref(fr, 64))
    assert torch.equal(ops.crf_image(fr.to(dev)).cpu(), crf_image_ref(fr))
    u8 = torch.randint(0, 256, (2, 3, 90, 120), generator=g(6), dtype=torch.uint8)
    assert torch.equal(ops.crf_image(u8.to(dev), 64).cpu(), crf_image_ref(u8, 64))
    # the round trip is not the identity: some integral levels drop by one
    assert (crf_image_ref(lv).int() != (lv * 255).round().int().permute(0, 2, 3, 1)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(64, 64), (40, 56), (97, 131)])
def test_normalisers_and_one_iteration_messages(dev, H, W):
    from wild_visual_navigation_amd import ops

    K = 5
    image = blocky_image(H, W, H + W)
    logits = torch.randn(1, K, H, W, generator=g(H)) * 2
    _, _, dbg = ops.dense_crf(logits.to(dev), image[None].to(dev), iterations=1, return_probs=True, _debug=True)
    dbg = dbg[0].reshape(dbg.shape[1], H * W).double()
    KP = 32
    _, first = crf_ref(logits[0].double().to(dev), image.to(dev), 1, parts=True)
    nb_err = ((dbg[2 * KP] - first["n_b"]).abs() / first["n_b"]).max().item()
    ng_err = ((dbg[2 * KP + 1] - first["n_g"]).abs() / first["n_g"]).max().item()
    assert nb_err <= 1e-5 and ng_err <= 1e-5, (nb_err, ng_err)
    pos, col = _features(H, W, image, dev)
    scale_b = first["n_b"] * kernel_apply(pos, col, first["n_b"][:, None], 67.0, 3.0)[:, 0]
    scale_g = first["n_g"] * kernel_apply(pos, col, first["n_g"][:, None], 1.0)[:, 0]
    eb = _rel_message_error(dbg[:K].T, first["msg_b"], scale_b)
    eg = _rel_message_error(dbg[KP:KP + K].T, first["msg_g"], scale_g)
    assert eb <= 1e-5 and eg <= 1e-5, (eb, eg)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 27, 40, 64])
def test_ten_iterations_against_fp64(dev, K):
    from wild_visual_navigation_amd import ops

    H, W = 40, 52
    image = blocky_image(H, W, K)
    logits = torch.randn(1, K, H, W, generator=g(K)) * 1.5
    lab, Q = ops.dense_crf(logits.to(dev), image[None].to(dev), return_probs=True)
    Q64 = crf_ref(logits[0].double().to(dev), image.to(dev))
    err = (Q[0].double() - Q64).abs().max().item()
    assert err <= 1e-4, err
    top2 = Q64.topk(2, 0).values
    margin = top2[0] - top2[1]
    want = Q64.argmax(0)
    bad = (lab[0].long() != want) & (margin >= 1e-4)
    assert not bad.any(), int(bad.sum())


@pytest.mark.gpu
def test_448_sampled_rows_one_iteration(dev):
    from wild_visual_navigation_amd import ops

    S, K = 448, 27
    image = blocky_image(S, S, 448, levels=6)
    logits = torch.randn(1, K, S, S, generator=g(448)) * 2
    _, _, dbg = ops.dense_crf(logits.to(dev), image[None].to(dev), iterations=1, return_probs=True, _debug=True)
    dbg = dbg[0].reshape(dbg.shape[1], S * S).double()
    pos, col = _features(S, S, image, dev)
    N = S * S
    ones = torch.ones(N, 1, dtype=torch.float64, device=dev)
    nb = (kernel_apply(pos, col, ones, 67.0, 3.0, chunk=256)[:, 0] + 1e-20).rsqrt()      # all 200 704 normalisers (needed by every message)
    assert ((dbg[64] - nb).abs() / nb).max().item() <= 1e-5
    rows = torch.randperm(N, generator=g(9))[:2048].to(dev)
    Q0 = torch.softmax(unary64(logits[0].double().to(dev).reshape(K, N)), 1)
    msg = nb[rows, None] * kernel_apply(pos, col, nb[:, None] * Q0, 67.0, 3.0, rows=rows, chunk=256)
    scale = nb[rows] * kernel_apply(pos, col, nb[:, None], 67.0, 3.0, rows=rows, chunk=256)[:, 0]
    err = _rel_message_error(dbg[:K, rows].T, msg, scale)
    assert err <= 1e-5, err


@pytest.mark.gpu
def test_batching_and_shared_pass_are_bit_identical(dev):
    from wild_visual_navigation_amd import ops

    B, H, W = 3, 37, 45
    images = torch.stack([blocky_image(H, W, 30 + b) for b in range(B)]).to(dev)
    la = (torch.randn(B, 7, H, W, generator=g(1)) * 2).to(dev)
    lb = (torch.randn(B, 20, H, W, generator=g(2)) * 2).to(dev)
    lab, Q = ops.dense_crf(la, images, return_probs=True)
    for b in range(B):
        lb1, Qb = ops.dense_crf(la[b:b + 1], images[b:b + 1], return_probs=True)
        assert torch.equal(lab[b:b + 1], lb1) and torch.equal(Q[b:b + 1], Qb)
    # two CRFs in one pass (27 columns): the first group bit for bit as alone (same columns, same order); the second group's softmax
    # sums its columns in another register order, so it agrees to fp32 rounding
    lab2, Q2 = ops.dense_crf((la, lb), images, return_probs=True)
    lab_b, Q_b = ops.dense_crf(lb, images, return_probs=True)
    assert torch.equal(lab2[:, 0], lab) and torch.equal(Q2[:, :7], Q)
    assert (Q2[:, 7:] - Q_b).abs().max().item() <= 1e-6 and (lab2[:, 1] != lab_b).float().mean().item() <= 1e-3
    # strided (pixel-major) logits: the same as their contiguous copy
    pm = la.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert torch.equal(ops.dense_crf(pm, images), lab)


@pytest.mark.gpu
def test_the_crf_follows_the_colour_regions(dev):
    from wild_visual_navigation_amd import ops

    H, W = 48, 64
    truth = torch.zeros(H, W, dtype=torch.long)
    truth[:, W // 2:] = 1
    truth[H // 3: 2 * H // 3, W // 4: W // 2] = 1          # a notch, so that the map is not a half-plane
    image = torch.where(truth[..., None] == 1, torch.tensor([200, 40, 60]), torch.tensor([30, 120, 220]))
    image = (image + torch.randint(-3, 4, (H, W, 3), generator=g(3))).clamp(0, 255).to(torch.uint8)
    logits = torch.stack([(truth == 0).float(), (truth == 1).float()]) * 0.6 + torch.randn(2, H, W, generator=g(4)) * 0.8
    raw = logits.argmax(0)
    lab = ops.dense_crf(logits[None].to(dev), image[None].to(dev))[0].cpu().long()
    raw_acc = (raw == truth).float().mean().item()
    acc = (lab == truth).float().mean().item()
    assert raw_acc < 0.8 and acc > 0.99, (raw_acc, acc)


def _stego(dev, S, run_clustering, n_clusters, K_probe, n_lin=27, seed=0):
    from oracle import interfaces as OI, vit as OV
    from wild_visual_navigation_amd.feature_extractor.stego_interface import StegoInterface

    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=seed, depth=1)
    head = OI.make_stego_head_state_dict(384, 90, seed=seed + 1)
    gen = g(seed + 2)
    probes = {"clusters": torch.randn(K_probe, 90, generator=gen), "linear.weight": torch.randn(n_lin, 90, generator=gen) * 0.3,
              "linear.bias": torch.randn(n_lin, generator=gen) * 0.1}
    return StegoInterface(dev, input_size=S, n_image_clusters=n_clusters, run_clustering=run_clustering, run_crf=True, crf="exact",
                          backbone_weights=sd, head_weights=head, probe_weights=probes, precision="exact", flip_tta=False,
                          cluster_resolution="pixel", allow_synthetic=True), probes


def _up64(t, G, S):
    """[B, G*G, C] -> [B, C, S, S] float64, align_corners=True (the up-sample of the code / the probe logits)."""
    B, _, Cc = t.shape
    return F.interpolate(t.double().reshape(B, G, G, Cc).permute(0, 3, 1, 2), (S, S), mode="bilinear", align_corners=True)


def _check_map(got, Q64, frac=0.999):
    """got int [S, S] vs the fp64 Q [K, S, S]: >= frac equal, every mismatch at a near-tie of the fp64 Q."""
    want = Q64.argmax(0)
    top2 = Q64.topk(2, 0).values
    diff = got.long() != want
    assert 1 - diff.float().mean().item() >= frac
    assert not (diff & (top2[0] - top2[1] >= 1e-3)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("branch", ["probe", "probe_wide", "kmeans"])
def test_stego_interface_exact_crf_branches(dev, branch):
    from wild_visual_navigation_amd import ops

    S, G = 64, 8
    run_clustering = branch == "kmeans"
    K_probe = 40 if branch == "probe_wide" else 12       # 27 + 40 > 64: two passes; 27 + 12: one shared pass
    si, probes = _stego(dev, S, run_clustering, 5, K_probe)
    H = 80                                                # a camera height different from input_size
    img = torch.rand(2, 3, H, 96, generator=g(21))
    lin, clu = si.inference(img.to(dev))
    assert lin.shape == (1, 2, H, H) and clu.shape == (1, 2, H, H)
    code = si.feature_tokens
    image = crf_image_ref(img, S)
    upc = _up64(code, G, S)                               # [2, 90, S, S]
    pixn = upc / upc.norm(dim=1, keepdim=True).clamp_min(1e-12)
    lin_logits = _up64(code.double() @ probes["linear.weight"].double().to(dev).T + probes["linear.bias"].double().to(dev), G, S)
    if run_clustering:
        _, _, cent = ops.kmeans_cosine_pixels(code, G, S, 5, 10, relabel=False, return_centroids=True)
        cents = [cent[b].double() for b in range(2)]
    else:
        cents = [probes["clusters"].double().to(dev)] * 2
    nseg = si._n_segments
    for b in range(2):
        c = cents[b] / cents[b].norm(dim=1, keepdim=True).clamp_min(1e-12)
        clu_logits = 2 * torch.einsum("chw,kc->khw", pixn[b], c)
        Ql = crf_ref(lin_logits[b], image[b].to(dev))
        Qc = crf_ref(clu_logits, image[b].to(dev))
        # compared at the CRF's own resolution: every S x S pixel survives the nearest resample to H > S
        _check_map(_down(lin[0, b], S, H), Ql)
        got_c = _down(clu[0, b], S, H)
        if run_clustering:
            ids = torch.unique(got_c)
            assert int(nseg[b]) == ids.numel() and torch.equal(ids.cpu(), torch.arange(ids.numel(), dtype=ids.dtype))
            # undo the ascending relabel to compare against the fp64 map over the k-means ids
            want_ids = torch.unique(Qc.argmax(0))
            if want_ids.numel() == ids.numel():
                got_c = want_ids[got_c.long()]
        else:
            assert nseg is None
        _check_map(got_c, Qc)


def _down(m, S, H):
    """the S x S map back from its nearest resample to H x H (pixel y of the S map is the sample at floor(y * H / S) of the H map's source):
    every S pixel appears in the H map; read it at the first H position that maps to it."""
    idx = torch.arange(H, device=m.device) * S // H
    first = torch.full((S,), -1, dtype=torch.long, device=m.device)
    for h in range(H - 1, -1, -1):
        first[idx[h]] = h
    assert (first >= 0).all()
    return m[first][:, first]


@pytest.mark.gpu
def test_feature_extractor_stego_with_exact_crf(dev):
    from oracle import interfaces as OI, vit as OV
    from wild_visual_navigation_amd.feature_extractor import FeatureExtractor

    S = 64
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=3, depth=1)
    head = OI.make_stego_head_state_dict(384, 90, seed=4)
    fe = FeatureExtractor(dev, segmentation_type="stego", feature_type="stego", input_size=S, run_crf=True, crf="exact", pretrained_weights=sd,
                          head_weights=head, n_image_clusters=6, precision="exact", flip_tta=False, allow_synthetic=True)
    img = torch.rand(1, 3, S, S, generator=g(8)).to(dev)
    edges, feat, seg, center, _ = fe.extract(img)
    ids = torch.unique(seg)
    assert torch.equal(ids.cpu(), torch.arange(ids.numel(), dtype=ids.dtype))
    assert feat.shape == (ids.numel(), 90) and torch.isfinite(feat).all()
