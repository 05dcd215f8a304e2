"""End-to-end parity of the HIP backbone / interfaces / FeatureExtractor against the CPU oracle on the
same seeded inputs and weights, plus size-independent properties at BASELINE.json's full size.

Tolerances: exact mode (fp32 storage + fp32 FMA) <= 1e-3 absolute on un-normalised final features
(north_star); bf16 MFMA mode is compared at the tolerance bf16 operand rounding allows (stated per
test) -- it is the speed path, the fp32 mode is the parity gate.  Segment-index maps: bit-exact."""
import numpy as np
import pytest
import torch

from oracle import interfaces as OI, kmeans_linear as KL, segments as OS, vit as OV
from wild_visual_navigation_amd import ops
from wild_visual_navigation_amd.backbone import VitBackbone
from wild_visual_navigation_amd.feature_extractor import DinoInterface, FeatureExtractor, StegoInterface

pytestmark = pytest.mark.gpu


def g(seed):
    return torch.Generator().manual_seed(seed)


def rel_l2(a, b):
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("S,depth,B", [(64, 2, 3), (224, 12, 2), (448, 12, 1)])
def test_vit_exact_mode_within_1e3(dev, S, depth, B):
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=0, depth=depth)
    img = torch.rand(B, 3, S, S, generator=g(1))
    want = OV.vit_tokens(sd, OI.normalize(img), 8, 6)[:, 1:]
    bb = VitBackbone(sd, S, 8, 6, device=dev, precision="fp32", max_chunk=2)
    got = bb.forward_tokens(img.to(dev)).cpu()
    err = (got - want).abs().max().item()
    assert err < 1e-3, f"exact-mode tokens differ by {err}"
    feat = bb.forward(img.to(dev)).cpu()
    assert torch.equal(feat, got.reshape(B, S // 8, S // 8, 384).permute(0, 3, 1, 2))


@pytest.mark.parametrize("S,depth,B", [(64, 2, 3), (224, 12, 2), (448, 12, 1)])
def test_vit_bf16_mode(dev, S, depth, B):
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=0, depth=depth)
    img = torch.rand(B, 3, S, S, generator=g(1))
    want = OV.vit_tokens(sd, OI.normalize(img), 8, 6)[:, 1:]
    bb = VitBackbone(sd, S, 8, 6, device=dev, precision="bf16", max_chunk=2)
    got = bb.forward_tokens(img.to(dev)).cpu()
    # bf16 operands (2^-9 relative rounding per GEMM input) through `depth` residual blocks; outputs are
    # LayerNorm'ed (O(1) magnitudes).  Gates at about twice the measured error (printed; 12 blocks at 448^2: max 3.0e-2,
    # rel-L2 5.0e-3 -- bench.py `parity`): a 2x accuracy regression fails.
    print(f"bf16 tokens S={S} depth={depth}: max|err| {(got - want).abs().max().item():.3e} rel-L2 {rel_l2(got, want):.3e}")
    assert rel_l2(got, want) < 1.0e-2 and (got - want).abs().max().item() < 0.06
    cos = torch.nn.functional.cosine_similarity(got.reshape(-1, 384), want.reshape(-1, 384), dim=1)
    assert cos.min().item() > 0.995


@pytest.mark.parametrize("fuse_mlp,fuse_qkv", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("S,B", [(64, 3), (224, 2)])
def test_fused_block_kernels_agree_with_separate_kernels(dev, S, B, fuse_mlp, fuse_qkv):
    """The shipped bf16 ViT-S path runs LayerNorm + QKV and LayerNorm + fc1 + GELU + fc2 as single kernels (csrc/qkv_fused.hip,
    csrc/mlp_fused.hip); with the switches off it runs the LayerNorm kernel and the GEMM kernels.  Same rounding points, other
    summation orders: both must sit inside the oracle tolerance and within bf16 noise of each other."""
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=0, depth=12)
    img = torch.rand(B, 3, S, S, generator=g(7))
    want = OV.vit_tokens(sd, OI.normalize(img), 8, 6)[:, 1:]
    default = VitBackbone(sd, S, 8, 6, device=dev, precision="bf16")
    assert default.fuse_mlp and default.fuse_qkv          # allowed; used from about half a chip of row blocks on (csrc/vit_forward.hip)
    fused = VitBackbone(sd, S, 8, 6, device=dev, precision="bf16", fuse_mlp=True, fuse_qkv=True)   # explicit True: at every size
    a = fused.forward_tokens(img.to(dev)).cpu()
    if not (fuse_mlp or fuse_qkv):   # at these sizes the default takes the separate kernels: bit-identical to asking for them
        assert torch.equal(default.forward_tokens(img.to(dev)).cpu(),
                           VitBackbone(sd, S, 8, 6, device=dev, precision="bf16", fuse_mlp=False, fuse_qkv=False).forward_tokens(img.to(dev)).cpu())
    b = VitBackbone(sd, S, 8, 6, device=dev, precision="bf16", fuse_mlp=fuse_mlp or False, fuse_qkv=fuse_qkv or False).forward_tokens(img.to(dev)).cpu()
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert rel_l2(a, want) < 2.5e-2 and rel_l2(b, want) < 2.5e-2
    assert rel_l2(a, b) < 1.5e-2   # two bf16 paths differ from each other by about what each differs from fp32
    with pytest.raises(Exception):
        VitBackbone(sd, S, 8, 6, device=dev, precision="fp32", fuse_mlp=True)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_layernorm_handover_between_blocks(dev, monkeypatch, prec):
    """Where the block kernels run, block i's projection + MLP kernel keeps the residual rows in its accumulators and hands block
    i + 1 its norm1 output as operand fragments (include/wvn_hip.h: fc1_w_fused / qkv_w_fused).  Same rounding points as the forms
    without it (WVN_NO_HANDOVER: LayerNorm inside the QKV kernel; WVN_NO_RESIDENT: rows through memory twice per block), other
    summation orders; all three inside the oracle tolerance, and the chunked call (state per launch sequence) equals the whole one."""
    S, B = 224, 5
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=3, depth=12)
    img = torch.rand(B, 3, S, S, generator=g(17))
    want = OV.vit_tokens(sd, OI.normalize(img), 8, 6)[:, 1:]
    kw = dict(device=dev, precision=prec, fuse_mlp=True, fuse_qkv=True)
    a = VitBackbone(sd, S, 8, 6, max_chunk=8, **kw).forward_tokens(img.to(dev)).cpu()
    chunked = VitBackbone(sd, S, 8, 6, max_chunk=2, **kw).forward_tokens(img.to(dev)).cpu()     # 2 + 2 + 1 frames
    monkeypatch.setenv("WVN_NO_HANDOVER", "1")
    b = VitBackbone(sd, S, 8, 6, max_chunk=8, **kw).forward_tokens(img.to(dev)).cpu()
    monkeypatch.setenv("WVN_NO_RESIDENT", "1")
    c = VitBackbone(sd, S, 8, 6, max_chunk=8, **kw).forward_tokens(img.to(dev)).cpu()
    gate = 2.5e-2 if prec == "bf16" else 3e-3
    for t in (a, b, c, chunked):
        assert torch.isfinite(t).all() and rel_l2(t, want) < gate
    assert not torch.equal(a, b) and not torch.equal(b, c)      # three different kernel sequences did run
    assert rel_l2(a, b) < gate and rel_l2(a, c) < gate
    assert rel_l2(a, chunked) < gate * 0.5
    monkeypatch.delenv("WVN_NO_HANDOVER")
    monkeypatch.delenv("WVN_NO_RESIDENT")
    a2 = VitBackbone(sd, S, 8, 6, max_chunk=8, **kw).forward_tokens(img.to(dev)).cpu()
    assert torch.equal(a, a2), "run-to-run difference"


def test_fused_kernels_take_over_at_batch_size(dev):
    """From about half a chip of row blocks on wvn_vit_forward switches to the single-kernel block stages by itself: a 12-frame
    448^2 batch runs them (same tokens as forcing them), a 2-frame batch does not (same tokens as forbidding them)."""
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=0, depth=2)
    img = torch.rand(12, 3, 448, 448, generator=g(9)).to(dev)
    auto = VitBackbone(sd, 448, 8, 6, device=dev, precision="bf16", max_chunk=12)
    forced = VitBackbone(sd, 448, 8, 6, device=dev, precision="bf16", max_chunk=12, fuse_mlp=True, fuse_qkv=True)
    never = VitBackbone(sd, 448, 8, 6, device=dev, precision="bf16", max_chunk=12, fuse_mlp=False, fuse_qkv=False)
    t_auto, t_forced, t_never = auto.forward_tokens(img), forced.forward_tokens(img), never.forward_tokens(img)
    assert torch.equal(t_auto, t_forced) and not torch.equal(t_auto, t_never)
    assert rel_l2(t_auto.float().cpu(), t_never.float().cpu()) < 1.5e-2
    assert torch.equal(auto.forward_tokens(img[:2]), never.forward_tokens(img[:2]))


def test_batch_invariance_and_chunking(dev):
    """A frame's features must not depend on its batch neighbours or on the chunking (bit-exact)."""
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=0, depth=3)
    img = torch.rand(5, 3, 64, 64, generator=g(2)).to(dev)
    for prec in ("bf16", "fp32"):
        a = VitBackbone(sd, 64, 8, 6, device=dev, precision=prec, max_chunk=5).forward_tokens(img)
        b = VitBackbone(sd, 64, 8, 6, device=dev, precision=prec, max_chunk=2).forward_tokens(img)
        c = VitBackbone(sd, 64, 8, 6, device=dev, precision=prec, max_chunk=1).forward_tokens(img[3:4])
        assert torch.equal(a, b) and torch.equal(a[3:4], c), prec


def test_uint8_frames_equal_float_frames(dev, golden):
    """Frame ingest: the reference's callers turn 8-bit camera frames into fp32/255 on the host
    (quick_start.py:160-161, ros_converter.py:113-126); handing the uint8 frame straight to the drop-in classes gives
    bit-identical features in the bf16 mode (fused) and in the exact mode (converted on the GPU)."""
    frames = golden("demo_frames_224.pt")["frames_u8"][:2].to(dev)                      # [2,3,224,299]-like uint8
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=5, depth=2)
    for prec in ("bf16", "fp32"):
        di = DinoInterface(dev, input_size=224, backbone_type="vit_small", patch_size=8, pretrained_weights=sd, precision=prec)
        a = di.inference_tokens(frames.float() / 255)
        b = di.inference_tokens(frames)
        assert torch.equal(a, b), prec
    fe = FeatureExtractor(device=dev, segmentation_type="grid", feature_type="dino", patch_size=8, backbone_type="vit_small",
                          input_size=224, pretrained_weights=sd, precision="bf16")
    fa = fe.extract(img=frames[:1].float() / 255)
    fb = fe.extract(img=frames[:1])
    assert torch.equal(fa[2], fb[2]) and torch.equal(fa[0], fb[0])
    assert (fa[1] - fb[1]).abs().max().item() < 1e-5      # same tokens; the generic segment mean sums with atomics


@pytest.mark.parametrize("seg,ftype", [("stego", "stego"), ("grid", "dino")])
def test_two_stage_extract_batch_is_the_same_computation(dev, seg, ftype):
    """backbone_stage + extract_batch(backbone_out=...) (the split bench.py pipelines over two HIP streams) must give
    exactly what the one-call form gives, also when the first stage ran on another stream."""
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=11, depth=2)
    fe = FeatureExtractor(device=dev, segmentation_type=seg, feature_type=ftype, patch_size=8, backbone_type="vit_small",
                          input_size=64, pretrained_weights=sd, precision="bf16", n_image_clusters=6)
    img = torch.rand(3, 3, 64, 64, generator=g(12)).to(dev)
    feat, segm, nseg = fe.extract_batch(img)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tok = fe.backbone_stage(img)
        tok.record_stream(torch.cuda.current_stream())
    torch.cuda.current_stream().wait_stream(side)
    feat2, segm2, nseg2 = fe.extract_batch(img, backbone_out=tok)
    assert torch.equal(segm, segm2) and torch.equal(nseg, nseg2)
    assert torch.equal(torch.nan_to_num(feat, nan=-7.0), torch.nan_to_num(feat2, nan=-7.0))


def test_dino_interface_inference_matches_oracle(dev):
    """Non-square frame like assets/demo_data (299x224): resize(NEAREST)+center-crop, normalise, backbone,
    bilinear(align_corners) to (H, H)."""
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=3, depth=2)
    img = torch.rand(1, 3, 224, 299, generator=g(4))
    want = OI.dino_inference(sd, img, 224, 8, 6)
    di = DinoInterface(dev, input_size=224, backbone_type="vit_small", patch_size=8, pretrained_weights=sd,
                       precision="fp32")
    got = di.inference(img.to(dev)).cpu()
    assert got.shape == (1, 384, 224, 224) and (got - want).abs().max().item() < 1e-3
    assert di.input_size == 224 and di.vit_patch_size == 8 and di.backbone == "dino" and di.backbone_type == "vit_small"


@pytest.mark.parametrize("prec,tol", [("fp32", 1e-3), ("bf16", 0.2)])
def test_feature_extractor_grid_and_random(dev, prec, tol):
    S = 224
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=5, depth=2)
    img = torch.rand(1, 3, S, S, generator=g(6))
    dense = OI.dino_inference(sd, img, S, 8, 6)
    fe = FeatureExtractor(dev, segmentation_type="grid", feature_type="dino", input_size=S, backbone_type="vit_small",
                          patch_size=8, pretrained_weights=sd, precision=prec)
    edges, feat, seg, center, dfeat = fe.extract(img.to(dev), return_dense_features=True)
    oseg = OS.segment_grid(S, S, 32)
    assert torch.equal(seg.cpu(), oseg[0, 0])  # segment-index map: bit-exact
    assert torch.equal(edges.cpu(), OS.adjacency_list(oseg).T)
    assert torch.allclose(center.cpu(), OS.centers(oseg), atol=1e-4)
    assert (feat.cpu() - OS.sparsify_features(dense, oseg[0, 0])).abs().max().item() < tol
    assert (dfeat.cpu() - dense).abs().max().item() < tol
    assert fe.feature_dim == 384 and fe.feature_type == "dino" and fe.segmentation_type == "grid"
    # public sparsify_features on an explicit dense map == reference semantics
    sp = fe.sparsify_features(dfeat, seg)
    assert (sp.cpu() - OS.sparsify_features(dfeat.cpu(), seg.cpu())).abs().max().item() < 1e-4
    # random-pixel mode (feature_extractor.py:96-111)
    fr = FeatureExtractor(dev, segmentation_type="random", feature_type="dino", input_size=S,
                          backbone_type="vit_small", patch_size=8, pretrained_weights=sd, precision=prec)
    e2, f2, s2, c2, d2 = fr.extract(img.to(dev), n_random_pixels=100)
    assert e2 is None and c2 is None and d2 is None and f2.shape == (100, 384)
    s2 = s2.cpu()
    idx = torch.stack([(s2.reshape(-1) == j).nonzero()[0, 0] for j in range(100)])
    assert (s2 >= 0).sum() == 100
    assert (f2.cpu() - dense[0].reshape(384, -1)[:, idx].T).abs().max().item() < tol


@pytest.mark.parametrize("reading", ["upstream", "cheap"])
def test_feature_extractor_stego_pipeline(dev, reading):
    """feature_type = segmentation_type = 'stego' (the reference's ROS default): code, k-means segment map (bit-exact given the
    GPU's own fp32 code), relabel, pooled 90-d features -- under the class DEFAULTS (the upstream reading: flip-averaged code,
    k-means over the code pixels) and under the documented cheap options (single pass, k-means over the patch codes)."""
    S, K = 224, 20
    G = S // 8
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=7, depth=2)
    head = OI.make_stego_head_state_dict(384, 90, seed=0)
    img = torch.rand(1, 3, S, S, generator=g(8))
    tok = OV.vit_tokens(sd, OI.normalize(img), 8, 6)[:, 1:]
    if reading == "upstream":
        code_ref = OI.stego_code_flip_average(head, tok, OV.vit_tokens(sd, OI.normalize(img).flip(-1), 8, 6)[:, 1:], G)
        opts = {}
    else:
        code_ref = OI.stego_code_tokens(head, tok)  # [1, P, 90]
        opts = dict(flip_tta=False, cluster_resolution="patch")
    for prec, tol in (("fp32", 1e-3), ("bf16", 0.25)):
        fe = FeatureExtractor(dev, segmentation_type="stego", feature_type="stego", input_size=S,
                              backbone_type="vit_small", patch_size=8, pretrained_weights=sd, head_weights=head,
                              n_image_clusters=K, precision=prec, **opts)
        edges, feat, seg, center, dense = fe.extract(img.to(dev), return_dense_features=True)
        code = fe._extractor.feature_tokens.cpu()
        assert (code - code_ref).abs().max().item() < tol, prec
        # integer outputs: oracle clustering of the SAME fp32 code must agree bit-for-bit
        if reading == "upstream":
            lab = OI.relabel_ascending(KL.kmeans_cosine_labels_pixels_linear(code[0].numpy(), G, S, K))
            want_seg = torch.from_numpy(lab).reshape(S, S).long()
        else:
            lab = OI.relabel_ascending(OI.kmeans_cosine_labels(code[0].numpy(), K))
            want_seg = OI.upsample_nearest(torch.from_numpy(lab).reshape(1, G, G).int(), S)[0, 0].long()
        assert torch.equal(seg.cpu(), want_seg), prec
        n_seg = int(want_seg.max()) + 1
        assert feat.shape == (n_seg, 90) and center.shape == (n_seg, 2)
        dense_ref = OI.upsample_bilinear_ac(code.reshape(1, G, G, 90).permute(0, 3, 1, 2), S)
        assert (dense.cpu() - dense_ref).abs().max().item() < 1e-4
        assert (feat.cpu() - OS.sparsify_features(dense_ref, want_seg)).abs().max().item() < 1e-4
        assert torch.equal(edges.cpu(), OS.adjacency_list(want_seg[None, None]).T)
        assert fe.feature_dim == 90


def test_stego_interface_contract(dev):
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=9, depth=1)
    si = StegoInterface(dev, input_size=64, n_image_clusters=6, run_crf=False, run_clustering=True,
                        backbone_weights=sd, precision="fp32")
    lin, clu = si.inference(torch.rand(2, 3, 64, 64, generator=g(1)).to(dev))
    assert lin is None                                      # no linear probe was given: nothing is invented for it
    assert clu.shape == (1, 2, 64, 64) and clu.dtype == torch.int32
    assert si.features.shape == (2, 90, 64, 64) and si.cluster_segments is clu and si.linear_segments is None
    assert int(clu.min()) == 0 and int(clu.max()) < 6


def _lightning_ckpt(sd, head, clusters, lin_w, lin_b, layout):
    """A Stego.load_from_checkpoint-style file (stego_interface.py:43) in the upstream STEGO key layout (``net.model.*``,
    ``net.cluster1/2.*`` as 1x1 convolutions, ``cluster_probe.clusters``, ``linear_probe.*``) or the
    self_supervised_segmentation one (``backbone.*``, ``segmentation_head.linear/nonlinear.*``)."""
    out = {}
    bb, c1, c2 = ("net.model.", "net.cluster1.", "net.cluster2.") if layout == "stego" else \
                 ("backbone.model.", "segmentation_head.linear.", "segmentation_head.nonlinear.")
    for k, v in sd.items():
        out[bb + k] = v
    conv = lambda w: w[:, :, None, None]
    out[c1 + "0.weight"], out[c1 + "0.bias"] = conv(head["cluster1.0.weight"]), head["cluster1.0.bias"]
    out[c2 + "0.weight"], out[c2 + "0.bias"] = conv(head["cluster2.0.weight"]), head["cluster2.0.bias"]
    out[c2 + "2.weight"], out[c2 + "2.bias"] = conv(head["cluster2.2.weight"]), head["cluster2.2.bias"]
    out["cluster_probe.clusters"] = clusters
    out["linear_probe.weight"], out["linear_probe.bias"] = conv(lin_w), lin_b
    return {"state_dict": out, "hyper_parameters": {"n_classes": lin_w.shape[0]}}


@pytest.mark.parametrize("layout,prec", [("stego", "fp32"), ("sss", "exact"), ("stego", "bf16")])
def test_stego_checkpoint_probes_flip_tta_and_pixel_clustering(dev, tmp_path, layout, prec):
    """StegoInterface(model_path=...) (stego_interface.py:23,43): backbone + head + cluster probe + linear probe come from the
    Lightning checkpoint; run_clustering=False labels with the learned cluster probe (cosine argmax), the linear probe gives
    linear_pred; flip_tta averages the mirrored pass; cluster_resolution="pixel" clusters the up-sampled code."""
    S, P = 64, 8
    G = S // P
    sd = OV.make_vit_state_dict("vit_small", P, pretrain_grid=28, seed=21, depth=1)
    head = OI.make_stego_head_state_dict(384, 90, seed=4)
    gg = g(31)
    clusters, lin_w, lin_b = torch.randn(27, 90, generator=gg), torch.randn(27, 90, generator=gg) * 0.3, torch.randn(27, generator=gg) * 0.1
    path = str(tmp_path / "stego_ckpt.ckpt")
    torch.save(_lightning_ckpt(sd, head, clusters, lin_w, lin_b, layout), path)
    img = torch.rand(2, 3, S, S, generator=g(32))
    tok = OV.vit_tokens(sd, OI.normalize(img), P, 6)[:, 1:]
    code = OI.stego_code_tokens(head, tok)                                      # [2, G*G, 90]
    tol = {"fp32": 1e-4, "exact": 1e-4, "bf16": 0.15}[prec]

    si = StegoInterface(dev, input_size=S, model_path=path, n_image_clusters=5, run_crf=False, run_clustering=False, precision=prec,
                        flip_tta=False, cluster_resolution="patch")   # (the probes at patch resolution: labels comparable patch by patch)
    lin, clu = si.inference(img.to(dev))
    assert (si.feature_tokens.cpu() - code).abs().max().item() < tol
    assert lin.shape == clu.shape == (1, 2, S, S) and lin.dtype == torch.int32
    want_clu = (torch.nn.functional.normalize(code, dim=-1) @ torch.nn.functional.normalize(clusters, dim=1).T).argmax(-1)
    want_lin = (code @ lin_w.T + lin_b).argmax(-1)
    agree = lambda got, want: (got[0].cpu()[:, ::P, ::P].reshape(2, -1) == want).float().mean().item()
    thr = 0.999 if prec != "bf16" else 0.9
    assert agree(clu, want_clu) >= thr and agree(lin, want_lin) >= thr

    flip = StegoInterface(dev, input_size=S, model_path=path, n_image_clusters=5, run_crf=False, run_clustering=True, precision=prec)   # (the default)
    tok_f = OV.vit_tokens(sd, OI.normalize(img.flip(-1)), P, 6)[:, 1:]
    code_f = OI.stego_code_tokens(head, tok_f).reshape(2, G, G, 90).flip(2).reshape(2, G * G, 90)
    assert (flip.code_tokens(img.to(dev)).cpu() - 0.5 * (code + code_f)).abs().max().item() < tol

    if prec == "fp32":
        pix = StegoInterface(dev, input_size=S, model_path=path, n_image_clusters=5, run_crf=False, run_clustering=True,
                             precision=prec, cluster_resolution="pixel")
        _, clu_p = pix.inference(img.to(dev))
        gcode = pix.feature_tokens.cpu().numpy()                                 # [2, G*G, 90] from the GPU
        for b in range(2):
            want = OI.relabel_ascending(KL.kmeans_cosine_labels_pixels_linear(gcode[b], G, S, 5))
            assert np.array_equal(clu_p[0, b].cpu().numpy().reshape(-1), want)   # bit-exact on identical fp32 input
        # the probes under the same reading (cluster_resolution="pixel"): per-patch scores interpolated, argmax per pixel
        pp = StegoInterface(dev, input_size=S, model_path=path, n_image_clusters=5, run_crf=False, run_clustering=False, precision=prec,
                            flip_tta=False, cluster_resolution="pixel")
        lin_p, clu_pp = pp.inference(img.to(dev))
        gc = torch.from_numpy(pp.feature_tokens.cpu().numpy())
        up = lambda t: torch.from_numpy(np.stack([OI.upsample_bilinear_fixed(t[b].reshape(G, G, -1).numpy(), S) for b in range(2)]))
        want_lin_p = up(gc @ lin_w.T + lin_b).argmax(-1)
        want_clu_p = up(gc @ torch.nn.functional.normalize(clusters, dim=1).T).argmax(-1)
        assert (lin_p[0].cpu() == want_lin_p).float().mean().item() >= 0.999 and (clu_pp[0].cpu() == want_clu_p).float().mean().item() >= 0.999
        fe = FeatureExtractor(dev, segmentation_type="stego", feature_type="stego", input_size=S, model_path=path,
                              n_image_clusters=5, precision=prec, cluster_resolution="pixel")
        edges, feat, seg, center, _ = fe.extract(img[:1].to(dev))
        assert feat.shape == (int(seg.max()) + 1, 90) and torch.isfinite(feat).all()


def test_extract_batch_equals_per_frame(dev):
    """Batched hot path (BASELINE config 3 shape, scaled down) == per-frame extract()."""
    S = 64
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=11, depth=2)
    img = torch.rand(4, 3, S, S, generator=g(12)).to(dev)
    fe = FeatureExtractor(dev, segmentation_type="grid", feature_type="dino", input_size=S, backbone_type="vit_small",
                          patch_size=8, pretrained_weights=sd, precision="bf16")
    feat, seg, nseg = fe.extract_batch(img, cell_size=16)
    assert feat.shape == (4, 16, 384) and seg.shape == (4, S, S) and nseg.tolist() == [16] * 4
    for b in range(4):
        _, f1, s1, _, _ = fe.extract(img[b:b + 1], cell_size=16)
        # tokens are bit-identical (batch invariance); the patch-aligned and the general pooling kernels associate the same
        # sums differently, hence round-off-level differences only
        assert torch.allclose(f1, feat[b], atol=1e-5, rtol=0) and torch.equal(s1.int(), seg[b])


# ------------------------------------------------------------------------------ full-size properties
def test_full_size_properties_448(dev):
    """448x448 ViT-S/8 (N = 3137 tokens), 12 blocks, bf16: properties that do not need a full-size oracle."""
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=0)
    bb = VitBackbone(sd, 448, 8, 6, device=dev, precision="bf16", max_chunk=2)
    img = torch.rand(3, 3, 448, 448, generator=g(1)).to(dev)
    img[2] = img[0]
    tok = bb.forward_tokens(img)
    assert tok.shape == (3, 3136, 384) and torch.isfinite(tok).all()
    assert torch.equal(tok[0], tok[2])  # identical frames -> identical features, whatever the batch slot
    assert not torch.equal(tok[0], tok[1])
    # final LayerNorm: every token has the affine-LN statistics of norm.weight / norm.bias
    gm, bt = sd["norm.weight"].to(dev), sd["norm.bias"].to(dev)
    z = (tok - bt) / gm
    assert z.mean(-1).abs().max().item() < 2e-3 and (z.var(-1, unbiased=False) - 1).abs().max().item() < 2e-2
    # fused pooling: a grid cell's pooled feature == mean over its pixels of the explicitly up-sampled map
    seg = OS.segment_grid(448, 448, 32)[0, 0].to(dev)
    pooled = ops.segpool_bilinear_mean(seg[None].int(), tok[:1], 56, 196)[0]
    dense = ops.upsample_bilinear(tok[:1], 56, 448)
    want = dense[0].reshape(384, 14, 32, 14, 32).mean(dim=(2, 4)).reshape(384, 196).T
    assert (pooled - want).abs().max().item() < 1e-4
    # weights of every segment sum to one: pooling a constant map returns the constant
    ones = torch.ones(1, 3136, 8, device=dev)
    assert (ops.segpool_bilinear_mean(seg[None].int(), ones, 56, 196) - 1).abs().max().item() < 1e-5


def test_position_table_rule_size_matches_the_oracle(dev):
    """VitBackbone(pos_embed_rule="size"): HuggingFace's reading of the position-table resampling (oracle/vit.py rule "size", cross-checked against
    transformers at G = 56 in tests/test_oracle_vit.py) -- a different table, the same network."""
    from wild_visual_navigation_amd.backbone import VitBackbone
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=5, depth=2)
    img = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(6))
    for rule in ("dino", "size"):
        want = OV.vit_tokens(sd, OI.normalize(img), 8, 6, pos_embed_rule=rule)[:, 1:]
        got = VitBackbone(sd, 128, 8, 6, device=dev, precision="exact", pos_embed_rule=rule).forward_tokens(img.to(dev)).cpu()
        assert (got - want).abs().max().item() < 1e-3, rule
    a = OV.vit_tokens(sd, OI.normalize(img), 8, 6, pos_embed_rule="dino")
    b = OV.vit_tokens(sd, OI.normalize(img), 8, 6, pos_embed_rule="size")
    assert (a - b).abs().max().item() > 1e-3      # (the two readings really are different networks on a random table)
