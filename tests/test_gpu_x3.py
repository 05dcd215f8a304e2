"""Exact mode ON THE MATRIX PIPE (precision "exact" = WVN_PREC_X3): every MFMA operand is two bf16 planes (hi + lo) and every
product hi*hi + hi*lo + lo*hi with fp32 accumulation.  Building blocks against fp64 references, then the whole backbone against
the CPU oracle at the north_star tolerance (<= 1e-3 absolute on the final LayerNorm'ed tokens), including the shipped kernel
instantiations bench.py runs (448^2, (frame, head) count a multiple of 8 -> XCD block order; 25 query blocks; masked last tile)."""
import pytest
import torch

from oracle import interfaces as OI, vit as OV
from wild_visual_navigation_amd import _lib, ops
from wild_visual_navigation_amd.backbone import VitBackbone, split_planes

pytestmark = pytest.mark.gpu


def g(seed):
    return torch.Generator().manual_seed(seed)


def unsplit(p):
    return p[0].double() + p[1].double()


def test_split_planes_carries_16_bits(dev):
    x = (torch.randn(300, 77, generator=g(0)) * 3).to(dev)
    p = ops.split_planes(x)
    assert torch.equal(p, split_planes(x))                       # the device kernel == the torch restatement used for weights
    rel = ((unsplit(p) - x.double()).abs() / x.double().abs().clamp_min(1e-30)).max().item()
    assert rel < 2.0 ** -16, rel


@pytest.mark.parametrize("M,N,K", [(256, 384, 384), (300, 1536, 384), (515, 384, 1536), (128, 90, 768), (200, 384, 192),
                                   (130, 768, 640)])
@pytest.mark.parametrize("epi", ["planes", "gelu", "relu", "f32", "resid"])
def test_gemm_x3_is_fp32_class(dev, M, N, K, epi):
    a = torch.randn(M, K, generator=g(1)).to(dev)
    w = (torch.randn(N, K, generator=g(2)) * 0.05).to(dev)
    bias = (torch.randn(N, generator=g(3)) * 0.1).to(dev)
    ref = a.double() @ w.double().T + bias.double()
    mag = a.double().abs() @ w.double().abs().T + bias.double().abs()     # scale of the rounding error of any summation order
    ap, wp = ops.split_planes(a), ops.split_planes(w)
    if epi == "planes":
        got = unsplit(ops.gemm_x3(ap, wp, bias, _lib.EPI_BF16))
    elif epi == "gelu":
        got = unsplit(ops.gemm_x3(ap, wp, bias, _lib.EPI_GELU_BF16))
        ref = torch.nn.functional.gelu(ref)                                 # exact erf form
    elif epi == "relu":
        got = unsplit(ops.gemm_x3(ap, wp, bias, _lib.EPI_RELU_BF16))
        ref = ref.clamp_min(0)
    elif epi == "f32":
        got = ops.gemm_x3(ap, wp, bias, _lib.EPI_F32).double()
    else:
        c0 = torch.randn(M, N, generator=g(4)).to(dev)
        got = ops.gemm_x3(ap, wp, bias, _lib.EPI_RESID_F32, out=c0.clone()).double()
        ref = ref + c0.double()
        mag = mag + c0.double().abs()
    err = ((got - ref).abs() / mag).max().item()
    # operands carry 2^-17 relative error each, the dropped lo*lo term 2^-16 of a product, planes of the output 2^-17
    assert err < 4e-5, err
    # and it is at least 50x closer than single-plane bf16 would be (guards against a dropped lo term)
    assert err < (2.0 ** -9) / 50


def test_gemm_x3_unaligned_odd_ldc_output_with_n_tail(dev):
    """The output is columns 1..N of a sentinel-filled [2, M, N + 3] (planes) or [M, N + 3] (fp32) buffer: ldc is odd and C is off
    16-byte alignment, so the tiled kernel stores element by element (csrc/tile_epilogue.h, vec_ok == false), and N % 8 = N % 4 = 2
    ends both store loops in their scalar tail.  Values as in test_gemm_x3_is_fp32_class; nothing outside the N columns is written."""
    M, N, K = 130, 90, 128
    a = torch.randn(M, K, generator=g(1)).to(dev)
    w = (torch.randn(N, K, generator=g(2)) * 0.05).to(dev)
    bias = (torch.randn(N, generator=g(3)) * 0.1).to(dev)
    ref = a.double() @ w.double().T + bias.double()
    mag = a.double().abs() @ w.double().abs().T + bias.double().abs()
    ap, wp = ops.split_planes(a), ops.split_planes(w)

    def edge_bits(buf):
        edge = torch.cat([buf[..., :1], buf[..., N + 1:]], -1).contiguous()
        return edge.view(torch.int16 if edge.element_size() == 2 else torch.int32)

    buf = torch.full((2, M, N + 3), -7.0, dtype=torch.bfloat16, device=dev)
    clean = edge_bits(buf)
    ops.gemm_x3(ap, wp, bias, _lib.EPI_BF16, out=buf[:, :, 1:1 + N])
    err = ((unsplit(buf[:, :, 1:1 + N]) - ref).abs() / mag).max().item()
    assert err < 4e-5, err
    assert torch.equal(edge_bits(buf), clean)
    c0 = torch.randn(M, N, generator=g(4)).to(dev)
    buf = torch.full((M, N + 3), -7.0, device=dev)
    clean = edge_bits(buf)
    buf[:, 1:1 + N] = c0
    ops.gemm_x3(ap, wp, bias, _lib.EPI_RESID_F32, out=buf[:, 1:1 + N])
    err = ((buf[:, 1:1 + N].double() - (ref + c0.double())).abs() / (mag + c0.double().abs())).max().item()
    assert err < 4e-5, err
    assert torch.equal(edge_bits(buf), clean)


def test_gemm_x3_accum_epilogue_is_the_residual_arithmetic(dev):
    """EPI_ACCUM_F32 (the second GEMM of a sum) is documented as the arithmetic of EPI_RESID_F32: the same bits."""
    M, N, K = 130, 90, 128
    ap = ops.split_planes(torch.randn(M, K, generator=g(1)).to(dev))
    wp = ops.split_planes((torch.randn(N, K, generator=g(2)) * 0.05).to(dev))
    bias = (torch.randn(N, generator=g(3)) * 0.1).to(dev)
    c0 = torch.randn(M, N, generator=g(4)).to(dev)
    resid = ops.gemm_x3(ap, wp, bias, _lib.EPI_RESID_F32, out=c0.clone())
    assert torch.equal(ops.gemm_x3(ap, wp, bias, _lib.EPI_ACCUM_F32, out=c0.clone()), resid)
    assert not torch.equal(resid, c0)


def _attention_ref(q, k, v, scale):
    s = (q.double() @ k.double().transpose(-1, -2)) * scale
    return (s.softmax(-1) @ v.double())


@pytest.mark.parametrize("B,heads,ntok", [(1, 6, 330), (4, 6, 197), (2, 12, 3137)])
def test_attention_x3_is_fp32_class(dev, B, heads, ntok):
    """nbh = 6 (plain block order), 24 and 24 (XCD block order); ntok 3137 = the 448^2 sequence (25 query blocks, 50 tiles,
    masked tail of 63 keys)."""
    npad = (ntok + 127) // 128 * 128
    q = torch.randn(B, heads, ntok, 64, generator=g(5)).to(dev)
    k = torch.randn(B, heads, ntok, 64, generator=g(6)).to(dev)
    v = torch.randn(B, heads, ntok, 64, generator=g(7)).to(dev)
    ref = _attention_ref(q, k, v, 0.125).transpose(1, 2).reshape(B * ntok, heads * 64)

    def padded(t):
        o = torch.zeros(B, heads, npad, 64, device=dev)
        o[:, :, :ntok] = t
        return o

    qp = ops.split_planes(padded(q).reshape(-1, 64)).reshape(2, B, heads, npad, 64)
    kp = ops.split_planes(padded(k).reshape(-1, 64)).reshape(2, B, heads, npad, 64)
    vt = padded(v).transpose(-1, -2)[..., ops.vt_token_order(npad, dev)].contiguous()      # [B,h,64,npad], token-permuted
    vp = ops.split_planes(vt.reshape(-1, npad)).reshape(2, B, heads, 64, npad)
    out = torch.zeros(2, B * ntok, heads * 64, dtype=torch.bfloat16, device=dev)
    _lib.check(_lib.lib().wvn_attention_x3(qp[0].data_ptr(), qp[1].data_ptr(), kp[0].data_ptr(), kp[1].data_ptr(), vp[0].data_ptr(),
                                           vp[1].data_ptr(), out[0].data_ptr(), out[1].data_ptr(), B, heads, ntok, npad, 0.125,
                                           _lib.stream()), "wvn_attention_x3")
    err = (unsplit(out) - ref).abs().max().item()
    assert err < 5e-5, err      # outputs are convex combinations of O(1) values


@pytest.mark.parametrize("precision", ["exact", "mixed"])
@pytest.mark.parametrize("S,depth,B", [(64, 2, 3), (224, 12, 2), (448, 12, 1), (448, 2, 8)])
def test_vit_exact_mode_on_mfma_within_1e3(dev, S, depth, B, precision):
    """The north_star gate on the matrix-pipe paths; (448, 2, 8): nbh = 48 -> the XCD-ordered attention instantiation.  "mixed": the
    linears as in "exact", the attention products on the fp16 kernel (WVN_PREC_MIX) -- gated at HALF the clause from 224^2 on (measured
    1.7 - 2.4e-4 at 224^2 / 448^2 x 12; the CPU emulation of profiles/r04a_error_budget_synthetic.md predicts 2.3e-4)."""
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=0, depth=depth)
    img = torch.rand(B, 3, S, S, generator=g(1))
    want = OV.vit_tokens(sd, OI.normalize(img), 8, 6)[:, 1:]
    bb = VitBackbone(sd, S, 8, 6, device=dev, precision=precision, max_chunk=8)
    got = bb.forward_tokens(img.to(dev)).cpu()
    err = (got - want).abs().max().item()
    print(f"{precision} tokens S={S} depth={depth} B={B}: max|err| = {err:.3e}")
    # (64^2: 65 keys per query -- a probability's fp16 rounding is averaged over far fewer terms than at 3137 keys)
    assert err < (1e-3 if precision == "exact" or S < 224 else 5e-4), f"{precision}-mode tokens differ by {err}"


def test_mixed_mode_is_batch_invariant_and_matches_exact(dev):
    """WVN_PREC_MIX against WVN_PREC_X3 on the same frames (the difference is the attention products' operand format), and the same
    frame alone / inside a batch: bit for bit.  At 64 x 64 five frames are 400 token rows, so this is the TILED route only; the split-operand
    / MX block kernels (from 8192 rows on) have their own invariance checks in tests/test_gpu_block_kernels_wrap.py, and bits are not
    invariant ACROSS that threshold (MX planes)."""
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=3, depth=3)
    img = torch.rand(5, 3, 64, 64, generator=g(5)).to(dev)
    a = VitBackbone(sd, 64, 8, 6, device=dev, precision="mixed", max_chunk=5).forward_tokens(img)
    b = VitBackbone(sd, 64, 8, 6, device=dev, precision="mixed", max_chunk=2).forward_tokens(img)
    c = VitBackbone(sd, 64, 8, 6, device=dev, precision="mixed", max_chunk=1).forward_tokens(img[3:4])
    assert torch.equal(a, b) and torch.equal(a[3:4], c)
    e = VitBackbone(sd, 64, 8, 6, device=dev, precision="exact", max_chunk=5).forward_tokens(img)
    assert (a - e).abs().max().item() < 1e-3


def test_exact_agrees_with_fp32_fma_mode_and_is_batch_invariant(dev):
    """WVN_PREC_X3 against the fp32 FMA mode, and the same frame alone / inside a batch, bit for bit -- on the TILED route only: 400 token
    rows never reach the split-operand block kernels, whose invariance tests/test_gpu_block_kernels_wrap.py checks at 9456 / 18912 rows."""
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=0, depth=3)
    img = torch.rand(5, 3, 64, 64, generator=g(2)).to(dev)
    a = VitBackbone(sd, 64, 8, 6, device=dev, precision="exact", max_chunk=5).forward_tokens(img)
    b = VitBackbone(sd, 64, 8, 6, device=dev, precision="exact", max_chunk=2).forward_tokens(img)
    c = VitBackbone(sd, 64, 8, 6, device=dev, precision="exact", max_chunk=1).forward_tokens(img[3:4])
    assert torch.equal(a, b) and torch.equal(a[3:4], c)
    f = VitBackbone(sd, 64, 8, 6, device=dev, precision="fp32", max_chunk=5).forward_tokens(img)
    assert (a - f).abs().max().item() < 2e-4


def test_vit_base_exact_and_bf16(dev):
    """ViT-Base/8 (D = 768, 12 heads): the backbone of the reference's released STEGO checkpoint (stego_interface.py:23)."""
    sd = OV.make_vit_state_dict("vit_base", 8, pretrain_grid=28, seed=4, depth=3)
    img = torch.rand(2, 3, 96, 96, generator=g(8))
    want = OV.vit_tokens(sd, OI.normalize(img), 8, 12)[:, 1:]
    got = VitBackbone(sd, 96, 8, 12, device=dev, precision="exact").forward_tokens(img.to(dev)).cpu()
    assert (got - want).abs().max().item() < 1e-3
    got = VitBackbone(sd, 96, 8, 12, device=dev, precision="fp32").forward_tokens(img.to(dev)).cpu()
    assert (got - want).abs().max().item() < 1e-3
    got = VitBackbone(sd, 96, 8, 12, device=dev, precision="bf16").forward_tokens(img.to(dev)).cpu()
    assert ((got - want).norm() / want.norm()).item() < 2.5e-2


@pytest.mark.parametrize("arch,heads,S,depth,B", [("vit_small", 6, 70, 2, 3), ("vit_base", 12, 518, 2, 1), ("vit_base", 12, 224, 12, 2)])
def test_dinov2_layerscale_patch14(dev, arch, heads, S, depth, B):
    """DINOv2 ViT-{S,B}/14 (BASELINE configs[4]: ViT-B/14 at 518^2 -> 37 x 37 + 1 = 1370 tokens): LayerScale on both branch
    outputs, patch 14 (588-wide patch rows padded to 640 for the MFMA GEMMs), D = 768 through the generic tiled kernels."""
    sd = OV.make_dinov2_state_dict(arch, 14, pretrain_grid=37, seed=3, depth=depth)
    img = torch.rand(B, 3, S, S, generator=g(9))
    want = OV.vit_tokens(sd, OI.normalize(img), 14, heads)[:, 1:]
    for prec, tol in (("exact", 1e-3), ("fp32", 1e-3)):
        got = VitBackbone(sd, S, 14, heads, device=dev, precision=prec, max_chunk=2).forward_tokens(img.to(dev)).cpu()
        err = (got - want).abs().max().item()
        print(f"dinov2 {arch} S={S} depth={depth} [{prec}]: max|err| = {err:.3e}")
        assert err < tol, (prec, err)
    got = VitBackbone(sd, S, 14, heads, device=dev, precision="bf16", max_chunk=2).forward_tokens(img.to(dev)).cpu()
    assert ((got - want).norm() / want.norm()).item() < 2.5e-2


# ---------------------------------------------------------------------------------------------------------------------------
# "Test what you bench": the instantiations bench.py actually launches, against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def test_reference_448_frame_through_the_full_backbone(dev, golden):
    """assets/graph/img.png -- the one real 448 x 448 frame the reference ships -- through all 12 blocks in every precision."""
    u8 = golden("graph_img_448.pt")["frame_u8"]
    img = (u8.float() / 255)[None]
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=0)
    want = OV.vit_tokens(sd, OI.normalize(img), 8, 6)[:, 1:]
    got = VitBackbone(sd, 448, 8, 6, device=dev, precision="exact").forward_tokens(img.to(dev)).cpu()
    err = (got - want).abs().max().item()
    print(f"img.png 448^2 exact: max|err| = {err:.3e}")
    assert err < 1e-3
    # the <= 1e-3 mode: q as two planes in the first six blocks only (the default; include/wvn_hip.h WVN_VIT_QSPLIT_BLOCKS) -- the query's
    # rounding enters in the early blocks: the table this prints is profiles/r05_qsplit_blocks.md's GPU column
    errs = {}
    for n in (None, 12, 4, 2, 0):
        got = VitBackbone(sd, 448, 8, 6, device=dev, precision="mixed", qsplit_blocks=n).forward_tokens(img.to(dev)).cpu()
        errs[n] = (got - want).abs().max().item()
        print(f"img.png 448^2 mixed, q split in the first {'6 (default)' if n is None else n} blocks: max|err| = {errs[n]:.3e}")
    assert errs[None] < 5e-4 and errs[12] < 2e-4 and errs[4] < 1e-3, errs
    bb = VitBackbone(sd, 448, 8, 6, device=dev, precision="bf16")
    got = bb.forward_tokens(img.to(dev)).cpu()
    rel = ((got - want).norm() / want.norm()).item()
    print(f"img.png 448^2 bf16: rel-L2 = {rel:.3e}, max|err| = {(got - want).abs().max().item():.3e}")
    assert rel < 2.5e-2
    assert torch.equal(bb.forward_tokens(u8[None].to(dev)).cpu(), got)          # uint8 ingest: bit-identical


def test_vit_base_8_mixed_at_448_within_1e3(dev, golden):
    """ViT-Base/8 (D = 768, 12 heads, 12 blocks: the backbone of the reference's released STEGO checkpoint, stego_interface.py:23) on the reference's
    real 448 x 448 frame in the <= 1e-3 mode (class default).  D = 768 has no row-panel / A-stationary kernels: the linears run on the tiled
    split-operand kernel (csrc/gemm_x3.hip), attention on the fp16 kernel with the two-plane q of the first six blocks."""
    u8 = golden("graph_img_448.pt")["frame_u8"]
    img = (u8.float() / 255)[None]
    sd = OV.make_vit_state_dict("vit_base", 8, pretrain_grid=28, seed=2)
    want = OV.vit_tokens(sd, OI.normalize(img), 8, 12)[:, 1:]
    got = VitBackbone(sd, 448, 8, 12, device=dev, precision="mixed").forward_tokens(img.to(dev)).cpu()
    err = (got - want).abs().max().item()
    print(f"img.png 448^2 ViT-Base/8 mixed: max|err| = {err:.3e}")
    assert err < 1e-3


def test_bf16_shipped_instantiations_at_448(dev):
    """bf16 path exactly as bench.py drives it, scaled down in depth only: 448^2 (25 query blocks, 50 key tiles, masked tail),
    B = 16 frames in ONE launch sequence -> (frame, head) count 96 = XCD-ordered attention, pre-scaled-q kernel; 50,432 token
    rows = 197 row blocks -> the fc2 row-panel kernel WITH its thin-last-round hand-over to the tiled kernel (the dispatcher's
    threshold is 192 row blocks); A-stationary K = 384 kernels with the persistent unit-balanced schedule."""
    B = 16
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=2, depth=2)
    img = torch.rand(B, 3, 448, 448, generator=g(11))
    want = OV.vit_tokens(sd, OI.normalize(img), 8, 6)[:, 1:]
    # (a) as shipped: at this size wvn_vit_forward takes the single-kernel LayerNorm + QKV / LayerNorm + MLP stages
    auto = VitBackbone(sd, 448, 8, 6, device=dev, precision="bf16", max_chunk=B).forward_tokens(img.to(dev)).cpu()
    rel = ((auto - want).norm() / want.norm()).item()
    print(f"bf16 448^2 B=16 (XCD attention, fused block stages): rel-L2 = {rel:.3e}, max|err| = {(auto - want).abs().max().item():.3e}")
    assert rel < 6e-3 and (auto - want).abs().max().item() < 0.06      # about twice the measured error (printed above)
    # (b) the separate kernels at the same size: A-stationary QKV / fc1, row-panel fc2 with its hand-over
    bb = VitBackbone(sd, 448, 8, 6, device=dev, precision="bf16", max_chunk=B, fuse_mlp=False, fuse_qkv=False)
    got = bb.forward_tokens(img.to(dev)).cpu()
    rel = ((got - want).norm() / want.norm()).item()
    print(f"bf16 448^2 B=16 (XCD attention, row-panel fc2): rel-L2 = {rel:.3e}, max|err| = {(got - want).abs().max().item():.3e}")
    assert rel < 6e-3 and (got - want).abs().max().item() < 0.06
    # the same frames one at a time take the non-XCD attention instantiation and the tiled fc2 kernel: same bits as (b)
    one = VitBackbone(sd, 448, 8, 6, device=dev, precision="bf16", max_chunk=1)
    for b in (0, 7, 15):
        assert torch.equal(one.forward_tokens(img[b:b + 1].to(dev)).cpu()[0], got[b]), b
