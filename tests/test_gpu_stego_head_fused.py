"""The STEGO head run off the residual rows (csrc/gemm_a384_x3.hip, X_HEAD; ops.stego_head_fused): ONE A-stationary launch forms the final
LayerNorm on load from fp32 residual rows + their {mean, rstd} and writes ReLU(tok W_hid^T + b_hid) as hi / lo bf16 planes and
tok W_lin^T + b_lin as fp32 rows with a padded stride.  Checked against fp64 at the smallest shapes that reach each way the kernel can go
wrong, with today's path (ops.split_planes + ops.gemm_x3 on the normalised rows) as the yardstick: the new launch may be at most twice as far
from fp64 (+ 1e-6) -- the factor covers the different fp32 summation order over K = 384, and is a margin over a measured reference.

Measured on MI355X, max |err| against fp64, new launch (today's path):
    frames 1, npatch  64:  hidden 3.192e-05 (3.192e-05)   code 2.706e-05 (2.813e-05)
    frames 3, npatch 196:  hidden 3.766e-05 (3.766e-05)   code 3.472e-05 (3.472e-05)
    frames 6, npatch 784:  hidden 4.167e-05 (4.167e-05)   code 3.590e-05 (3.590e-05)
(the hidden figure is the bf16 hi + lo representation of values up to ~4: one unit of the lo plane.  The launch forms
((x - mean) * rstd) * gamma + beta in the fp32 LayerNorm kernel's operation order and sums in the tiled kernel's: on rows whose fp32
statistics equal that kernel's, its results are the separate launches' bit for bit -- tests/test_gpu_stego_head_e2e.py.)
"""
import pytest
import torch

from wild_visual_navigation_amd import _lib, ops
from wild_visual_navigation_amd.backbone import split_planes

pytestmark = pytest.mark.gpu

D, C, LD = 384, 90, 128
FILL = -7.0          # exactly representable in bf16: rows the kernel must not write keep it
# (frames, npatch, ntok_s):
#   64 rows    = half a row block: row clamping on load, guarded stores
#   588 rows   = frame boundaries inside row blocks, the CLS skip, a partial last block
#   4704 rows  = 37 row blocks x 8 column tiles = 296 units on 256 workgroups: workgroups that cross a row-block boundary, row blocks shared by two
SHAPES = [(1, 64, 80), (3, 196, 208), (6, 784, 800)]


def _case(frames, npatch, ntok_s, seed):
    g = torch.Generator().manual_seed(seed)
    R = frames * ntok_s
    x = torch.randn(R, D, generator=g)
    x[::4] += 40.0                                        # a common offset far above the spread on every fourth row (|mean| >> std)
    w_hid, b_hid = torch.randn(D, D, generator=g) * 0.06, torch.randn(D, generator=g) * 0.02
    w_lin, b_lin = torch.randn(C, D, generator=g) * 0.08, torch.randn(C, generator=g) * 0.02
    ln_g, ln_b = 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    x64 = x.double()
    mean, var = x64.mean(1), x64.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-6)
    stats = torch.stack([mean, rstd], 1).float()
    patch = torch.zeros(R, dtype=torch.bool)
    for f in range(frames):
        patch[f * ntok_s + 1:f * ntok_s + 1 + npatch] = True
    tok64 = ((x64 - mean[:, None]) * rstd[:, None] * ln_g.double() + ln_b.double())[patch]       # [M, D]: the rows the head reads
    want_hid = torch.relu(tok64 @ w_hid.double().T + b_hid.double())
    want_code = tok64 @ w_lin.double().T + b_lin.double()
    x[~patch] = float("nan")                              # the class rows, the padding rows and their statistics are never read
    stats[~patch] = float("nan")
    return dict(x=x, stats=stats, ln_g=ln_g, ln_b=ln_b, w_hid=w_hid, b_hid=b_hid, w_lin=w_lin, b_lin=b_lin, tok64=tok64,
                want_hid=want_hid, want_code=want_code)


@pytest.mark.parametrize("frames,npatch,ntok_s", SHAPES)
def test_head_on_load_against_fp64_and_todays_path(dev, frames, npatch, ntok_s):
    c = _case(frames, npatch, ntok_s, seed=frames)
    M = frames * npatch
    pad = 128 - M % 128 + 8                                # past the end of the last row block
    to = lambda t: t.to(dev).contiguous()                  # noqa: E731
    w_cat, b_cat = ops.pack_stego_head(to(c["w_hid"]), to(c["b_hid"]), to(c["w_lin"]), to(c["b_lin"]))
    hid = torch.full((2, M + pad, D), FILL, dtype=torch.bfloat16, device=dev)
    code = torch.full((M + pad, LD), FILL, dtype=torch.float32, device=dev)
    ops.stego_head_fused(to(c["x"]), to(c["stats"]), to(c["ln_g"]), to(c["ln_b"]), w_cat, b_cat, frames, npatch, ntok_s, hid=hid, code=code)
    torch.cuda.synchronize()
    hid, code = hid.cpu(), code.cpu()
    # rows past M keep their fill (guarded stores); every written value is finite (the remap never reads a poisoned row)
    assert (hid[:, M:].float() == FILL).all() and (code[M:] == FILL).all()
    assert torch.isfinite(hid[:, :M].float()).all() and torch.isfinite(code[:M]).all()
    assert (code[:M, C:] == 0).all()                       # the zero rows of the padded weight
    got_hid = hid[0, :M].double() + hid[1, :M].double()
    got_code = code[:M, :C].double()

    # today's path on the same normalised rows: fp32 tokens -> hi / lo planes -> gemm_x3
    tok = ops.split_planes(to(c["tok64"].float()))
    old_hid = ops.gemm_x3(tok, split_planes(to(c["w_hid"])), to(c["b_hid"]), _lib.EPI_RELU_BF16).cpu()
    old_code = ops.gemm_x3(tok, split_planes(to(c["w_lin"])), to(c["b_lin"]), _lib.EPI_F32).cpu()
    old_hid = old_hid[0].double() + old_hid[1].double()

    e_hid, e_hid_old = (got_hid - c["want_hid"]).abs().max().item(), (old_hid - c["want_hid"]).abs().max().item()
    e_code, e_code_old = (got_code - c["want_code"]).abs().max().item(), (old_code.double() - c["want_code"]).abs().max().item()
    print(f"head on load, frames {frames} npatch {npatch}: hidden {e_hid:.3e} (today {e_hid_old:.3e})  code {e_code:.3e} (today {e_code_old:.3e})")
    assert e_hid <= 2 * e_hid_old + 1e-6, (e_hid, e_hid_old)
    assert e_code <= 2 * e_code_old + 1e-6, (e_code, e_code_old)


def test_head_on_load_refuses_before_launching():
    """Bad shapes / pointers answer WVN_ERR_ARG before any launch (no GPU touched: host-only like tests/test_lib_abi.py, but the library must be loaded)."""
    h = _lib.lib()
    assert h.wvn_debug_stego_head_fused(None, 384, None, None, None, None, None, None, None, None, 128, 1, 64, 80, None) == 1001
    assert h.wvn_vit_forward_frames_head(None, None, 0, 1, 1, None, None, None, 1, None, None, 0, None) == 1001
