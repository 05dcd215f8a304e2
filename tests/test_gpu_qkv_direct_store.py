"""The register-direct q | k | v^T stores of the two-workgroups-per-CU MX kernel (csrc/gemm_a384_x3.hip: gemm_a384_mx2_kernel<X_QKV_F16>): a lane
stores two 16-byte chunks of its own token row (q | k, after one exchange between the half-waves) or of its own V^T row (no exchange), at
per-lane (frame, token) offsets.  The shapes are the smallest at which that addressing can go wrong: 32-row wave blocks that straddle frame
boundaries, a half-valid last block, fewer rows than one workgroup (waves with no valid row), and more row blocks than one with a partial
last one.  Every output plane is pre-filled with a sentinel: the kernel must write every element of the rows below M, and not one byte
anywhere else (the token slots [ntok_s, npad), and the whole second q plane when none is asked for).  Reference, tolerances and the V^T
permutation are those of tests/test_gpu_mx.py::test_mx_qkv."""
import functools

import pytest
import torch

from wild_visual_navigation_amd import _lib
from wild_visual_navigation_amd.backbone import pack_a384_mx

pytestmark = pytest.mark.gpu

HEADS, NPAD = 6, 128
QS = 0.125 * 1.4426950408889634
SENTINEL = 0x7DA5          # an fp16 NaN: the kernel saturates and never produces one


def g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture
def two_workgroup_form():
    lib = _lib.lib()
    lib.wvn_debug_n384_pair(32 + 2)
    yield
    lib.wvn_debug_n384_pair(32)


@functools.lru_cache(maxsize=None)
def _case(ntok_s, B):
    """Inputs and the float64 reference [B][ntok_s][3][heads][64] of one shape (shared by its two runs, never modified)."""
    M = B * ntok_s
    x = torch.randn(M, 384, generator=g(11 + M)) * 1.3
    gam, bet = 1.0 + 0.1 * torch.randn(384, generator=g(7)), 0.05 * torch.randn(384, generator=g(8))
    w, b = torch.randn(3 * HEADS * 64, 384, generator=g(1)) * 0.06, torch.randn(3 * HEADS * 64, generator=g(2)) * 0.02
    mean, var = x.double().mean(-1), x.double().var(-1, unbiased=False)
    stats = torch.stack([mean, 1.0 / torch.sqrt(var + 1e-6)], dim=-1).float().contiguous()
    y = torch.nn.functional.layer_norm(x.double(), (384,), gam.double(), bet.double(), eps=1e-6)
    ref = (y @ w.double().T + b.double()).reshape(B, ntok_s, 3, HEADS, 64)
    return x, stats, gam, bet, w, b, ref


@pytest.mark.parametrize("two_plane", [True, False], ids=["q-two-planes", "q-one-plane"])
@pytest.mark.parametrize("ntok_s,B", [(48, 5), (16, 3), (80, 13)])
def test_qkv_direct_store(dev, two_workgroup_form, ntok_s, B, two_plane):
    lib = _lib.lib()
    M = B * ntok_s
    x, stats, gam, bet, w, b, ref = _case(ntok_s, B)
    d = lambda t: t.to(dev).contiguous()   # noqa: E731
    per = B * HEADS * NPAD * 64
    buf = torch.full((4 * per,), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16)   # (one allocation: one buffer descriptor covers q | k | v^T)
    q, k, vt = buf[:2 * per].view(2, B, HEADS, NPAD, 64), buf[2 * per:3 * per].view(B, HEADS, NPAD, 64), buf[3 * per:].view(B, HEADS, 64, NPAD)
    xd, sd_, gd, bd, wp, bb = d(x), d(stats), d(gam), d(bet), pack_a384_mx(d(w)), d(b)
    _lib.check(lib.wvn_debug_qkv_mx(xd.data_ptr(), 384, sd_.data_ptr(), gd.data_ptr(), bd.data_ptr(), wp.data_ptr(), bb.data_ptr(), q[0].data_ptr(),
                                    q[1].data_ptr() if two_plane else 0, k.data_ptr(), vt.data_ptr(), HEADS, NPAD, ntok_s, QS, M, 0, _lib.stream()), "qkv_mx")
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int16).cpu()   # noqa: E731
    qb, kb, vb = bits(q), bits(k), bits(vt)

    # (2) what the kernel has no business writing is the sentinel, bit for bit
    assert (qb[0][:, :, ntok_s:] == SENTINEL).all(), "q: token slots behind ntok_s were written"
    assert (kb[:, :, ntok_s:] == SENTINEL).all(), "k: token slots behind ntok_s were written"
    assert (vb[:, :, :, ntok_s:] == SENTINEL).all(), "v^T: token slots behind ntok_s were written"
    if two_plane:
        assert (qb[1][:, :, ntok_s:] == SENTINEL).all(), "q_lo: token slots behind ntok_s were written"
    else:
        assert (qb[1] == SENTINEL).all(), "a second q plane was written although none was asked for"

    # (3) every element of the rows below M was written
    assert not (qb[0][:, :, :ntok_s] == SENTINEL).any(), "q: rows below M left unwritten"
    assert not (kb[:, :, :ntok_s] == SENTINEL).any(), "k: rows below M left unwritten"
    assert not (vb[:, :, :, :ntok_s] == SENTINEL).any(), "v^T: rows below M left unwritten"
    if two_plane:
        assert not (qb[1][:, :, :ntok_s] == SENTINEL).any(), "q_lo: rows below M left unwritten"

    # (1) the values, against the float64 reference
    qr = ref[:, :, 0].permute(0, 2, 1, 3) * QS
    if two_plane:
        qg = (q[0].double() + q[1].double()).cpu()[:, :, :ntok_s]
        assert (qg - qr).abs().max().item() < 2e-4
    else:
        qg = q[0].double().cpu()[:, :, :ntok_s]
        assert ((qg - qr).abs() <= 6e-4 * qr.abs() + 2e-4).all()         # one fp16 plane: its own rounding
    kg = k.double().cpu()[:, :, :ntok_s]
    kr = ref[:, :, 1].permute(0, 2, 1, 3)
    assert ((kg - kr).abs() <= 6e-4 * kr.abs() + 2e-4).all()
    # v^T: tokens of every aligned group of 16 in the order 0-3, 8-11, 4-7, 12-15
    t = torch.arange(ntok_s)
    perm = (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)
    vg = vt.double().cpu()[:, :, :, :ntok_s][..., perm]
    vr = ref[:, :, 2].permute(0, 2, 3, 1)
    assert ((vg - vr).abs() <= 6e-4 * vr.abs() + 2e-4).all()
