"""The split-operand (bf16 x 3) and MX block kernels where a workgroup takes MORE than one 128-row block: the row-panel kernels launch
min(ceil(M / 128), #CU) workgroups and re-enter `for (rb = blockIdx.x; rb < nrb; rb += gridDim.x)` only beyond #CU row blocks -- every
headline chunk (50432 rows) does, the every-row tests of tests/test_gpu_mx.py / tests/test_gpu_x3_fast.py stop at 99 row blocks.  The only
thing between a workgroup's row blocks is one __syncthreads(): the ring that becomes staging, the LayerNorm statistics, the vmcnt counts of
the first stages all meet there.  Mw = 128 (#CU + 1) + 16 rows: the first two workgroups take a second row block, the last one is ragged
inside a 32-row group.  Three kinds of check at that size:
  A  every row against float64 (and, MX, against the float64 statement of the same operand roundings), guard rows behind M untouched;
     the MX row-panel kernel also at K = 128 (8 stages = ONE trip of the unrolled body: the first-stage waits and the surplus loads
     are most of the kernel) and K = 256, without bias / LayerScale, and into a wider C (ldc = 388);
  B  the identical call ten times: every output plane bit-identical (a ring or wait race would show as an occasional difference);
  C  rows [128 #CU, Mw) -- the ones second-round workgroups computed -- as a problem of their own: bit-identical (a row's k order is
     fixed by K, nothing may depend on which workgroup, or which of its rounds, computes it).
The forward-level checks (B, C) carry the row-panel kernels' LayerNorm statistics output, which no stand-alone entry exposes."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mx import _ln_stats, a384_form  # noqa: E402, F401  (a384_form: the fixture that selects the form of the A-stationary MX kernel)
from test_gpu_x3_fast import n384_pair  # noqa: E402, F401  (the fixture that selects the form of the fragment row-panel kernel)

from oracle import vit as OV  # noqa: E402
from wild_visual_navigation_amd import _lib  # noqa: E402
from wild_visual_navigation_amd.backbone import (VitBackbone, mx_fragments, mx_matmul_reference, pack_a384_mx, pack_fc2_fragment_major,  # noqa: E402
                                                 pack_n384_mx, split_planes)

pytestmark = pytest.mark.gpu

REPEATS = 10
BOTH_PAIR_FORMS = pytest.mark.parametrize("n384_pair", [1, 0], indirect=True, ids=["wave-pair", "one-wave-per-simd"])


def g(seed):
    return torch.Generator().manual_seed(seed)


def wrap_rows(dev):
    """(ncu, Mw, T): Mw rows = ncu + 2 row blocks, the last one of 16 rows; rows from T = 128 ncu on belong to second-round workgroups."""
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    return ncu, 128 * (ncu + 1) + 16, 128 * ncu


def all_equal_to_first(call, what):
    first = call()
    for n in range(1, REPEATS):
        again = call()
        for name, a, b in zip(what, first, again):
            assert torch.equal(a, b), f"run {n}: {name} differs from run 0 in {int((a != b).sum())} elements"


# ---- the MX row-panel kernel (csrc/gemm_n384_x3.hip: gemm_n384_mx_pair_kernel) -------------------------------------------------------------

class N384MX:
    """x += (A W^T + b) * ls, the inputs of tests/test_gpu_mx.py::test_row_panel_mx_every_row."""

    def __init__(self, dev, M, K, affine=True, ldc=384):
        self.dev, self.M, self.K, self.ldc = dev, M, K, ldc
        a = torch.randn(M, K, generator=g(M + K))
        a[::7, ::5] *= 30.0                               # a spread of magnitudes inside one row (the residues must keep their own exponents)
        self.a = a.to(dev)
        self.w = (torch.randn(384, K, generator=g(1)) * 0.03).to(dev)
        self.bias = (torch.randn(384, generator=g(2)) * 0.1).to(dev) if affine else None
        self.ls = (0.5 + torch.rand(384, generator=g(3))).to(dev) if affine else None
        self.wp = pack_n384_mx(self.w)
        self.x0 = torch.randn(M + 64, ldc, generator=g(4)).to(dev)   # (ldc > 384: the columns behind 384 are sentinels)

    def run(self, first=0):
        """Rows [first, M) as a problem of their own (first = 0: the whole) -> C with its 64 guard rows."""
        M = self.M - first
        ah, al8, ah8 = mx_fragments(self.a[first:])
        planes = torch.cat([ah.view(torch.uint8).reshape(-1), al8.reshape(-1), ah8.reshape(-1)])   # one allocation: hi | l8 | h8
        n_h = ah.numel() * 2
        c = self.x0[first:].clone()
        _lib.check(_lib.lib().wvn_debug_gemm_n384_mx(planes.data_ptr(), planes.data_ptr() + n_h, planes.data_ptr() + n_h + al8.numel(), self.wp.data_ptr(),
                                                     self.bias.data_ptr() if self.bias is not None else 0, self.ls.data_ptr() if self.ls is not None else 0,
                                                     c.data_ptr(), self.ldc, M, self.K, 0, _lib.stream()), "n384_mx")
        torch.cuda.synchronize()
        return c

    def check_every_row(self, c, tag):
        M, x0 = self.M, self.x0
        b = self.bias.double() if self.bias is not None else 0.0
        ls = self.ls.double() if self.ls is not None else 1.0
        got = c[:M, :384].double()
        same = x0[:M, :384].double() + (mx_matmul_reference(self.a, self.w) + b) * ls
        want = x0[:M, :384].double() + (self.a.double() @ self.w.double().T + b) * ls
        scale = (self.a.double().abs() @ self.w.double().abs().T).max().item()
        e_same, e_want = (got - same).abs().max().item() / scale, (got - want).abs().max().item() / scale
        print(f"n384_mx {tag} M = {M} K = {self.K}: |got - MX statement| = {e_same:.2e} * scale, |got - float64| = {e_want:.2e} * scale, "
              f"|MX statement - float64| = {(same - want).abs().max().item() / scale:.2e} * scale, scale = {scale:.1f}")
        assert e_same < 3e-6, "the kernel does not compute the MX statement"
        assert e_want < 4e-5
        assert torch.equal(c[M:], x0[M:]), "guard rows behind M were written"
        assert torch.equal(c[:, 384:], x0[:, 384:]), "columns behind 384 were written"


@pytest.mark.parametrize("K", [384, 128, 256])
def test_row_panel_mx_every_row_past_one_block_per_cu(dev, K):
    ncu, Mw, _ = wrap_rows(dev)
    p = N384MX(dev, Mw, K)
    p.check_every_row(p.run(), f"[{ncu} CUs]")


def test_row_panel_mx_without_bias_and_layerscale(dev):
    """bias = ls = NULL: the kernel's tables hold 0 / 1."""
    p = N384MX(dev, 300, 128, affine=False)
    p.check_every_row(p.run(), "[no bias, no LayerScale]")


def test_row_panel_mx_wider_c(dev):
    """ldc = 388: the four columns behind a row's 384 are not the kernel's."""
    p = N384MX(dev, 300, 128, ldc=388)
    p.x0[:, 384:] = -77.0
    p.check_every_row(p.run(), "[ldc 388]")


def test_row_panel_mx_repeatable(dev):
    p = N384MX(dev, wrap_rows(dev)[1], 384)
    all_equal_to_first(lambda: (p.run(),), ["x"])


def test_row_panel_mx_rows_do_not_depend_on_their_position(dev):
    _, Mw, T = wrap_rows(dev)
    p = N384MX(dev, Mw, 384)
    assert torch.equal(p.run()[T:], p.run(first=T))


# ---- the bf16 x 3 row-panel kernel (gemm_n384_x3_kernel) -----------------------------------------------------------------------------------

class N384X3:
    """The inputs of tests/test_gpu_x3_fast.py::test_row_panel_residual_update_every_row."""

    def __init__(self, dev, M, K):
        self.M, self.K = M, K
        self.a = torch.randn(M, K, generator=g(M + K)).to(dev)
        self.w = (torch.randn(384, K, generator=g(1)) * 0.03).to(dev)
        self.bias, self.ls = (torch.randn(384, generator=g(2)) * 0.1).to(dev), (0.5 + torch.rand(384, generator=g(3))).to(dev)
        self.wp = split_planes(self.w)
        self.x0 = torch.randn(M + 64, 384, generator=g(4)).to(dev)

    def run(self, first=0):
        ap = split_planes(self.a[first:])
        c = self.x0[first:].clone()
        _lib.check(_lib.lib().wvn_debug_gemm_n384_x3(ap[0].data_ptr(), ap[1].data_ptr(), self.K, self.wp[0].data_ptr(), self.wp[1].data_ptr(), self.bias.data_ptr(),
                                                     self.ls.data_ptr(), c.data_ptr(), 384, self.M - first, self.K, 0, _lib.stream()), "n384_x3")
        torch.cuda.synchronize()
        return c


@pytest.mark.parametrize("K", [384, 1536])
def test_row_panel_x3_every_row_past_one_block_per_cu(dev, K):
    ncu, Mw, _ = wrap_rows(dev)
    p = N384X3(dev, Mw, K)
    c = p.run()
    want = p.x0[:Mw].double() + (p.a.double() @ p.w.double().T + p.bias.double()) * p.ls.double()
    err = (c[:Mw].double() - want).abs().max().item()
    print(f"n384_x3 [{ncu} CUs] M = {Mw} K = {K}: |got - float64| = {err:.2e}")
    assert err < 1e-4
    assert torch.equal(c[Mw:], p.x0[Mw:])


def test_row_panel_x3_repeatable(dev):
    p = N384X3(dev, wrap_rows(dev)[1], 1536)
    all_equal_to_first(lambda: (p.run(),), ["x"])


def test_row_panel_x3_rows_do_not_depend_on_their_position(dev):
    _, Mw, T = wrap_rows(dev)
    p = N384X3(dev, Mw, 384)
    assert torch.equal(p.run()[T:], p.run(first=T))


# ---- the bf16 x 3 A-stationary kernel (csrc/gemm_a384_x3.hip), stand-alone -----------------------------------------------------------------

@pytest.mark.parametrize("N,epi", [(1536, 1), (384, 4)], ids=["gelu-planes", "residual"])
def test_a_stationary_x3_repeatable(dev, N, epi):
    """(its values at this size: every row block of tests/test_gpu_x3_fast.py::test_a_stationary_k384_every_row already shares its workgroup with others)"""
    lib = _lib.lib()
    Mw = wrap_rows(dev)[1]
    a = torch.randn(Mw, 384, generator=g(Mw + N)).to(dev)
    w = (torch.randn(N, 384, generator=g(1)) * 0.05).to(dev)
    bias = (torch.randn(N, generator=g(2)) * 0.1).to(dev)
    ap, wp = split_planes(a), split_planes(w)
    x0 = torch.randn(Mw + 32, N, generator=g(5)).to(dev)

    def call():
        if epi == 1:
            c = torch.zeros(2, Mw + 32, N, dtype=torch.bfloat16, device=dev)
            _lib.check(lib.wvn_debug_gemm_a384_x3(ap[0].data_ptr(), ap[1].data_ptr(), 384, wp[0].data_ptr(), wp[1].data_ptr(), bias.data_ptr(), c[0].data_ptr(),
                                                  c[1].data_ptr(), N, Mw, N, epi, 0, _lib.stream()), "a384_x3")
            torch.cuda.synchronize()
            return c[0].view(torch.int16), c[1].view(torch.int16)       # (bits, not values: -0 == 0 and NaN != NaN are not what is asked)
        c = x0.clone()
        _lib.check(lib.wvn_debug_gemm_a384_x3(ap[0].data_ptr(), ap[1].data_ptr(), 384, wp[0].data_ptr(), wp[1].data_ptr(), bias.data_ptr(), c.data_ptr(), 0, N,
                                              Mw, N, epi, 0, _lib.stream()), "a384_x3")
        torch.cuda.synchronize()
        return (c.view(torch.int32),)

    all_equal_to_first(call, ["hi plane", "lo plane"] if epi == 1 else ["x"])


# ---- the bf16 x 3 MLP: fc1 writes fragments, the fragment row-panel kernel consumes them ----------------------------------------------------

class MlpX3Frag:
    """The inputs of tests/test_gpu_x3_fast.py::test_fragment_major_mlp_every_row."""
    F = 1536

    def __init__(self, dev, M):
        F = self.F
        self.dev, self.M = dev, M
        self.a = torch.randn(M, 384, generator=g(M)).to(dev)
        self.w1, self.b1 = (torch.randn(F, 384, generator=g(1)) * 0.05).to(dev), (torch.randn(F, generator=g(2)) * 0.1).to(dev)
        self.w2, self.b2 = (torch.randn(384, F, generator=g(3)) * 0.03).to(dev), (torch.randn(384, generator=g(4)) * 0.1).to(dev)
        self.w1p, self.w2p = split_planes(self.w1), pack_fc2_fragment_major(self.w2)
        self.x0 = torch.randn(M + 64, 384, generator=g(5)).to(dev)

    def run(self, first=0):
        """-> (x with its guard rows, hidden planes as bits [2][ceil(M / 32)][F * 32])"""
        M, F = self.M - first, self.F
        ap = split_planes(self.a[first:])
        Mp = (M + 31) // 32 * 32
        hid = torch.zeros(2, Mp * F, dtype=torch.bfloat16, device=self.dev)
        x = self.x0[first:].clone()
        _lib.check(_lib.lib().wvn_debug_mlp_x3_frag(ap[0].data_ptr(), ap[1].data_ptr(), self.w1p[0].data_ptr(), self.w1p[1].data_ptr(), self.b1.data_ptr(), hid[0].data_ptr(),
                                                    hid[1].data_ptr(), self.w2p.data_ptr(), self.b2.data_ptr(), x.data_ptr(), M, F, 0, 0, _lib.stream()), "mlp_x3_frag")
        torch.cuda.synchronize()
        return x, hid.view(torch.int16).reshape(2, Mp // 32, F * 32)


@BOTH_PAIR_FORMS
def test_fragment_major_mlp_every_row_past_one_block_per_cu(dev, n384_pair):
    ncu, Mw, _ = wrap_rows(dev)
    p = MlpX3Frag(dev, Mw)
    x, _ = p.run()
    want = p.x0[:Mw].double() + torch.nn.functional.gelu(p.a.double() @ p.w1.double().T + p.b1.double()) @ p.w2.double().T + p.b2.double()
    err = (x[:Mw].double() - want).abs().max().item()
    print(f"mlp_x3_frag [{ncu} CUs, pair = {n384_pair}] M = {Mw}: |got - float64| = {err:.2e}")
    assert err < 2e-4
    assert torch.equal(x[Mw:], p.x0[Mw:])


@BOTH_PAIR_FORMS
def test_fragment_major_mlp_repeatable(dev, n384_pair):
    p = MlpX3Frag(dev, wrap_rows(dev)[1])
    all_equal_to_first(p.run, ["x", "hidden planes"])


@BOTH_PAIR_FORMS
def test_fragment_major_mlp_rows_do_not_depend_on_their_position(dev, n384_pair):
    _, Mw, T = wrap_rows(dev)
    p = MlpX3Frag(dev, Mw)
    (x, hid), (xs, hids) = p.run(), p.run(first=T)
    assert torch.equal(hid[:, T // 32:], hids), "fc1 (A-stationary kernel, fragment epilogue)"
    assert torch.equal(x[T:], xs), "fc2 (fragment row-panel kernel)"


# ---- the MX MLP and q | k | v^T: LayerNorm on load, A-stationary MX kernel in both forms ---------------------------------------------------

class MlpMX:
    """The inputs of tests/test_gpu_mx.py::test_mx_block_mlp_every_row (whose M = 128 * 530 + 40 checks the values past one row block per CU)."""
    F = 1536

    def __init__(self, dev, M):
        F = self.F
        self.dev, self.M = dev, M
        x = torch.randn(M, 384, generator=g(M)) * 1.7 + 0.3
        self.x, self.st = x.to(dev), _ln_stats(x).to(dev)
        self.gam, self.bet = (1.0 + 0.1 * torch.randn(384, generator=g(7))).to(dev), (0.05 * torch.randn(384, generator=g(8))).to(dev)
        self.w1p, self.b1 = pack_a384_mx((torch.randn(F, 384, generator=g(1)) * 0.05).to(dev)), (torch.randn(F, generator=g(2)) * 0.1).to(dev)
        self.w2p, self.b2 = pack_n384_mx((torch.randn(384, F, generator=g(3)) * 0.03).to(dev)), (torch.randn(384, generator=g(4)) * 0.1).to(dev)
        self.x0 = torch.randn(M + 64, 384, generator=g(5)).to(dev)

    def run(self, first=0):
        """-> (x with its guard rows, hid_h bits [ceil(M / 32)][F * 32], hid_l8 [ceil(M / 32)][F * 32])"""
        M, F = self.M - first, self.F
        Mp = (M + 31) // 32 * 32
        n_h, n_8 = Mp * F * 2, Mp * F
        hid = torch.zeros(Mp * F * 4, dtype=torch.uint8, device=self.dev)
        x, st = self.x[first:].contiguous(), self.st[first:].contiguous()
        xo = self.x0[first:].clone()
        _lib.check(_lib.lib().wvn_debug_mlp_mx(x.data_ptr(), 384, st.data_ptr(), self.gam.data_ptr(), self.bet.data_ptr(), self.w1p.data_ptr(), self.b1.data_ptr(),
                                               hid.data_ptr(), hid.data_ptr() + n_h, hid.data_ptr() + n_h + n_8, self.w2p.data_ptr(), self.b2.data_ptr(), xo.data_ptr(),
                                               M, F, 0, 0, _lib.stream()), "mlp_mx")
        torch.cuda.synchronize()
        return xo, hid[:n_h].view(torch.int16).reshape(Mp // 32, F * 32), hid[n_h:n_h + n_8].reshape(Mp // 32, F * 32)


def test_mx_block_mlp_repeatable(dev, a384_form):  # noqa: F811
    p = MlpMX(dev, wrap_rows(dev)[1])
    all_equal_to_first(p.run, ["x", "hid_h", "hid_l8"])


def test_mx_block_mlp_rows_do_not_depend_on_their_position(dev, a384_form):  # noqa: F811
    _, Mw, T = wrap_rows(dev)
    p = MlpMX(dev, Mw)
    (x, hh, hl), (xs, hhs, hls) = p.run(), p.run(first=T)
    assert torch.equal(hh[T // 32:], hhs) and torch.equal(hl[T // 32:], hls), "fc1 (A-stationary MX kernel, fragment epilogue)"
    assert torch.equal(x[T:], xs), "fc2 (MX row-panel kernel)"


class QkvMX:
    """The inputs of tests/test_gpu_mx.py::test_mx_qkv at B = 4."""
    heads, ntok_s, npad, B = 6, 3152, 3200, 4

    def __init__(self, dev):
        self.dev = dev
        x = torch.randn(self.B * self.ntok_s, 384, generator=g(11)) * 1.3
        self.x, self.st = x.to(dev), _ln_stats(x).to(dev)
        self.gam, self.bet = (1.0 + 0.1 * torch.randn(384, generator=g(7))).to(dev), (0.05 * torch.randn(384, generator=g(8))).to(dev)
        self.wp, self.b = pack_a384_mx((torch.randn(1152, 384, generator=g(1)) * 0.06).to(dev)), (torch.randn(1152, generator=g(2)) * 0.02).to(dev)

    def run(self, frames=slice(0, 4)):
        """-> (q, q_lo, k, v^T) of the frames as bits, tokens [:ntok_s]"""
        heads, ntok_s, npad = self.heads, self.ntok_s, self.npad
        B = frames.stop - frames.start
        x, st = self.x[frames.start * ntok_s:frames.stop * ntok_s].contiguous(), self.st[frames.start * ntok_s:frames.stop * ntok_s].contiguous()
        per = B * heads * npad * 64
        buf = torch.zeros(4 * per, dtype=torch.float16, device=self.dev)       # (one allocation: the kernel addresses q | k | v^T through one buffer descriptor)
        q, k, vt = buf[:2 * per].view(2, B, heads, npad, 64), buf[2 * per:3 * per].view(B, heads, npad, 64), buf[3 * per:].view(B, heads, 64, npad)
        _lib.check(_lib.lib().wvn_debug_qkv_mx(x.data_ptr(), 384, st.data_ptr(), self.gam.data_ptr(), self.bet.data_ptr(), self.wp.data_ptr(), self.b.data_ptr(),
                                               q[0].data_ptr(), q[1].data_ptr(), k.data_ptr(), vt.data_ptr(), heads, npad, ntok_s, 0.125 * 1.4426950408889634,
                                               B * ntok_s, 0, _lib.stream()), "qkv_mx")
        torch.cuda.synchronize()
        bits = lambda t: t.contiguous().view(torch.int16)   # noqa: E731
        return bits(q[0, :, :, :ntok_s]), bits(q[1, :, :, :ntok_s]), bits(k[:, :, :ntok_s]), bits(vt[..., :ntok_s])


QKV_PLANES = ["q", "q_lo", "k", "v^T"]


def test_mx_qkv_repeatable(dev, a384_form):  # noqa: F811
    all_equal_to_first(QkvMX(dev).run, QKV_PLANES)


def test_mx_qkv_frames_do_not_depend_on_their_position(dev, a384_form):  # noqa: F811
    p = QkvMX(dev)
    for name, a, b in zip(QKV_PLANES, p.run(), p.run(frames=slice(2, 4))):
        assert torch.equal(a[2:4], b), name


# ---- one forward level: every block kernel of the route, with the LayerNorm statistics the row-panel kernels leave -------------------------

def _backbone_and_frames(dev, precision, max_chunk):
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=0, depth=2)
    bb = VitBackbone(sd, 448, 8, 6, device=dev, precision=precision, max_chunk=max_chunk)
    assert bb.mx == (precision == "mixed")
    return bb, torch.rand(6, 3, 448, 448, generator=g(6)).to(dev)


@pytest.mark.parametrize("precision", ["mixed", "exact"])
def test_forward_repeatable(dev, precision):
    """6 frames at 448^2 in one chunk (18912 rows, 148 row blocks) through 2 blocks, twice."""
    bb, img = _backbone_and_frames(dev, precision, 6)
    a = bb.forward_tokens(img).clone()
    b = bb.forward_tokens(img)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("precision", ["mixed", "exact"])
def test_forward_frames_do_not_depend_on_their_position(dev, precision):
    """Frames 3 - 5 of a 6-frame chunk against the 3-frame chunk of those frames (9456 rows): both on the split-operand route (from 8192 rows
    on), so kernel selection is the same and a frame's bits may not depend on its slot or on the size of its chunk."""
    bb, img = _backbone_and_frames(dev, precision, 6)
    a = bb.forward_tokens(img).clone()
    bb3, _ = _backbone_and_frames(dev, precision, 3)
    b = bb3.forward_tokens(img[3:])
    assert torch.equal(a[3:], b)
