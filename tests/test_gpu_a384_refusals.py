"""The A-stationary K = 384 launchers (csrc/gemm_a384_x3.hip) refuse what they cannot run: WVN_ERR_ARG, before anything is launched.
One table of ineligible descriptors per stand-alone entry point; every row differs from an eligible call of the same shape in the named
arguments only, must come back with WVN_ERR_ARG and leave a sentinel-filled output buffer as it was, and the eligible call must run.
Shapes are tiny (at most 128 rows): nothing here checks values, the kernels' results are the business of test_gpu_x3_fast.py / test_gpu_mx.py.

Not reachable through these entry points, so not pinned: N != 3 * heads * 64 (wvn_debug_qkv_mx derives N from heads), ldc != N of the
fragment form (both MLP entries pass F for either), and the LayerNorm-on-load checks of the plain launcher (no entry hands it ln_x)."""
import pytest
import torch

from wild_visual_navigation_amd import _lib
from wild_visual_navigation_amd.backbone import pack_a384_mx, pack_fc2_fragment_major, split_planes

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


def g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(params=[2, 1], ids=["two-workgroups-per-cu", "one-wave-per-simd"])
def a384_form(request):
    """Both forms of the MX kernel: each has its own launcher, and each launcher its own LayerNorm-on-load check."""
    lib = _lib.lib()
    lib.wvn_debug_n384_pair(32 + request.param)
    yield request.param
    lib.wvn_debug_n384_pair(32)


def refused_then_runs(call, base, change, out, overwrites=True):
    """call(**base, **change) is refused and leaves `out` alone; call(**base) runs (and, where it does not add to what is there, shows in `out`)."""
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    assert call(**{**base, **change}) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to its output"
    assert call(**base) == 0
    torch.cuda.synchronize()
    assert not overwrites or not bool((out == SENTINEL).all())


# ---- LayerNorm on load + q | k | v^T, MX form (wvn_debug_qkv_mx -> wvn_gemm_a384_mx_launch, EPI_QKV) ----
HEADS, NTOK_S, NPAD, FRAMES = 6, 32, 32, 2
PER = FRAMES * HEADS * NPAD * 64 * 2   # bytes of one fp16 q / k / v^T tensor


@pytest.fixture(scope="module")
def qkv(dev):
    M = FRAMES * NTOK_S
    x = torch.randn(128 * 386 + 8, generator=g(1)).to(dev)          # room for ldx = 386, for M = 72 and for a shifted base
    st = torch.stack([torch.zeros(136), torch.ones(136)], dim=-1).contiguous().to(dev)
    gam, bet = torch.ones(384, device=dev), torch.zeros(384, device=dev)
    wp = pack_a384_mx((torch.randn(3 * HEADS * 64, 384, generator=g(2)) * 0.05).to(dev))
    bias = torch.zeros(3 * HEADS * 64, device=dev)
    out = torch.empty(4 * PER, dtype=torch.uint8, device=dev)       # q | q_lo | k | v^T
    o = out.data_ptr()
    base = dict(x=x.data_ptr(), ldx=384, st=st.data_ptr(), g=gam.data_ptr(), b=bet.data_ptr(), q=o, q_lo=o + PER, k=o + 2 * PER, vt=o + 3 * PER,
                npad=NPAD, ntok_s=NTOK_S, M=M)

    def call(x, ldx, st, g, b, q, q_lo, k, vt, npad, ntok_s, M):
        return _lib.lib().wvn_debug_qkv_mx(x, ldx, st, g, b, wp.data_ptr(), bias.data_ptr(), q, q_lo, k, vt, HEADS, npad, ntok_s, 0.125, M, 0, _lib.stream())

    return call, base, out, (x, st, gam, bet, wp, bias)


QKV_ROWS = {
    "ldx % 4": lambda b: dict(ldx=386),
    "x off 16 bytes": lambda b: dict(x=b["x"] + 8),
    "stats off 8 bytes": lambda b: dict(st=b["st"] + 4),
    "x null": lambda b: dict(x=0),
    "stats null": lambda b: dict(st=0),
    "gamma null": lambda b: dict(g=0),
    "beta null": lambda b: dict(b=0),
    "ntok_s % 16": lambda b: dict(ntok_s=24, M=48),
    "M % 16": lambda b: dict(M=72),
    "npad % 16": lambda b: dict(npad=40),
    "k null": lambda b: dict(k=0),
    # q_off = q - min(q, k, v^T) = 2 * PER here; a second q plane at an address below that cannot carry the same offset
    "q_lo below q_off": lambda b: dict(q=b["k"], k=b["q"], q_lo=16),
}


@pytest.mark.parametrize("row", list(QKV_ROWS))
def test_qkv_mx_refusals(qkv, a384_form, row):
    call, base, out, _ = qkv
    refused_then_runs(call, base, QKV_ROWS[row](base), out)


def test_qkv_mx_span_limit(dev, qkv, a384_form):
    """q | k | v^T go through ONE buffer descriptor: max - min + one tensor must stay below 2^31 bytes.  One allocation of 2 GiB, v^T at its far
    end: at the limit the call is refused, 16 bytes below it runs (and writes v^T there)."""
    call, base, _, _ = qkv
    big = torch.empty((1 << 31) + 4096, dtype=torch.uint8, device=dev)
    o = big.data_ptr()
    lo, hi = big[:3 * PER], big[(1 << 31) - PER - 16:]
    near = dict(q=o, q_lo=o + PER, k=o + 2 * PER)
    lo.fill_(SENTINEL), hi.fill_(SENTINEL)
    torch.cuda.synchronize()
    assert call(**{**base, **near, "vt": o + (1 << 31) - PER}) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all())
    assert call(**{**base, **near, "vt": o + (1 << 31) - PER - 16}) == 0
    torch.cuda.synchronize()
    assert not bool((hi[:PER] == SENTINEL).all()) and bool((hi[PER:] == SENTINEL).all())


# ---- LayerNorm on load + fc1 + GELU -> MX fragment planes (wvn_debug_mlp_mx with W2p == NULL -> wvn_gemm_a384_mx_launch, EPI_GELU_FRAG) ----
@pytest.fixture(scope="module")
def fc1_mx(dev, qkv):
    M, F = 48, 128
    x, st, gam, bet, _, _ = qkv[3]
    w1p = pack_a384_mx((torch.randn(F, 384, generator=g(3)) * 0.05).to(dev))
    b1 = torch.zeros(F, device=dev)
    out = torch.empty(64 * F * 3 + 16, dtype=torch.uint8, device=dev)   # 64 rows: fp16 fragments | l8 (+ room for a shifted base)
    o = out.data_ptr()
    base = dict(x=x.data_ptr(), ldx=384, st=st.data_ptr(), g=gam.data_ptr(), b=bet.data_ptr(), h=o, l8=o + 64 * F * 2, F=F)

    def call(x, ldx, st, g, b, h, l8, F):
        return _lib.lib().wvn_debug_mlp_mx(x, ldx, st, g, b, w1p.data_ptr(), b1.data_ptr(), h, l8, 0, 0, 0, 0, M, F, 0, 0, _lib.stream())

    return call, base, out


FC1_MX_ROWS = {
    "ldx % 4": lambda b: dict(ldx=386),
    "x off 16 bytes": lambda b: dict(x=b["x"] + 8),
    "stats off 8 bytes": lambda b: dict(st=b["st"] + 4),
    "x null": lambda b: dict(x=0),
    "stats null": lambda b: dict(st=0),
    "gamma null": lambda b: dict(g=0),
    "beta null": lambda b: dict(b=0),
    "N % 64": lambda b: dict(F=96),
    "fragments null": lambda b: dict(h=0),
    "l8 null": lambda b: dict(l8=0),
    "fragments off 16 bytes": lambda b: dict(h=b["h"] + 8),
}


@pytest.mark.parametrize("row", list(FC1_MX_ROWS))
def test_fc1_mx_refusals(fc1_mx, a384_form, row):
    call, base, out = fc1_mx
    refused_then_runs(call, base, FC1_MX_ROWS[row](base), out)


# ---- split bf16 operands: GELU planes / fp32 residual (wvn_debug_gemm_a384_x3 -> wvn_gemm_a384_x3_launch) ----
@pytest.fixture(scope="module")
def planes(dev):
    M, N = 48, 128
    ap = split_planes(torch.randn(M + 1, 384, generator=g(4)).to(dev))
    wp = split_planes((torch.randn(N, 384, generator=g(5)) * 0.05).to(dev))
    bias = torch.zeros(N, device=dev)
    out = torch.empty(2 * M * N * 4 + 16, dtype=torch.uint8, device=dev)
    o = out.data_ptr()
    base = dict(A=ap[0].data_ptr(), A_lo=ap[1].data_ptr(), lda=384, W=wp[0].data_ptr(), W_lo=wp[1].data_ptr(), C=o, C_lo=o + M * N * 4, ldc=N, M=M, N=N)

    def call(epi):
        def f(A, A_lo, lda, W, W_lo, C, C_lo, ldc, M, N):
            return _lib.lib().wvn_debug_gemm_a384_x3(A, A_lo, lda, W, W_lo, bias.data_ptr(), C, C_lo, ldc, M, N, epi, 0, _lib.stream())
        return f

    return call, base, out, (ap, wp)


PLANES_ROWS = {
    "N % 64": lambda b: dict(N=96),
    "M == 0": lambda b: dict(M=0),
    "lda % 8": lambda b: dict(lda=380),
    "A off 16 bytes": lambda b: dict(A=b["A"] + 8),
    "A_lo null": lambda b: dict(A_lo=0),
    "W off 16 bytes": lambda b: dict(W=b["W"] + 8),
    "W_lo not behind W": lambda b: dict(W=b["W_lo"], W_lo=b["W"]),
    "W_lo == W": lambda b: dict(W_lo=b["W"]),
    "C null": lambda b: dict(C=0),
    "C off 16 bytes": lambda b: dict(C=b["C"] + 8),
    "ldc % 4": lambda b: dict(ldc=b["N"] + 2),
}


@pytest.mark.parametrize("epi", [1, 4], ids=["gelu-planes", "residual"])
@pytest.mark.parametrize("row", list(PLANES_ROWS) + ["ldc % 8", "C_lo null"])
def test_planes_refusals(planes, row, epi):
    call, base, out, _ = planes
    if row == "ldc % 8":        # the 16-bit planes need 16-byte rows; fp32 rows of ldc % 4 == 0 are eligible
        change = dict(ldc=base["N"] + 4)
    elif row == "C_lo null":    # (the residual form has no second plane)
        change = dict(C_lo=0)
    else:
        change = PLANES_ROWS[row](base)
    if epi == 4 and row in ("ldc % 8", "C_lo null"):
        out.fill_(SENTINEL)
        assert call(epi)(**{**base, **change}) == 0
        return
    refused_then_runs(call(epi), base, change, out, overwrites=epi == 1)   # (the residual form adds to the sentinel: too small to show)


# ---- split bf16 operands, fragment-major hidden planes (wvn_debug_mlp_x3_frag -> wvn_gemm_a384_x3_launch, EPI_GELU_FRAG) ----
@pytest.fixture(scope="module")
def frag(dev, planes):
    M, F = 48, 192   # (the row-panel consumer behind fc1 wants F % 96 == 0)
    ap = planes[3][0]
    w1p = split_planes((torch.randn(F, 384, generator=g(7)) * 0.05).to(dev))
    b1, b2 = torch.zeros(F, device=dev), torch.zeros(384, device=dev)
    w2p = pack_fc2_fragment_major((torch.randn(384, F, generator=g(6)) * 0.05).to(dev))
    xres = torch.zeros(M, 384, device=dev)
    out = torch.empty(2 * 64 * F * 2 + 16, dtype=torch.uint8, device=dev)   # 64 rows: hi | lo fragment planes
    o = out.data_ptr()
    base = dict(hid=o, hid_lo=o + 64 * F * 2, F=F)

    def call(hid, hid_lo, F):
        return _lib.lib().wvn_debug_mlp_x3_frag(ap[0].data_ptr(), ap[1].data_ptr(), w1p[0].data_ptr(), w1p[1].data_ptr(), b1.data_ptr(), hid, hid_lo, w2p.data_ptr(),
                                                b2.data_ptr(), xres.data_ptr(), M, F, 0, 0, _lib.stream())

    return call, base, out


FRAG_ROWS = {
    "N % 64": lambda b: dict(F=96),
    "hi plane null": lambda b: dict(hid=0),
    "lo plane null": lambda b: dict(hid_lo=0),
    "hi plane off 16 bytes": lambda b: dict(hid=b["hid"] + 8),
    "lo plane off 16 bytes": lambda b: dict(hid_lo=b["hid_lo"] + 8),
}


@pytest.mark.parametrize("row", list(FRAG_ROWS))
def test_fragment_planes_refusals(frag, row):
    call, base, out = frag
    refused_then_runs(call, base, FRAG_ROWS[row](base), out)
