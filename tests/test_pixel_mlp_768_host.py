"""Host-side size queries of the fused per-pixel kernels at D = 768 (ViT-Base features), through the C ABI: the formulas
include/wvn_hip.h documents.  No GPU needed."""
import ctypes as C

from wild_visual_navigation_amd import _lib


def test_per_pixel_host_queries_768():
    h = _lib.lib()
    d = _lib.MlpDesc(768, 256, 32, 0)
    tiles = 768 // 32 + 1                                              # 24 reconstruction tiles + the traversability tile
    w2, w3 = 16 * 2 * 32 * 16, tiles * 2 * 2 * 32 * 16               # W2 and W3 fragment images (bf16)
    nbias = 256 + 32 + tiles * 32
    assert h.wvn_pixel_mlp_zx_cols(C.byref(d)) == 1024
    assert h.wvn_pixel_mlp_pack_bytes(C.byref(d)) == 256 * 768 * 2 + w2 + w3 + 4 * nbias
    assert h.wvn_pixel_mlp_exact_pack_bytes(C.byref(d)) == 2 * (w2 + w3) + 4 * nbias
    for B, G in ((1, 14), (2, 56), (16, 37)):
        rows = B * G * G
        assert h.wvn_pixel_mlp_exact_workspace_bytes(C.byref(d), B, G) == rows * 256 * 4 + 2 * rows * 1024 * 2 + 256


def test_only_three_input_sizes_are_supported():
    h = _lib.lib()
    for D in (64, 89, 91, 383, 385, 767, 769, 1024, 1536):
        d = _lib.MlpDesc(D, 256, 32, 0)
        assert h.wvn_pixel_mlp_pack_bytes(C.byref(d)) == 0 and h.wvn_pixel_mlp_exact_pack_bytes(C.byref(d)) == 0
        assert h.wvn_pixel_mlp_zx_cols(C.byref(d)) == 0 and h.wvn_pixel_mlp_exact_workspace_bytes(C.byref(d), 1, 14) == 0
