"""Host-side contract of the fused per-segment inference (csrc/segment_predict.hip): the workspace query and the argument checks of
wvn_segment_predict, which refuse before any GPU call (runs without a GPU)."""
import ctypes as C

from wild_visual_navigation_amd import _lib

ERR_ARG = 1001
P = 1 << 20   # a 16-byte aligned stand-in pointer (never dereferenced: every call below is refused first)


def test_workspace_query():
    h = _lib.lib()
    for D in (90, 384, 768, 1, 1024):
        d = _lib.MlpDesc(D, 256, 32, 0)
        assert h.wvn_segment_predict_workspace_bytes(C.byref(d), 1, 20) == 20 * 4 * 4      # {trav, conf, loss, pad} per segment
        assert h.wvn_segment_predict_workspace_bytes(C.byref(d), 64, 196) == 64 * 196 * 16
    d = _lib.MlpDesc(384, 256, 32, 0)
    assert h.wvn_segment_predict_workspace_bytes(C.byref(d), 0, 20) == 0
    assert h.wvn_segment_predict_workspace_bytes(C.byref(d), 1, 0) == 0
    assert h.wvn_segment_predict_workspace_bytes(None, 1, 20) == 0
    for D, h1, h2 in ((1025, 256, 32), (0, 256, 32), (384, 128, 32), (384, 256, 16)):
        assert h.wvn_segment_predict_workspace_bytes(C.byref(_lib.MlpDesc(D, h1, h2, 0)), 1, 20) == 0


def _call(desc=None, params=P, feat=P, ld_row=384, ld_frame=20 * 384, B=2, S=20, seg=P, seg_bytes=4, H=37, W=53,
          trav=P, conf=P, loss=None, ws=P, ws_bytes=1 << 16, conf_state=None):
    d = desc if desc is not None else _lib.MlpDesc(384, 256, 32, 0)
    return _lib.lib().wvn_segment_predict(C.byref(d), params, feat, ld_row, ld_frame, B, S, seg, seg_bytes, H, W, 0.9, 0.25, 0.5,
                                          conf_state, trav, conf, loss, ws, ws_bytes, None)


def test_argument_validation_without_gpu():
    h = _lib.lib()
    assert h.wvn_segment_predict(None, P, P, 384, 0, 1, 20, P, 4, 8, 8, 0.0, 1.0, 0.5, None, P, P, None, P, 1 << 16, None) == ERR_ARG
    for k in ("params", "feat", "seg", "ws"):
        assert _call(**{k: None}) == ERR_ARG, k
    for k in ("B", "S", "H", "W"):
        assert _call(**{k: 0}) == ERR_ARG, k
        assert _call(**{k: -1}) == ERR_ARG, k
    assert _call(seg_bytes=2) == ERR_ARG and _call(seg_bytes=1) == ERR_ARG and _call(seg_bytes=16) == ERR_ARG
    assert _call(desc=_lib.MlpDesc(1025, 256, 32, 0), ld_row=1025) == ERR_ARG       # D beyond 1024
    assert _call(desc=_lib.MlpDesc(384, 128, 32, 0)) == ERR_ARG                     # H1 = 128
    assert _call(desc=_lib.MlpDesc(384, 256, 64, 0)) == ERR_ARG                     # H2 = 64
    assert _call(ld_row=383) == ERR_ARG                                             # rows shorter than D
    assert _call(ld_frame=-1) == ERR_ARG
    assert _call(params=P + 4) == ERR_ARG and _call(ws=P + 8) == ERR_ARG           # 16-byte alignment
    assert _call(seg_bytes=8, seg=P + 4) == ERR_ARG                                 # int64 ids on a 4-byte boundary
    # a workspace smaller than the query's answer
    need = h.wvn_segment_predict_workspace_bytes(C.byref(_lib.MlpDesc(384, 256, 32, 0)), 2, 20)
    assert _call(ws_bytes=need - 1) == 1002
