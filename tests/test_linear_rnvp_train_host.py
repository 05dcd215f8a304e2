"""The LinearRnvp training step, host side (no GPU): the wvn_rnvp_train_* symbols, their sizes and their argument checks, which
refuse before any GPU call, and the estimator's CPU route, which keeps autograd and ``torch.optim.Adam``."""
import ctypes as C
import os
import re

import torch

from wild_visual_navigation_amd import _lib
from wild_visual_navigation_amd.cfg import ExperimentParams
from wild_visual_navigation_amd.traversability_estimator import RnvpTrainer, TraversabilityEstimator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1001
P = 1 << 20   # a stand-in device pointer (never dereferenced: every call below is refused first)
NAMES = ("wvn_rnvp_train_param_count", "wvn_rnvp_train_workspace_bytes", "wvn_rnvp_train_pack_bytes", "wvn_rnvp_train_pack",
         "wvn_rnvp_train_phase_a", "wvn_rnvp_train_phase_b", "wvn_rnvp_train_phase_c")


def test_symbols_are_declared_exported_and_bound():
    h = _lib.lib()
    with open(os.path.join(ROOT, "include", "wvn_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(h, name)


def test_sizes():
    h = _lib.lib()
    d384, d90 = _lib.RnvpDesc(384, 200, 2), _lib.RnvpDesc(90, 200, 2)
    assert h.wvn_rnvp_train_param_count(C.byref(d384)) == 777536
    assert h.wvn_rnvp_train_param_count(C.byref(d90)) == 305960
    T = h.wvn_rnvp_row_tile()
    for d in (d384, d90, _lib.RnvpDesc(90, 256, 2)):
        w = [h.wvn_rnvp_train_workspace_bytes(C.byref(d), R) for R in (0, 1, T, T + 1, 8 * T, 800)]
        assert w[0] > 0 and w[1] == w[2] and w[2] < w[3] < w[4] < w[5]      # grows with R, tile by tile
        assert h.wvn_rnvp_train_pack_bytes(C.byref(d)) > 0
    assert h.wvn_rnvp_train_workspace_bytes(C.byref(d384), -1) == 0
    for bad in (_lib.RnvpDesc(64, 200, 2), _lib.RnvpDesc(384, 300, 2), _lib.RnvpDesc(384, 200, 3)):
        b = C.byref(bad)
        assert h.wvn_rnvp_train_param_count(b) == 0 and h.wvn_rnvp_train_workspace_bytes(b, 8) == 0
        assert h.wvn_rnvp_train_pack_bytes(b) == 0
    assert h.wvn_rnvp_train_param_count(None) == 0


def test_entry_points_check_arguments_on_the_host():
    h = _lib.lib()
    ok = _lib.RnvpDesc(384, 200, 2)
    d = C.byref(ok)
    big = h.wvn_rnvp_train_workspace_bytes(d, 800)

    def pack(desc=d, params=P, packed=P, tpacked=P):
        return h.wvn_rnvp_train_pack(desc, params, packed, tpacked, None)

    def a(desc=d, packed=P, x=P, ldx=384, R=8, score=P, stats=P, ws=P, ws_bytes=big):
        return h.wvn_rnvp_train_phase_a(desc, packed, x, ldx, R, score, stats, ws, ws_bytes, None)

    def b(desc=d, packed=P, tpacked=P, R=8, stats=P, grads=P, ws=P, ws_bytes=big):
        return h.wvn_rnvp_train_phase_b(desc, packed, tpacked, R, stats, grads, ws, ws_bytes, None)

    def c(desc=d, params=P, grads=P, m=P, v=P, step=1, stats=P, method=0, cstate=P, losses=P, mask=P, perm=P, packed=P, tpacked=P):
        return h.wvn_rnvp_train_phase_c(desc, params, grads, m, v, step, 1e-3, stats, method, cstate, losses, mask, perm, packed,
                                        tpacked, None)

    for bad in (_lib.RnvpDesc(64, 200, 2), _lib.RnvpDesc(384, 300, 2), _lib.RnvpDesc(768, 200, 2), _lib.RnvpDesc(384, 200, 3)):
        for fn in (pack, a, b, c):
            assert fn(desc=C.byref(bad)) == ERR_ARG
    for fn in (pack, a, b, c):
        assert fn(desc=None) == ERR_ARG
    for kw in (dict(params=None), dict(packed=None), dict(tpacked=None), dict(packed=P + 8), dict(tpacked=P + 4)):
        assert pack(**kw) == ERR_ARG, kw
    small = h.wvn_rnvp_train_workspace_bytes(d, 8)
    for kw in (dict(packed=None), dict(packed=P + 8), dict(x=None), dict(score=None), dict(stats=None), dict(ws=None), dict(ldx=383),
               dict(R=-1), dict(R=1 << 31), dict(ws_bytes=0), dict(ws_bytes=small - 1), dict(R=33, ws_bytes=small)):
        assert a(**kw) == ERR_ARG, kw
    for kw in (dict(packed=None), dict(tpacked=None), dict(stats=None), dict(grads=None), dict(ws=None), dict(R=-1),
               dict(ws_bytes=small - 1), dict(R=33, ws_bytes=small)):
        assert b(**kw) == ERR_ARG, kw
    for kw in (dict(params=None), dict(grads=None), dict(m=None), dict(v=None), dict(step=0), dict(stats=None), dict(method=4),
               dict(method=-1), dict(cstate=None), dict(losses=None), dict(mask=None), dict(perm=None), dict(packed=None),
               dict(tpacked=None)):
        assert c(**kw) == ERR_ARG, kw


def test_cpu_estimator_keeps_autograd_and_adam():
    p = ExperimentParams()
    p.model.name = "LinearRnvp"
    p.model.linear_rnvp_cfg.input_size = 90
    te = TraversabilityEstimator(p, device="cpu", anomaly_detection=True)
    assert isinstance(te._optimizer, torch.optim.Adam) and not isinstance(te._optimizer, RnvpTrainer)
    tr = RnvpTrainer(te._model)
    sd = tr.optimizer_state_dict()          # torch.optim.Adam.state_dict() shape: 24 parameters, empty state before the first step
    assert sd["state"] == {} and sd["param_groups"][0]["params"] == list(range(24))
    torch.optim.Adam(te._model.parameters(), lr=1e-3).load_state_dict(sd)
