"""The SimpleGCN training step without a GPU: the float64 yardstick (tests/simple_gcn_train_ref.py) against autograd, and the host-side
checks of the new entry points."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_gcn_ref as REF  # noqa: E402
import simple_gcn_train_ref as TREF  # noqa: E402

from wild_visual_navigation_amd import _lib  # noqa: E402
from wild_visual_navigation_amd.model import SimpleGCN  # noqa: E402
from wild_visual_navigation_amd.traversability_estimator import GcnTrainer  # noqa: E402


def _case(N=9, D=5, hidden=(7, 3, 1)):
    g = torch.Generator().manual_seed(3)
    sd = REF.glorot_state_dict(D, list(hidden), 7)
    x = 2 * torch.randn(N, D, generator=g, dtype=torch.float64)
    # a directed graph: a path 0 -> 1 -> ... and a few one-way chords, a duplicate and a self loop
    ei = torch.tensor([[i, i + 1] for i in range(N - 1)] + [[0, 4], [0, 4], [7, 2], [3, 3], [8, 1]]).t().contiguous()
    y = torch.rand(N, generator=g, dtype=torch.float64)
    yv = torch.arange(N) % 2 == 0
    return sd, x, ei, y, yv


def _rel(a, b):
    return max(((a[k] - b[k]).abs().max() / b[k].abs().max()).item() for k in b)


@pytest.mark.parametrize("balanced", [True, False])
def test_closed_form_backward_equals_autograd_and_needs_the_transpose(balanced):
    sd, x, ei, y, yv = _case()
    N = x.shape[0]
    A = TREF.dense_adjacency(ei, N)
    assert (A - A.t()).abs().max().item() > 0.1                       # a directed graph: A is not symmetric

    def loss_fn(out):
        return TREF.loss64(out, x, y, yv, 0.03, 0.5, 0.5, anomaly_balanced=balanced)

    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    total = loss_fn(REF.forward(sd64, x, ei))[0]
    want = dict(zip(sd64, torch.autograd.grad(total, list(sd64.values()))))
    z1, z2 = TREF.preactivations(sd, x, A)
    got, res, _ = TREF.backward(sd, x, A, A.t(), (z1 > 0, z2 > 0), loss_fn)
    assert abs(res[0].item() - total.item()) <= 1e-12 * abs(total.item())
    assert _rel(got, want) <= 1e-12, _rel(got, want)
    wrong, _, _ = TREF.backward(sd, x, A, A, (z1 > 0, z2 > 0), loss_fn)
    assert _rel(wrong, want) > 1e-2, _rel(wrong, want)                # A in the place of A^T misses by a wide margin


def test_adam_steps_equal_torch_adam():
    sd, x, ei, y, yv = _case()
    ps = {k: v.double().clone().requires_grad_() for k, v in sd.items()}
    opt = torch.optim.Adam(list(ps.values()), lr=0.05)

    def grads_of(p):
        q = {k: v.detach().requires_grad_() for k, v in p.items()}
        total = TREF.loss64(REF.forward(q, x, ei), x, y, yv, 1.0, 1.0, 0.5)[0]
        return dict(zip(q, torch.autograd.grad(total, list(q.values()))))

    for _ in range(3):
        opt.zero_grad()
        TREF.loss64(REF.forward(ps, x, ei), x, y, yv, 1.0, 1.0, 0.5)[0].backward()
        opt.step()
    want, _, _ = TREF.adam_steps(sd, grads_of, 0.05, 3)
    for k in sd:
        assert (ps[k].detach() - want[k]).abs().max().item() <= 1e-12


def test_entry_points_check_their_arguments_without_a_gpu():
    h = _lib.lib()
    d = _lib.MlpDesc(12, 8, 4, 0)
    N, E = 10, 30
    need = h.wvn_gcn_train_workspace_bytes(C.byref(d), N, E + N)
    assert need > h.wvn_gcn_workspace_bytes(C.byref(d), N, E + N) > 0
    for desc, nodes, cap in ((_lib.MlpDesc(2000, 8, 4, 0), N, E + N), (_lib.MlpDesc(12, 300, 4, 0), N, E + N), (_lib.MlpDesc(12, 8, 4, 1), N, E + N),
                             (d, 0, E), (d, N, N - 1), (d, (1 << 16) + 1, (1 << 16) + 1)):
        assert h.wvn_gcn_train_workspace_bytes(C.byref(desc), nodes, cap) == 0
    assert h.wvn_gcn_train_workspace_bytes(None, N, E + N) == 0
    offs = (C.c_size_t * 3)()
    assert h.wvn_gcn_train_saved(C.byref(d), N, E + N, C.addressof(offs)) == 0
    assert 0 < offs[0] < offs[1] < offs[2] < need and all(o % 256 == 0 for o in offs)
    assert h.wvn_gcn_train_saved(C.byref(d), N, E + N, None) == 1001
    p = 1 << 20   # (never dereferenced: every call below is refused first)
    cd = _lib.ConfDesc(3, 1, p, 0)   # moving_average without minmax

    def a(desc=d, params=p, x=p, ldx=12, ei=p, E=E, yv=p, nodes=N, cap=E + N, stats=p, bad=p, ws=p, nbytes=need, sync=p, conf=None):
        return h.wvn_gcn_train_phase_a(C.byref(desc) if desc else None, params, x, ldx, ei, E, 1, E, yv, nodes, cap, stats, bad, ws, nbytes, sync,
                                       conf, None)

    def b(desc=d, params=p, x=p, ldx=12, y=p, yv=p, nodes=N, cap=E + N, stats=p, grads=p, ws=p, nbytes=need, conf=None):
        return h.wvn_gcn_train_phase_b(C.byref(desc) if desc else None, params, x, ldx, y, yv, nodes, cap, stats, 0.5, 0.03, 0.5, grads, None, ws,
                                       nbytes, conf, None)

    for call in (a, b):
        for kw in ({"desc": None}, {"params": None}, {"x": None}, {"yv": None}, {"stats": None}, {"ws": None}, {"nodes": 0}, {"nodes": -3},
                   {"ldx": 11}, {"nbytes": need - 1}, {"desc": _lib.MlpDesc(2000, 8, 4, 0)}, {"desc": _lib.MlpDesc(12, 8, 0, 0)},
                   {"nodes": (1 << 16) + 1, "cap": 1 << 20}, {"conf": C.byref(cd)}):
            assert call(**kw) == 1001, (call.__name__, kw)
    assert a(ei=None) == 1001 and a(bad=None) == 1001 and a(sync=None) == 1001 and a(E=-1) == 1001 and a(cap=E + N - 1) == 1001
    assert b(y=None) == 1001 and b(grads=None) == 1001


def test_trainer_refuses_an_unknown_method():
    with pytest.raises(ValueError, match="Unknown ConfidenceGenerator method"):
        GcnTrainer(SimpleGCN(12, True, [8, 4, 1]), method="median")
    assert GcnTrainer(SimpleGCN(12, True, [8, 4, 1]), method="kalman_filter")._conf
