"""The SimpleGCN training step stated in float64 on the CPU: the yardstick of the fused step (csrc/simple_gcn_train.hip).

    loss64      TraversabilityLoss (utils/loss.py) on float64 tensors, for every ConfidenceGenerator method and both
                ``anomaly_balanced`` forms (another method than latest_measurement takes its confidence from a ConfidenceGenerator
                that the caller keeps between steps)
    backward    the closed-form backward with an explicit dense A^T and the ReLU masks PASSED IN:
                    Z_l = A X_{l-1} W_l^T + b_l,  X_l = Z_l * mask_l,  G_l = dL/dZ_l
                    T_l = A^T G_l,  dW_l = T_l^T X_{l-1},  db_l = column sums of G_l,  G_{l-1} = (T_l W_l) * mask_{l-1}
                (only the seed G_3 = dL/dZ_3 comes from autograd, over the loss alone)
    adam_steps  k torch.optim.Adam steps in float64
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_gcn_ref as REF  # noqa: E402

W = ["layers.0.lin.weight", "layers.1.lin.weight", "layers.2.lin.weight"]
B = ["layers.0.bias", "layers.1.bias", "layers.2.bias"]


def dense_adjacency(edge_index, N, dtype=torch.float64):
    """A [N, N]: A[i, j] = sum of coef_e over the edges j -> i of the normalised graph (self loops re-added, duplicates kept)."""
    src, dst, deg = REF.normalised_graph(edge_index.cpu(), N)
    dinv = torch.tensor(deg, dtype=dtype).pow(-0.5)
    A = torch.zeros(N, N, dtype=dtype)
    for j, i in zip(src, dst):
        A[i, j] += dinv[j] * dinv[i]
    return A


def loss64(out, x, y, yv, w_trav, w_reco, std_factor, method="latest_measurement", anomaly_balanced=True, cg=None):
    """-> (total, mean raw traversability loss, mean reconstruction loss of the labelled rows, confidence)."""
    loss_reco = ((out[:, 1:] - x) ** 2).mean(1)
    with torch.no_grad():
        if method == "latest_measurement":
            pos = loss_reco[yv]
            conf = REF.table(out, x, pos.mean().item(), pos.std().item(), std_factor)[2]
        else:
            conf = cg.update(x=loss_reco.detach(), x_positive=loss_reco.detach()[yv]).to(out.dtype)
    raw = (out[:, 0] - y) ** 2
    # (the row weight is a constant of the step: stated outside the product, a NaN confidence -- fewer than two labelled rows -- of
    #  a labelled row stays out of that row's gradient, where torch.where's backward would multiply it by zero)
    weight = torch.where(yv, torch.ones_like(conf), 1 - conf)
    trav = (raw * weight).sum() / y.shape[0] if anomaly_balanced else raw.mean()
    return w_trav * trav + w_reco * loss_reco[yv].mean(), raw.mean(), loss_reco[yv].mean(), conf


def preactivations(sd, x, A):
    """float64 pre-activations (Z_1, Z_2) of the hidden layers with float64's own ReLU."""
    p = {k: v.detach().double() for k, v in sd.items()}
    z1 = A @ x.double() @ p[W[0]].t() + p[B[0]]
    z2 = A @ torch.relu(z1) @ p[W[1]].t() + p[B[1]]
    return z1, z2


def backward(sd, x, A, At, masks, loss_fn):
    """Closed-form gradients {state-dict key: tensor} of ``loss_fn(out)[0]`` in float64; masks = (m1 [N, h1], m2 [N, h2]) as 0 / 1
    tensors; ``At`` is the operator of the backward (pass A in its place to see what the symmetric shortcut gives)."""
    p = {k: v.detach().double() for k, v in sd.items()}
    x = x.double()
    m1, m2 = (m.double() for m in masks)
    x1 = (A @ x @ p[W[0]].t() + p[B[0]]) * m1
    x2 = (A @ x1 @ p[W[1]].t() + p[B[1]]) * m2
    z3 = (A @ x2 @ p[W[2]].t() + p[B[2]]).requires_grad_()
    out = torch.cat([torch.sigmoid(z3[:, :1]), z3[:, 1:]], dim=1)
    res = loss_fn(out)
    (g,) = torch.autograd.grad(res[0], z3)
    grads = {}
    for l, (xin, mask) in zip((2, 1, 0), ((x2, m2), (x1, m1), (x, None))):
        t = At @ g
        grads[W[l]] = t.t() @ xin
        grads[B[l]] = g.sum(0)
        if mask is not None:
            g = (t @ p[W[l]]) * mask
    return grads, res, out.detach()


def adam_steps(sd, grads_of, lr, k, eps=1e-8, b1=0.9, b2=0.999):
    """k Adam steps in float64 from zero moments; ``grads_of(sd)`` -> {key: gradient}.  -> (parameters, m, v)."""
    p = {n: v.detach().double().clone() for n, v in sd.items()}
    m = {n: torch.zeros_like(v) for n, v in p.items()}
    v = {n: torch.zeros_like(u) for n, u in p.items()}
    for t in range(1, k + 1):
        g = grads_of(p)
        for n in p:
            gn = g[n].double()
            m[n] = b1 * m[n] + (1 - b1) * gn
            v[n] = b2 * v[n] + (1 - b2) * gn * gn
            p[n] = p[n] - lr * (m[n] / (1 - b1 ** t)) / ((v[n] / (1 - b2 ** t)).sqrt() + eps)
    return p, m, v


def flat_to_dict(flat, sd):
    """The flat buffer [W1|b1|W2|b2|W3|b3] -> {state-dict key: tensor}."""
    out, off = {}, 0
    for l in range(3):
        for k in (W[l], B[l]):
            n = sd[k].numel()
            out[k] = flat[off:off + n].reshape(sd[k].shape)
            off += n
    return out
