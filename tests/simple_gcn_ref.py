"""SimpleGCN stated from its definition (the published closed form of torch_geometric's GCNConv with its defaults), in any float
dtype: float64 is the reference the kernels are held to, the same statement in float32 on the CPU is the yardstick of the
accuracy rule.  The graph is normalised in plain Python loops over the edge list; a layer is

    1. every edge with source j == target i dropped, then exactly one self loop per node added (duplicates stay duplicated)
    2. deg_i = number of edges whose target is i after step 1 (>= 1)
    3. coef_e = deg_j^-1/2 deg_i^-1/2
    4. out_i = sum_{e: j -> i} coef_e (x_j W^T) + b

and the model is D -> h1 (ReLU) -> h2 (ReLU) -> 1 + D with the sigmoid on column 0.  ``edge_index`` [2, E]: row 0 = source, row 1
= target, used as given (not symmetrised).  Every endpoint must lie in [0, N): dropping bad edges is the kernels' business."""
import math

import torch

KEYS = ["layers.0.bias", "layers.0.lin.weight", "layers.1.bias", "layers.1.lin.weight", "layers.2.bias", "layers.2.lin.weight"]


def normalised_graph(edge_index, N):
    """-> (src, dst, deg) as Python lists: steps 1 and 2."""
    src, dst = [], []
    for j, i in zip(edge_index[0].tolist(), edge_index[1].tolist()):
        assert 0 <= j < N and 0 <= i < N, (j, i, N)
        if j != i:
            src.append(j)
            dst.append(i)
    for n in range(N):
        src.append(n)
        dst.append(n)
    deg = [0] * N
    for i in dst:
        deg[i] += 1
    return src, dst, deg


def gcn_layer(x, graph, W, b):
    src, dst, deg = graph
    dinv = torch.tensor(deg, dtype=x.dtype).pow(-0.5)
    s, d = torch.tensor(src, dtype=torch.long), torch.tensor(dst, dtype=torch.long)
    xw = x @ W.t()
    out = torch.zeros(x.shape[0], W.shape[0], dtype=x.dtype)
    out.index_add_(0, d, xw[s] * (dinv[s] * dinv[d])[:, None])
    return out + b


def forward(sd, x, edge_index, dtype=torch.float64):
    """state dict (PyG keys), x [N, D], edge_index [2, E] -> [N, 1 + D] in ``dtype`` on the CPU; differentiable in ``sd``."""
    x = x.detach().cpu().to(dtype)
    p = {k: v.cpu().to(dtype) if not v.requires_grad else v for k, v in sd.items()}
    graph = normalised_graph(edge_index.cpu(), x.shape[0])
    h = torch.relu(gcn_layer(x, graph, p["layers.0.lin.weight"], p["layers.0.bias"]))
    h = torch.relu(gcn_layer(h, graph, p["layers.1.lin.weight"], p["layers.1.bias"]))
    o = gcn_layer(h, graph, p["layers.2.lin.weight"], p["layers.2.bias"])
    return torch.cat([torch.sigmoid(o[:, :1]), o[:, 1:]], dim=1)


def glorot_state_dict(D, hidden, seed):
    """Glorot-uniform weights; the biases are small random numbers, not the default zeros, so that a bias error shows."""
    g = torch.Generator().manual_seed(seed)
    sizes = [D, hidden[0], hidden[1], 1 + D]
    sd = {}
    for l in range(3):
        a = math.sqrt(6.0 / (sizes[l] + sizes[l + 1]))
        sd[f"layers.{l}.bias"] = 0.1 * torch.randn(sizes[l + 1], generator=g)
        sd[f"layers.{l}.lin.weight"] = (2 * torch.rand(sizes[l + 1], sizes[l], generator=g) - 1) * a
    return {k: sd[k] for k in KEYS}


def bound(got, sd, x, edge_index):
    """The accuracy rule: (max abs error of ``got`` against the float64 statement, the bound) with the bound the larger of
    8 x the error of the float32 statement on the CPU on the same inputs and 2^-16 x max|float64 output|."""
    ref64 = forward(sd, x, edge_index, torch.float64)
    ref32 = forward(sd, x, edge_index, torch.float32).double()
    return rule(got, ref64, ref32)


def rule(got, ref64, ref32):
    err = (got.detach().cpu().double() - ref64).abs().max().item()
    err32 = (ref32.double() - ref64).abs().max().item()
    return err, max(8 * err32, 2.0 ** -16 * ref64.abs().max().item()), err32


def table(out, x, mean, std, std_factor):
    """[N, 1 + D] forward output and its input -> (trav, loss_reco, conf) per row in the dtype of ``out``
    (confidence_generator.py:182-193, inference_without_update)."""
    x = x.detach().cpu().to(out.dtype)
    loss = ((out[:, 1:] - x) ** 2).mean(1)
    shifted = mean + std * std_factor
    lo, hi = max(shifted - std, 0.0), shifted + std
    conf = 1 - (loss.clip(lo, hi) - lo) / (hi - lo)
    return out[:, 0], loss, conf


def adam_step(sd, grads, lr, eps=1e-8, b1=0.9, b2=0.999):
    """The first torch.optim.Adam step (zero moments) in float64."""
    new = {}
    for k, p in sd.items():
        g = grads[k].double()
        m, v = (1 - b1) * g, (1 - b2) * g * g
        new[k] = p.double() - lr * (m / (1 - b1)) / ((v / (1 - b2)).sqrt() + eps)
    return new
