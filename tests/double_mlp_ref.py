"""DoubleMLP and its training step in float64, written from the definition (no GPU, no project code):

    networks.0 : D -> h1 -> ReLU -> h2 -> ReLU -> 1 -> sigmoid
    networks.1 : D -> h1 -> ReLU -> h2 -> ReLU -> D
    out = cat([networks.0(x), networks.1(x)], dim=1)

the TraversabilityLoss (loss.py:93-160) with every ConfidenceGenerator method (confidence_generator.py) and torch.optim.Adam's
update.  ``sd`` is a state dict with the keys ``networks.{0,1}.{0,2,4}.{weight,bias}``.
"""
import torch

KEYS = [f"networks.{n}.{i}.{p}" for n in (0, 1) for i in (0, 2, 4) for p in ("weight", "bias")]


def forward(sd, x):
    """x [R, D] -> out [R, 1 + D] in float64 (NaN rows stay NaN: torch.relu keeps them)."""
    x = x.double()
    outs = []
    for n in (0, 1):
        h = x
        for i in (0, 2):
            h = torch.relu(h @ sd[f"networks.{n}.{i}.weight"].double().T + sd[f"networks.{n}.{i}.bias"].double())
        outs.append(h @ sd[f"networks.{n}.4.weight"].double().T + sd[f"networks.{n}.4.bias"].double())
    return torch.cat([torch.sigmoid(outs[0]), outs[1]], dim=1)


def confidence(loss, mean, std, f):
    """ConfidenceGenerator.inference_without_update (confidence_generator.py:182-193)."""
    sh = mean + std * f
    lo, hi = max(sh - std, 0.0), sh + std
    return 1 - (loss.clamp(lo, hi) - lo) / (hi - lo)


def per_segment(sd, feat, seg, mean=0.0, std=1.0, f=0.5):
    """feat [B, S, D], seg [B, H, W] -> (trav, conf, loss_reco) [B, H, W] float64.  Ids in [-S, 0) wrap, any other id outside
    [0, S) gives NaN."""
    B, S, D = feat.shape
    out = forward(sd, feat.reshape(B * S, D))
    loss = ((out[:, 1:] - feat.reshape(B * S, D).double()) ** 2).mean(1)
    table = torch.stack([out[:, 0], confidence(loss, mean, std, f), loss], dim=1).reshape(B, S, 3)
    ids = seg.long()
    ids = torch.where(ids < 0, ids + S, ids)
    bad = (ids < 0) | (ids >= S)
    res = torch.stack([table[b][ids[b].clamp(0, S - 1)] for b in range(B)])   # [B, H, W, 3]
    res[bad] = float("nan")
    return res[..., 0], res[..., 1], res[..., 2]


class F64Step:
    """One optimisation step at a time: forward, confidence update on this step's labelled rows, loss, autograd, Adam."""

    def __init__(self, sd, method="latest_measurement", balanced=True, f=0.5, w_trav=0.03, w_reco=0.5, lr=1e-3):
        self.p = {k: sd[k].double().clone() for k in KEYS}
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.method, self.balanced, self.f, self.w_trav, self.w_reco, self.lr, self.t = method, balanced, f, w_trav, w_reco, lr, 0
        self.mean, self.var, self.std = 0.0, 1.0, 1.0
        self.run = [0.0, 0.0, 0.0]
        self.window = []
        self.grads = None

    def _update(self, lr, pos):
        n, s, s2 = float(pos.numel()), float(pos.sum()), float((pos ** 2).sum())
        if self.method == "running_mean":
            self.run = [self.run[0] + n, self.run[1] + s, self.run[2] + s2]
            self.mean = self.run[1] / self.run[0]
            self.var = self.run[2] / self.run[0] - self.mean ** 2
            self.std = self.var ** 0.5
        elif self.method == "kalman_filter":   # scalar filter: process noise 0.2, measurement noise 1
            if n > 0:
                vp = self.var + 0.2
                k = vp / (vp + 1.0)
                self.mean += k * (s / n - self.mean)
                self.var = (1 - k) * vp
            self.std = self.var ** 0.5
        elif self.method == "moving_average":  # the positives of the last 5 steps
            self.window = (self.window + [pos])[-5:]
            w = torch.cat(self.window)
            self.mean, self.std = float(w.mean()), float(w.std())
        else:
            self.mean, self.std = float(pos.mean()), float(pos.std())
        if self.method == "kalman_filter":
            c = torch.exp(-0.5 * ((lr - self.mean) / (self.std * self.f)) ** 2)
            return torch.where(lr < self.mean, torch.ones_like(c), c)
        if self.method == "moving_average":
            xc = lr.clamp(self.mean - 2 * self.std, self.mean + 2 * self.std)
            return (xc - xc.min()) / (xc.max() - xc.min())
        return confidence(lr, self.mean, self.std, self.f)

    def step(self, x, y, yv):
        """-> ([total, trav (raw mean), reco, conf mean, conf std], confidence [R])"""
        x, y = x.double(), y.double()
        p = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        out = forward(p, x)
        lr = ((out[:, 1:] - x) ** 2).mean(1)
        conf = self._update(lr.detach(), lr.detach()[yv])
        raw = (out[:, 0] - y) ** 2
        trav = torch.where(yv, raw, raw * (1 - conf)).sum() / len(y) if self.balanced else raw.mean()
        loss = self.w_trav * trav + self.w_reco * lr[yv].mean()
        loss.backward()
        self.t += 1
        self.grads = {k: (p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])) for k in KEYS}
        for k in KEYS:
            g = self.grads[k]
            self.m[k] = 0.9 * self.m[k] + 0.1 * g
            self.v[k] = 0.999 * self.v[k] + 0.001 * g * g
            den = (self.v[k] / (1 - 0.999 ** self.t)).sqrt() + 1e-8
            self.p[k] = self.p[k] - self.lr / (1 - 0.9 ** self.t) * self.m[k] / den
        return [loss.item(), raw.mean().item(), lr[yv].mean().item(), self.mean, self.std], conf
