"""float64 statement of the LinearRnvp anomaly-detection mode, written from its definition (no project code, no reference code):
the two-coupling flow, the score, and one AnomalyLoss + Adam step.

State dict (what ``get_model`` builds: two coupling layers with separate s and t networks, each followed by a permutation):
``prior_mean``, ``prior_var``, ``flows.{0,2}.mask``, ``flows.{0,2}.{s,t}.{0,2,4}.{weight,bias}`` (D -> h -> h -> D, ReLU after the
first two linears), ``flows.{1,3}.{p,invp}``.

Per coupling layer, m = mask:  mu = u*m;  s = tanh(S(mu));  t = T(mu);  x = mu + (1-m)*(u*exp(s) + t);  log_det += sum((1-m)*s, 1);
then x = x[:, p].  logprob = -z^2/2 - log(sqrt(2 pi));  score = logprob.sum(1) + log_det.
AnomalyLoss: loss = -mean(score); the confidence statistic is updated with x = x_positive = -score.
"""
import math

import torch

PARAM_KEYS = [f"flows.{f}.{n}.{i}.{w}" for f in (0, 2) for n in ("s", "t") for i in (0, 2, 4) for w in ("weight", "bias")]
KEYS = ["prior_mean", "prior_var"] + [k for f in (0, 2) for k in
                                      ([f"flows.{f}.mask"] + [p for p in PARAM_KEYS if p.startswith(f"flows.{f}.")] +
                                       [f"flows.{f + 1}.p", f"flows.{f + 1}.invp"])]


def expand_sd0(compact):
    """The fixture stores an initial state dict without its ``t`` networks: at construction they are copies of the ``s`` ones."""
    sd = dict(compact)
    for k, v in compact.items():
        if ".s." in k:
            sd[k.replace(".s.", ".t.")] = v.clone()
    return {k: sd[k] for k in KEYS}


def seeded_sd(D, h, seed, mask_type="odds", scale=1.0):
    """A state dict with upstream's shapes and Linear's default value ranges, s and t different (as after training)."""
    g = torch.Generator().manual_seed(seed)
    if mask_type == "odds":
        mask = torch.arange(D).float() % 2
    else:
        mask = torch.zeros(D)
        mask[: D // 2] = 1
    sd = {"prior_mean": torch.zeros(D), "prior_var": torch.ones(D)}
    for f in (0, 2):
        sd[f"flows.{f}.mask"] = mask.clone()
        for n in ("s", "t"):
            for i, (o, k) in zip((0, 2, 4), ((h, D), (h, h), (D, h))):
                b = scale / math.sqrt(k)
                sd[f"flows.{f}.{n}.{i}.weight"] = (torch.rand(o, k, generator=g) * 2 - 1) * b
                sd[f"flows.{f}.{n}.{i}.bias"] = (torch.rand(o, generator=g) * 2 - 1) * b
        p = torch.randperm(D, generator=g)
        sd[f"flows.{f + 1}.p"], sd[f"flows.{f + 1}.invp"] = p, torch.argsort(p)
    return {k: sd[k] for k in KEYS}


def _net(p, pre, x):
    h = torch.relu(x @ p[pre + ".0.weight"].T + p[pre + ".0.bias"])
    h = torch.relu(h @ p[pre + ".2.weight"].T + p[pre + ".2.bias"])
    return h @ p[pre + ".4.weight"].T + p[pre + ".4.bias"]


def flow(sd, x):
    """(z, log_det, score) in float64; differentiable in the float64 tensors of ``sd``."""
    p = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    u = x.double()
    log_det = torch.zeros(u.shape[0], dtype=torch.float64)
    for f in (0, 2):
        m = p[f"flows.{f}.mask"]
        mu = u * m
        s = torch.tanh(_net(p, f"flows.{f}.s", mu))
        t = _net(p, f"flows.{f}.t", mu)
        u = mu + (1 - m) * (u * torch.exp(s) + t)
        log_det = log_det + ((1 - m) * s).sum(1)
        u = u[:, p[f"flows.{f + 1}.p"]]
    score = (-0.5 * u * u - math.log(math.sqrt(2 * math.pi))).sum(1) + log_det
    return u, log_det, score


def interval_confidence(x, mean, std, std_factor):
    """ConfidenceGenerator's interval formula: 1 - (clip(x, lo, hi) - lo) / (hi - lo), lo = max(mean + std f - std, 0), hi = mean + std f + std."""
    shifted = mean + std * std_factor
    lo, hi = max(shifted - std, 0.0), shifted + std
    return 1 - (x.clamp(lo, hi) - lo) / (hi - lo)


class F64Step:
    """AnomalyLoss + torch.optim.Adam(lr, betas (0.9, 0.999), eps 1e-8) in float64, ``latest_measurement`` or ``running_mean``."""

    def __init__(self, sd0, method="latest_measurement", std_factor=0.5, lr=1e-3):
        self.sd = {k: (v.double().clone() if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
        self.method, self.f, self.lr, self.t = method, std_factor, lr, 0
        self.m = {k: torch.zeros_like(self.sd[k]) for k in PARAM_KEYS}
        self.v = {k: torch.zeros_like(self.sd[k]) for k in PARAM_KEYS}
        self.n = self.s1 = self.s2 = 0.0
        self.mean, self.std = 0.0, 1.0

    def step(self, x):
        """One training step on rows x -> (loss, confidence [R]); the statistic is in .mean / .std afterwards."""
        for k in PARAM_KEYS:
            self.sd[k].requires_grad_(True)
        _, _, score = flow(self.sd, x)
        loss = -score.mean()
        grads = torch.autograd.grad(loss, [self.sd[k] for k in PARAM_KEYS])
        a = -score.detach()
        if self.method == "running_mean":
            self.n, self.s1, self.s2 = self.n + a.numel(), self.s1 + a.sum().item(), self.s2 + (a * a).sum().item()
            self.mean = self.s1 / self.n
            self.std = math.sqrt(self.s2 / self.n - self.mean ** 2)
        else:
            self.mean, self.std = a.mean().item(), a.std().item()
        conf = interval_confidence(a, self.mean, self.std, self.f)
        self.t += 1
        with torch.no_grad():
            for k, g in zip(PARAM_KEYS, grads):
                self.sd[k].requires_grad_(False)
                self.m[k] = 0.9 * self.m[k] + 0.1 * g
                self.v[k] = 0.999 * self.v[k] + 0.001 * g * g
                mh, vh = self.m[k] / (1 - 0.9 ** self.t), self.v[k] / (1 - 0.999 ** self.t)
                self.sd[k] -= self.lr * mh / (vh.sqrt() + 1e-8)
        return loss.item(), conf
