"""Pin the training step with every ConfidenceGenerator method against the reference's OWN code and write
tests/golden/mlp_train_methods.pt.

Run in the build container only (needs the reference checkout that oracle.pin_reference.import_reference() loads; nothing under
oracle/ is changed):

    python scripts/pin_train_methods.py

Contents (all tensors on the CPU; inputs and initial weights are those of mlp_train.pt, not repeated here):
  cases[name]         name = "<method>_<balanced|unbalanced>": the reference's SimpleMLP + TraversabilityLoss + Adam(lr 1e-3) for
                      12 steps on the graph_pt_D90 rows of mlp_train.pt; step t trains on rows[t] (a seeded subset, R varies,
                      >= 2 labelled rows so that every unbiased std is finite).  traj [12, 6] = {total, trav, reco, mean, var, std}
                      after each step, conf[t] = the confidence update() returned in step t, sd12 = the final model state dict,
                      cg12 = the final ConfidenceGenerator state dict.
  d384[method]        the same for the synthetic_D384 rows (rows, traj; no state dicts), balanced
  updates[method]     host update() sequences: xs, xps (one positive set is empty), conf / mean / var / std after each update
  keys[method]        the ConfidenceGenerator state-dict (key, shape, dtype) list
  ref_loss_sd[method] the reference's traversability_loss_state_dict after the running_mean / kalman_filter balanced cases
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.pin_reference import import_reference  # noqa: E402

METHODS = ("latest_measurement", "running_mean", "kalman_filter", "moving_average")
CASES = [(m, b) for m in METHODS[1:] for b in (True, False)] + [("latest_measurement", False)]
STEPS = 12


def row_subsets(yv: torch.Tensor, seed: int):
    g = torch.Generator().manual_seed(seed)
    lab, unl = torch.nonzero(yv).flatten(), torch.nonzero(~yv).flatten()
    out = []
    for _ in range(STEPS):
        k = int(torch.randint(2, min(8, lab.numel()) + 1, (1,), generator=g))
        u = int(torch.randint(10, unl.numel() + 1, (1,), generator=g))
        rows = torch.cat([lab[torch.randperm(lab.numel(), generator=g)[:k]], unl[torch.randperm(unl.numel(), generator=g)[:u]]])
        out.append(rows.sort().values)
    return out


def run(x, y, yv, rows, method, balanced, sd0):
    from wild_visual_navigation.model.simple_mlp import SimpleMLP
    from wild_visual_navigation.utils.data import Data
    from wild_visual_navigation.utils.loss import TraversabilityLoss

    model = SimpleMLP(input_size=x.shape[1], hidden_sizes=[256, 32, 1], reconstruction=True)
    model.load_state_dict(sd0)
    model.train()
    loss_fn = TraversabilityLoss(w_trav=0.03, w_reco=0.5, w_temp=0.0, anomaly_balanced=balanced, model=model, method=method,
                                 confidence_std_factor=0.5, log_enabled=False, log_folder="/tmp")
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    cg = loss_fn._confidence_generator
    traj, conf = [], []
    for step, r in enumerate(rows):
        batch = Data(x=x[r], y=y[r], y_valid=yv[r])
        res = model(batch)
        loss, aux, _ = loss_fn(batch, res, step=step, log_step=False)
        opt.zero_grad()
        loss.backward()
        opt.step()
        traj.append([loss.item(), aux["loss_trav"].item(), aux["loss_reco"].item(), cg.mean.item(), cg.var.item(), cg.std.item()])
        conf.append(aux["confidence"].detach().clone())
        assert all(v == v for v in traj[-1]), (method, balanced, step, traj[-1])
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    cgsd = {k: v.detach().clone() for k, v in cg.state_dict().items()}
    return torch.tensor(traj, dtype=torch.float32), conf, sd, cgsd, loss_fn


def updates(method):
    from wild_visual_navigation.utils.confidence_generator import ConfidenceGenerator

    g = torch.Generator().manual_seed(11)
    cg = ConfidenceGenerator(std_factor=0.5, method=method, log_enabled=False, log_folder="/tmp")
    xs, xps, conf, mean, var, std = [], [], [], [], [], []
    for i in range(9):
        x = torch.rand(int(torch.randint(6, 20, (1,), generator=g)), generator=g) * 3.0
        xp = x[:0] if i == 4 else x[: int(torch.randint(2, 6, (1,), generator=g))]
        c = cg.update(x, xp, step=i)
        xs.append(x)
        xps.append(xp.clone())
        conf.append(c.clone())
        mean.append(cg.mean.detach().clone())
        var.append(cg.var.detach().clone())
        std.append(cg.std.detach().clone())
    keys = [(k, tuple(v.shape), str(v.dtype)) for k, v in cg.state_dict().items()]
    return {"xs": xs, "xps": xps, "conf": conf, "mean": mean, "var": var, "std": std}, keys


def main():
    import_reference()
    src = torch.load(os.path.join(ROOT, "tests", "golden", "mlp_train.pt"), weights_only=False)
    c90, c384 = src["graph_pt_D90"], src["synthetic_D384"]
    out = {"cases": {}, "d384": {}, "updates": {}, "keys": {}, "ref_loss_sd": {}}
    rows = row_subsets(c90["y_valid"], 1)
    for method, balanced in CASES:
        traj, conf, sd, cgsd, loss_fn = run(c90["x"], c90["y"], c90["y_valid"], rows, method, balanced, c90["sd0"])
        name = f"{method}_{'balanced' if balanced else 'unbalanced'}"
        for other in out["cases"].values():   # (unbalanced runs do not feed the confidence into the loss: their weights agree
            if all(torch.equal(sd[k], other["sd12"][k]) for k in sd):   # bit for bit; store such a state dict once)
                sd = other["sd12"]
                break
        out["cases"][name] = {"method": method, "balanced": balanced, "rows": rows, "traj": traj, "conf": conf, "sd12": sd,
                              "cg12": cgsd}
        if balanced and method in ("running_mean", "kalman_filter"):
            # the model entries share storage with sd12 (saved once)
            full = {}
            for k, v in loss_fn.state_dict().items():
                full[k] = sd[k[len("_model."):]] if k.startswith("_model.") else v.detach().clone()
            out["ref_loss_sd"][method] = full
        print(f"{name}: loss {traj[0, 0]:.5f} -> {traj[-1, 0]:.5f}, mean/var/std {traj[-1, 3:].tolist()}")
    rows384 = row_subsets(c384["y_valid"], 2)
    for method in METHODS[1:]:
        traj, _, _, _, _ = run(c384["x"], c384["y"], c384["y_valid"], rows384, method, True, c384["sd0"])
        out["d384"][method] = {"rows": rows384, "traj": traj}
        print(f"D384 {method}: loss {traj[0, 0]:.5f} -> {traj[-1, 0]:.5f}")
    for method in METHODS:
        out["updates"][method], out["keys"][method] = updates(method)
    path = os.path.join(ROOT, "tests", "golden", "mlp_train_methods.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
