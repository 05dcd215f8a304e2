"""Pin the anomaly-detection mode against the reference's OWN LinearRnvp and AnomalyLoss and write tests/golden/linear_rnvp.pt.

Run in the build container only (needs the reference checkout that oracle.pin_reference.import_reference() loads; nothing under
oracle/ is changed):

    python scripts/pin_linear_rnvp.py

Contents (all tensors on the CPU; the x rows are those of mlp_train.pt, not repeated here):
  d90.sd0            the seeded initial state dict of the reference's LinearRnvp(90, [200], use_permutation=True), WITHOUT its t
                     networks: at construction they are deep copies of the s networks (tests/linear_rnvp_ref.py: expand_sd0), and
                     with them the file would pass the size limit of a committed file
  d90.z / log_det / logprob_sum   the reference's forward on the 100 graph_pt_D90 rows
  d90.own_err        the reference's fp32 score against the float64 statement tests/linear_rnvp_ref.py: {"abs", "rel"} (max abs,
                     and that over max |score|), and "score_max" = max |score|
  d90.cases[method]  method = latest_measurement, running_mean: the reference's LinearRnvp + AnomalyLoss + Adam(lr 1e-3) for 12 steps,
                     every step on all 100 rows (in this mode a batch holds the labelled rows only, and all of them are positives):
                     traj [12, 3] = {loss, generator mean, generator std} after each step, conf[t] = the confidence returned in
                     step t, loss_sd12 = the final AnomalyLoss state dict, final = the trained model's z / log_det / logprob_sum on
                     the rows, sd12_shapes = keys and shapes of the final model state dict.  (The two final model state dicts
                     themselves are 1.2 MB each: over the limit.  What the trained weights compute is stored instead.)
  d384.own_err       the same own-error record for LinearRnvp(384, [200]) with seeded weights on the 160 synthetic_D384 rows; the
                     weights are too large to store, so the float64 statement is checked against the reference here, at pin time
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import linear_rnvp_ref as REF  # noqa: E402
from oracle.pin_reference import import_reference  # noqa: E402

H = 200
STEPS = 12
METHODS = ("latest_measurement", "running_mean")


def new_model(D, sd=None):
    from wild_visual_navigation.model import LinearRnvp

    model = LinearRnvp(input_size=D, coupling_topology=[H], mask_type="odds", conditioning_size=0, use_permutation=True,
                       single_function=False)
    if sd is not None:
        model.load_state_dict(sd)
    return model


def clone_sd(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def forward(model, x):
    from wild_visual_navigation.utils.data import Data

    with torch.no_grad():
        res = model(Data(x=x.clone()))
    return {"z": res["z"].clone(), "log_det": res["log_det"].clone(), "logprob_sum": res["logprob"].sum(1).clone()}


def own_error(model, sd, x):
    out = forward(model, x)
    z64, ld64, score64 = REF.flow(sd, x)
    score = (out["logprob_sum"] + out["log_det"]).double()
    err = (score - score64).abs().max().item()
    assert (out["z"].double() - z64).abs().max().item() < 1e-4 * max(1.0, z64.abs().max().item()), "the float64 statement disagrees (z)"
    assert (out["log_det"].double() - ld64).abs().max().item() < 1e-3, "the float64 statement disagrees (log_det)"
    assert err < 1e-5 * score64.abs().max().item() + 1e-3, "the float64 statement disagrees (score)"
    return {"abs": err, "rel": err / score64.abs().max().item(), "score_max": score64.abs().max().item()}


def run(x, sd0, method):
    from wild_visual_navigation.utils.data import Data
    from wild_visual_navigation.utils.loss import AnomalyLoss

    model = new_model(x.shape[1], sd0)
    model.train()
    loss_fn = AnomalyLoss(confidence_std_factor=0.5, method=method, log_enabled=False, log_folder="/tmp")
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    cg = loss_fn._confidence_generator
    ref = REF.F64Step(sd0, method)
    traj, conf = [], []
    for step in range(STEPS):
        batch = Data(x=x.clone())
        loss, aux, _ = loss_fn(batch, model(batch), step=step, log_step=False)
        opt.zero_grad()
        loss.backward()
        opt.step()
        traj.append([loss.item(), cg.mean.item(), cg.std.item()])
        conf.append(aux["confidence"].detach().clone())
        want_loss, want_conf = ref.step(x)   # the float64 statement follows the reference's trajectory
        assert abs(want_loss - traj[-1][0]) < 3e-4 * abs(want_loss), (method, step, want_loss, traj[-1])
        assert abs(ref.mean - traj[-1][1]) < 3e-4 * abs(ref.mean) and abs(ref.std - traj[-1][2]) < 1e-3 * ref.std, (method, step)
        print(f"  {method} step {step}: loss {traj[-1][0]:.4f} mean {traj[-1][1]:.4f} std {traj[-1][2]:.4f} "
              f"own conf err {(conf[-1].double() - want_conf).abs().max().item():.2e}")
    model.eval()
    return {"method": method, "traj": torch.tensor(traj, dtype=torch.float32), "conf": conf,
            "loss_sd12": {k: v.detach().clone() for k, v in loss_fn.state_dict().items()},
            "final": forward(model, x), "sd12_shapes": {k: tuple(v.shape) for k, v in model.state_dict().items()}}


def main():
    import_reference()
    src = torch.load(os.path.join(ROOT, "tests", "golden", "mlp_train.pt"), weights_only=False)
    x90, x384 = src["graph_pt_D90"]["x"], src["synthetic_D384"]["x"]
    torch.manual_seed(42)   # seed_everything(42), traversability_estimator.py:78
    m90 = new_model(90)
    sd0 = clone_sd(m90)
    assert list(sd0) == REF.KEYS, "state-dict keys of the reference changed"
    assert all(torch.equal(sd0[k], sd0[k.replace(".s.", ".t.")]) for k in sd0 if ".s." in k)
    compact = {k: v for k, v in sd0.items() if ".t." not in k}
    assert all(torch.equal(v, sd0[k]) for k, v in REF.expand_sd0(compact).items())
    out = {"hidden": H, "d90": {"sd0": compact, "cases": {}}, "d384": {}}
    out["d90"].update(forward(m90, x90))
    out["d90"]["own_err"] = own_error(m90, sd0, x90)
    print("D = 90 own error:", out["d90"]["own_err"])
    for method in METHODS:
        out["d90"]["cases"][method] = run(x90, sd0, method)
    torch.manual_seed(43)
    m384 = new_model(384)
    out["d384"]["own_err"] = own_error(m384, clone_sd(m384), x384)
    print("D = 384 own error:", out["d384"]["own_err"])
    path = os.path.join(ROOT, "tests", "golden", "linear_rnvp.pt")
    torch.save(out, path)
    size = os.path.getsize(path)
    print(f"wrote {path} ({size / 1024:.0f} KiB)")
    assert size < 1 << 20, "over the size limit of a committed file"


if __name__ == "__main__":
    main()
