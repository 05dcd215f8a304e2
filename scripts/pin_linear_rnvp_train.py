"""Pin the anomaly-detection TRAINING step against the reference's OWN LinearRnvp + AnomalyLoss + autograd and write
tests/golden/linear_rnvp_train.pt (scalars only, a few KB).

Run in the build container only (needs the reference checkout that oracle.pin_reference.import_reference() loads; nothing under
oracle/ is changed):

    python scripts/pin_linear_rnvp_train.py

Contents:
  grad[case][R]    case = tests/linear_rnvp_train_cases.py: case_key(D, mask, h), R one of ROW_COUNTS: {"own_err": [24], "gmax": [24]}
                   per parameter tensor in model.parameters() order (tests/linear_rnvp_ref.py: PARAM_KEYS): the reference's fp32
                   autograd gradient of AnomalyLoss on the first R rows against the float64 statement (max abs), and max |g64|
  traj             [12, 3] = {loss, generator mean, generator std} of the reference's LinearRnvp(384, [200]) + AnomalyLoss
                   (latest_measurement) + Adam(lr 1e-3) from traj_sd() on traj_rows(), every step on all 100 rows
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import linear_rnvp_ref as REF  # noqa: E402
import linear_rnvp_train_cases as CASES  # noqa: E402
from oracle.pin_reference import import_reference  # noqa: E402


def new_model(D, h, mask_type, sd):
    from wild_visual_navigation.model import LinearRnvp

    model = LinearRnvp(input_size=D, coupling_topology=[h], mask_type=mask_type, conditioning_size=0, use_permutation=True,
                       single_function=False)
    model.load_state_dict(sd)
    assert [k for k, _ in model.named_parameters()] == REF.PARAM_KEYS, "parameter order of the reference changed"
    return model.train()


def loss_of(model, loss_fn, x, step=0):
    from wild_visual_navigation.utils.data import Data

    batch = Data(x=x.clone())
    return loss_fn(batch, model(batch), step=step, log_step=False)[0]


def grad_case(D, mask_type, h, x):
    from wild_visual_navigation.utils.loss import AnomalyLoss

    sd = CASES.case_sd(D, mask_type, h)
    model = new_model(D, h, mask_type, sd)
    out = {}
    for R in sorted(set(CASES.ROW_COUNTS)):
        loss_fn = AnomalyLoss(confidence_std_factor=0.5, method="running_mean", log_enabled=False, log_folder="/tmp")
        g32 = torch.autograd.grad(loss_of(model, loss_fn, x[:R]), list(model.parameters()))
        sd64 = {k: (v.double().clone().requires_grad_(k in REF.PARAM_KEYS) if v.is_floating_point() else v) for k, v in sd.items()}
        g64 = torch.autograd.grad(-REF.flow(sd64, x[:R])[2].mean(), [sd64[k] for k in REF.PARAM_KEYS])
        own = [(a.double() - b).abs().max().item() for a, b in zip(g32, g64)]
        gmax = [b.abs().max().item() for b in g64]
        assert all(m > 0 for m in gmax), "a tensor's gradient is all zero"
        assert all(e < 1e-5 * m for e, m in zip(own, gmax)), "the float64 statement disagrees with the reference's gradient"
        out[R] = {"own_err": own, "gmax": gmax}
        print(f"  {CASES.case_key(D, mask_type, h)} R {R}: own_err / max|g| in [{min(e / m for e, m in zip(own, gmax)):.2e}, "
              f"{max(e / m for e, m in zip(own, gmax)):.2e}]")
    return out


def trajectory(x):
    from wild_visual_navigation.utils.loss import AnomalyLoss

    model = new_model(384, 200, "odds", CASES.traj_sd())
    loss_fn = AnomalyLoss(confidence_std_factor=0.5, method="latest_measurement", log_enabled=False, log_folder="/tmp")
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    cg = loss_fn._confidence_generator
    ref = REF.F64Step(CASES.traj_sd(), "latest_measurement")
    traj = []
    for step in range(CASES.TRAJ_STEPS):
        loss = loss_of(model, loss_fn, x, step)
        opt.zero_grad()
        loss.backward()
        opt.step()
        traj.append([loss.item(), cg.mean.item(), cg.std.item()])
        want, _ = ref.step(x)   # the float64 statement follows the reference's trajectory
        assert abs(want - traj[-1][0]) < 3e-4 * abs(want) and abs(ref.mean - traj[-1][1]) < 3e-4 * abs(ref.mean), (step, want, traj[-1])
        print(f"  step {step}: loss {traj[-1][0]:.4f} mean {traj[-1][1]:.4f} std {traj[-1][2]:.4f}")
    return torch.tensor(traj, dtype=torch.float64)


def main():
    import_reference()
    src = torch.load(os.path.join(ROOT, "tests", "golden", "mlp_train.pt"), weights_only=False)
    out = {"grad": {}, "param_keys": list(REF.PARAM_KEYS)}
    for D, mask_type, h in CASES.GRAD_CASES:
        out["grad"][CASES.case_key(D, mask_type, h)] = grad_case(D, mask_type, h, CASES.case_rows(src, D))
    out["traj"] = trajectory(CASES.traj_rows(src))
    path = os.path.join(ROOT, "tests", "golden", "linear_rnvp_train.pt")
    torch.save(out, path)
    size = os.path.getsize(path)
    print(f"wrote {path} ({size / 1024:.0f} KiB)")
    assert size < 64 << 10, "scalars only"


if __name__ == "__main__":
    main()
