"""The cases of the LinearRnvp training tests, shared by tests/test_gpu_linear_rnvp_train.py and scripts/pin_linear_rnvp_train.py
(which records the reference's own gradient error for exactly these states, rows and row counts)."""
import linear_rnvp_ref as REF

TILE = 32                                                    # wvn_rnvp_row_tile(); the GPU test asserts it
ROW_COUNTS = (1, 33, TILE - 1, TILE + 1, 2 * TILE + 5)
GRAD_CASES = [(90, "odds", 200), (90, "half", 200), (384, "odds", 200), (384, "half", 200),
              (90, "odds", 48), (384, "odds", 225), (90, "odds", 256)]
TRAJ_STEPS = 12


def case_key(D, mask_type, h):
    return f"D{D}_{mask_type}_h{h}"


def case_sd(D, mask_type, h):
    """Seeded weights, s and t different (as after training)."""
    return REF.seeded_sd(D, h, seed=1000 + D + h + (7 if mask_type == "half" else 0), mask_type=mask_type)


def case_rows(mlp_train, D):
    return mlp_train["graph_pt_D90"]["x"] if D == 90 else mlp_train["synthetic_D384"]["x"]


def traj_sd():
    return REF.seeded_sd(384, 200, seed=395)


def traj_rows(mlp_train):
    return mlp_train["synthetic_D384"]["x"][:100]
