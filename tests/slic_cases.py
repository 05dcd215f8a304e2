"""Inputs, the case table and a switchable restatement of the integer SLIC (csrc/slic.hip, oracle/slic.py) shared by
tests/test_slic_host.py (CPU) and tests/test_gpu_slic.py (GPU).  Helper only: no tests here.

Every input is built from a name and a seed.  ``slic_switchable`` restates oracle/slic.py with one switch per rule of the
algorithm; with every switch off it equals ``oracle.slic.slic`` (asserted in the host test), with one switch on it is a MUTANT: a
plausible wrong kernel.  The host test requires a named row of the table to tell each mutant from the oracle, so that the rows the
GPU test compares bit for bit are known to depend on the rule they are there for.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import slic as OSL

Case = namedtuple("Case", "name builder H W num_components compactness iters seed")


# ---- input builders: name, seed -> [3,H,W] (uint8 unless stated) ---------------------------------------------------------
def smooth_float(H, W, seed):
    """The construction of test_slic_shapes_and_repeatability: a bilinearly up-sampled coarse colour field plus 20 % noise, float32 in [0,1]."""
    import torch

    g = torch.Generator().manual_seed(seed)
    base = torch.rand(3, H // 8 + 1, W // 8 + 1, generator=g)
    img = torch.nn.functional.interpolate(base[None], size=(H, W), mode="bilinear")[0] * 0.8 + 0.2 * torch.rand(3, H, W, generator=g)
    return img.numpy().astype(np.float32)


def smooth(H, W, seed):
    return OSL.to_u8(smooth_float(H, W, seed))


def noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (3, H, W), dtype=np.uint8)


def const(H, W, seed):
    colour = np.random.default_rng(seed).integers(0, 256, 3, dtype=np.uint8)
    return np.broadcast_to(colour[:, None, None], (3, H, W)).copy()


def halves(H, W, seed):
    """Two flat colours, left and right.  The pairs are saturated primaries, so that a and b are far from zero and of both signs."""
    pairs = [((0, 255, 0), (0, 0, 255)), ((255, 0, 0), (0, 255, 255)), ((20, 200, 40), (230, 30, 220)), ((0, 120, 255), (250, 240, 10))]
    left, right = pairs[seed % len(pairs)]
    img = np.empty((3, H, W), np.uint8)
    img[:, :, : W // 2] = np.array(left, np.uint8)[:, None, None]
    img[:, :, W // 2:] = np.array(right, np.uint8)[:, None, None]
    return img


def two_level_noise(H, W, seed):
    v = (np.random.default_rng(seed).integers(0, 2, (H, W)) * 255).astype(np.uint8)
    return np.stack([v, v, v])


BLOCK_LEVELS = (40, 128, 215)


def blocks(H, W, seed):
    """8x8 flat blocks, each at one of three grey levels."""
    rng = np.random.default_rng(seed)
    lv = np.array(BLOCK_LEVELS, np.uint8)[rng.integers(0, 3, ((H + 7) // 8, (W + 7) // 8))]
    v = np.kron(lv, np.ones((8, 8), np.uint8))[:H, :W]
    return np.stack([v, v, v])


def faint_noise(H, W, seed):
    """One flat colour plus iid {-1, 0, +1} per channel.  The centres end up a few 1/64 Lab units apart, so the colour term and the
    spatial term of the distance are of the same size at m2q of 1 or 2: the only kind of frame on which the rounding of m2q shows."""
    rng = np.random.default_rng(seed)
    base = rng.integers(30, 226, 3)
    return (base[:, None, None] + rng.integers(-1, 2, (3, H, W))).astype(np.uint8)


def float_wrap(H, W, seed):
    """float32 in [-0.5, 1.5] (np.uint8(img * 255) wraps what is outside [0,1] and truncates toward zero), with the values at which
    truncation and rounding part planted: exact 0.0 and 1.0, k/255 and the float just below it."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-0.5, 1.5, (3, H, W)).astype(np.float32)
    flat = img.reshape(-1)
    n = flat.size
    k = rng.integers(0, 256, n).astype(np.float32) / np.float32(255.0)
    kind = rng.integers(0, 8, n)                         # half of the pixels keep their random value
    flat[kind == 0] = 0.0
    flat[kind == 1] = 1.0
    flat[kind == 2] = k[kind == 2]
    flat[kind == 3] = np.nextafter(k[kind == 3], np.float32(0.0))
    return img


BUILDERS = {"smooth": smooth, "smooth_float": smooth_float, "noise": noise, "const": const, "halves": halves,
            "two_level_noise": two_level_noise, "blocks": blocks, "faint_noise": faint_noise, "float_wrap": float_wrap}
FLOAT_BUILDERS = ("smooth_float", "float_wrap")

# The seed of the `blocks` rows.  Clusters are emptied for most seeds, but whether the centre is then kept or zeroed changes the final
# labels for few: of the seeds 0 .. 48 only 28, 47 and 48 (5.0 %, 2.5 % and 8.8 % of the labels).  tests/test_slic_host.py holds the
# choice: test_every_mutant_is_killed fails if this seed stops telling the two apart.
BLOCKS_SEED = 28


@functools.lru_cache(maxsize=None)
def _image(builder, H, W, seed):
    img = BUILDERS[builder](H, W, seed)
    img.setflags(write=False)
    return img


def image(case: Case) -> np.ndarray:
    """The (read-only, cached) input of a row."""
    return _image(case.builder, case.H, case.W, case.seed)


@functools.lru_cache(maxsize=None)
def _oracle(case: Case):
    out = OSL.slic(image(case), case.num_components, case.compactness, case.iters)
    out.setflags(write=False)
    return out


def oracle_labels(case: Case) -> np.ndarray:
    """oracle.slic.slic on a row: computed once per process, shared by the tests, read-only."""
    return _oracle(case)


def _rows():
    rows = []

    def add(tag, builder, H, W, nc, m=10.0, iters=10, seed=None):
        seed = (H * 1000 + W + nc) % 9973 if seed is None else seed
        rows.append(Case(f"{tag}-{builder}-{H}x{W}-n{nc}-m{m:g}-it{iters}", builder, H, W, nc, float(m), iters, seed))

    for b in ("smooth", "noise"):
        add("tail169", b, 37, 53, 12)            # H*W % 256 = 169, W < 64: no wave holds a whole row
        add("tail255", b, 65, 63, 9)             # % 256 = 255
        add("tail172", b, 50, 70, 30)            # % 256 = 172, K = 35 != components
        add("onerow", b, 8, 200, 10)             # ny = 1
        add("onecol", b, 200, 8, 10)             # nx = 1
        add("flat", b, 3, 300, 5)                # ny = 1, H < cell size
        add("single", b, 61, 67, 1)              # one cluster
        add("pixel", b, 1, 1, 1)                 # smallest frame
        add("lds57600", b, 48, 60, 2880)         # S2 = 1, one cell per pixel, 57 600 B of LDS
        add("lds57600", b, 48, 60, 100000)       # num_components > H*W
        add("lds61440", b, 48, 64, 3072)         # exactly the 60 KB limit
        add("lds52020", b, 256, 256, 2600)       # K = 2601 at a real cell size
        for m in (0.0, 0.02, 1000.0):            # 0.02^2 * 4096 = 1.6384: rounds to 2, truncates to 1
            add("compact", b, 96, 96, 40, m)
        add("e2e", b, 72, 104, 100)              # the frame size of the end-to-end test
        add("wide", b, 130, 200, 4, 1000.0)      # cells 66 pixels wide: whole waves inside one superpixel next to waves across a border
    for b in ("const", "halves", "two_level_noise", "noise"):
        for m in (0.0, 0.5, 10.0):
            add("ties", b, 70, 90, 20, m)
        add("ties", b, 70, 90, 20, 10.0, iters=1)
        add("ties", b, 70, 90, 20, 10.0, iters=2)
    for m in (0.02, 1.0):
        add("empty", "blocks", 64, 80, 20, m, seed=BLOCKS_SEED)
    add("m2q", "faint_noise", 96, 96, 40, 0.02, seed=5)
    add("m2q", "faint_noise", 64, 80, 20, 0.02, seed=3)
    add("wrap", "float_wrap", 37, 53, 12)
    add("wrap", "float_wrap", 70, 90, 20, 0.5)
    add("float", "smooth_float", 65, 63, 9)
    add("float", "smooth_float", 72, 104, 100)
    return tuple(rows)


CASES = _rows()
LDS_ROWS = tuple(c for c in CASES if c.name.startswith("lds"))


def by_name(name: str) -> Case:
    (c,) = [c for c in CASES if c.name == name]
    return c


# ---- the switchable restatement -------------------------------------------------------------------------------------------
SWITCHES = ("ties_highest", "empty_zeroed", "update_truncated", "update_c_division", "m2q_truncated", "u8_round", "u8_saturate",
            "window_short", "extra_update")


def _to_u8(img, u8_round, u8_saturate):
    if img.dtype == np.uint8:
        return img
    v = img.astype(np.float32) * np.float32(255.0)
    v = np.rint(v) if u8_round else np.trunc(v)
    v = v.astype(np.int64)
    if u8_saturate:
        v = np.clip(v, 0, 255)
    return (v & 255).astype(np.uint8)


def _c_div(a, b):
    """C's integer division: toward zero (b > 0)."""
    return np.where(a < 0, -((-a) // b), a // b)


def slic_switchable(img, num_components, compactness, iters=10, *, ties_highest=False, empty_zeroed=False, update_truncated=False,
                    update_c_division=False, m2q_truncated=False, u8_round=False, u8_saturate=False, window_short=None,
                    extra_update=False, stats=None):
    """oracle/slic.py restated with one switch per rule (all off: the oracle).  ``window_short``: None, "row" or "col" (the 3x3
    search stops one row / column of cells short).  ``stats``: a dict that receives counters (empty-cluster events, pixels whose
    two best distances tie, negative centre sums)."""
    u8 = _to_u8(img, u8_round, u8_saturate)
    _, H, W = u8.shape
    lab = OSL.lab64(u8)
    S2 = max(1, (H * W) // num_components)
    gs = 1
    while (gs + 1) * (gs + 1) <= S2:
        gs += 1
    nx, ny = max(1, (W + gs // 2) // gs), max(1, (H + gs // 2) // gs)
    m2f = np.float32(compactness) * np.float32(compactness) * np.float32(4096.0)
    m2q = int(m2f) if m2q_truncated else int(np.rint(m2f))
    K = nx * ny
    ci, cj = np.divmod(np.arange(K), nx)
    cx = ((2 * cj + 1) * W) // (2 * nx)
    cy = ((2 * ci + 1) * H) // (2 * ny)
    cent = np.stack([lab[0, cy, cx], lab[1, cy, cx], lab[2, cy, cx], cx, cy], axis=1).astype(np.int64)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pj = np.minimum(xs * nx // W, nx - 1)
    pi = np.minimum(ys * ny // H, ny - 1)
    ny_end = ny - 1 if window_short == "row" else ny
    nx_end = nx - 1 if window_short == "col" else nx
    n_assign = iters + 1 if extra_update else iters      # one update too many == one iteration more
    counters = {"empty_events": 0, "tied_pixels": 0, "negative_sums": 0}
    labels = None
    for it in range(n_assign):
        best = np.full((H, W), -1, dtype=np.int64)
        bestd = np.full((H, W), np.iinfo(np.int64).max, dtype=np.int64)
        tied = np.zeros((H, W), dtype=bool)
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                i, j = pi + di, pj + dj
                ok = (i >= 0) & (i < ny_end) & (j >= 0) & (j < nx_end)
                k = np.where(ok, i * nx + j, 0)
                c = cent[k]
                d = ((lab[0] - c[..., 0]) ** 2 + (lab[1] - c[..., 1]) ** 2 + (lab[2] - c[..., 2]) ** 2) * S2 \
                    + m2q * ((xs - c[..., 3]) ** 2 + (ys - c[..., 4]) ** 2)
                tied = np.where(ok & (d < bestd), False, tied) | (ok & (d == bestd) & (best >= 0))   # the best distance is shared
                take = ok & ((d <= bestd) if ties_highest else (d < bestd))
                bestd = np.where(take, d, bestd)
                best = np.where(take, k, best)
        labels = best
        counters["tied_pixels"] += int(tied.sum())
        if it == n_assign - 1:
            break
        flat = labels.ravel()
        live = flat >= 0
        n = np.bincount(flat[live], minlength=K)
        counters["empty_events"] += int((n == 0).sum())
        for c, v in enumerate((lab[0], lab[1], lab[2], xs, ys)):
            s = np.zeros(K, dtype=np.int64)
            np.add.at(s, flat[live], v.ravel()[live])
            counters["negative_sums"] += int((s < 0).sum())
            n1 = np.maximum(n, 1)
            if update_truncated:
                upd = s // n1
            elif update_c_division:
                upd = _c_div(2 * s + n, 2 * n1)
            else:
                upd = (2 * s + n) // (2 * n1)                # round half up, floor division
            cent[:, c] = np.where(n > 0, upd, 0 if empty_zeroed else cent[:, c])
    if stats is not None:
        stats.update(counters)
    return labels.astype(np.int32)


# ---- CIELAB in float64, the yardstick of the integer Lab ---------------------------------------------------------------------
def cielab_float64(u8: np.ndarray) -> np.ndarray:
    """[3,...] uint8 sRGB -> float64 (L, a, b): the sRGB D65 matrix, X and Z over the white point (0.95047, 1.08883), f with its
    threshold at 0.008856 and the linear branch 7.787 t + 16/116."""
    c = u8.astype(np.float64) / 255.0
    lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    R, G, B = lin[0], lin[1], lin[2]
    X = (0.412453 * R + 0.357580 * G + 0.180423 * B) / 0.95047
    Y = 0.212671 * R + 0.715160 * G + 0.072169 * B
    Z = (0.019334 * R + 0.119193 * G + 0.950227 * B) / 1.08883

    def f(t):
        return np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0)

    fx, fy, fz = f(X), f(Y), f(Z)
    return np.stack([116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)])


def all_colours_slab(r0: int, r1: int) -> np.ndarray:
    """[3, (r1 - r0) * 65536] uint8: every colour with R in [r0, r1), pixel index = (R - r0) * 65536 + G * 256 + B."""
    r, g, b = np.meshgrid(np.arange(r0, r1, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return np.stack([r.ravel(), g.ravel(), b.ravel()])
