"""The permutohedral dense CRF (csrc/dense_crf_permutohedral.hip) on the paths its first tests do not reach: more than 256 sort tiles
(second and third rounds of the digit and tile scans), 4, 5 and 7 radix passes of the bilateral lattice (either ping-pong half),
lattice points with thousands of contributors or with none above 3 (the chunked splat on both lattices), frames below one chunk or
one tile, the second CRF of a shared pass, relabel_last, and the 64-column debug rows.

Every comparison is against the statements of tests/test_dense_crf_permutohedral.py (``lattice32`` bit for bit, ``crf_lattice64`` in
float64 on that lattice) with that file's tolerances: normalisers and one-iteration messages <= 1e-5 relative to the message of unit
values, Q after ten iterations <= 1e-4 with equal labels where the float64 top-2 margin is >= 1e-4.  The frames are the named cases
of tests/dense_crf_cases.py; tests/test_dense_crf_cases_host.py asserts that each one reaches the path it is used for.  Each test
prints its figures before it asserts (DESIGN.md "Permutohedral dense CRF" quotes them)."""
import numpy as np
import pytest
import torch

from tests.dense_crf_cases import CASES, TINY
from tests.test_dense_crf import g
from tests.test_dense_crf_permutohedral import crf_lattice64, features32, filter64, lattice32

PERM = dict(method="permutohedral")


def _lattice_identity(dev, name, frames=1, which=(False, True)):
    from wild_visual_navigation_amd import ops

    c = CASES[name]
    images = torch.stack([c.image(b) for b in range(frames)])
    for bilateral in which:
        xy, rgb = (c.bi_xy, c.bi_rgb) if bilateral else (c.pos_xy, None)
        got_all = ops._permutohedral_lattice(images.to(dev), bilateral, xy, rgb if rgb else 1.0)
        for b in range(frames):
            got, want = got_all[b], lattice32(features32(c.H, c.W, images[b].numpy(), xy, rgb))
            assert got["M"] == want["M"], (name, bilateral, b, got["M"], want["M"])
            assert np.array_equal(got["keys"].numpy(), want["keys"]), (name, bilateral, b)
            assert np.array_equal(got["vert"].numpy(), want["vert"]), (name, bilateral, b)
            assert np.array_equal(got["bary"].numpy().view(np.int32), want["bary"].view(np.int32)), (name, bilateral, b)
            assert np.array_equal(got["nbr"].numpy(), want["nbr"]), (name, bilateral, b)


def _one_iteration(dev, name, K, seed):
    """Normalisers and first-iteration messages of frame 0 of the case, read from the debug rows: message rows c and KP + c, the
    normalisers at 2 KP and 2 KP + 1; the rows of the padding columns stay as the caller zeroed them."""
    from wild_visual_navigation_amd import ops

    c = CASES[name]
    H, W, KP = c.H, c.W, 32 if K <= 32 else 64
    image = c.image(0)
    logits = torch.randn(1, K, H, W, generator=g(seed)) * 2
    _, _, dbg = ops.dense_crf(logits.to(dev), image[None].to(dev), iterations=1, return_probs=True, _debug=True, **PERM, **c.stds)
    assert dbg.shape[1] == 2 * KP + 2
    dbg = dbg[0].reshape(2 * KP + 2, H * W).double()
    _, first = crf_lattice64(logits[0].double().to(dev), image.to(dev), 1, parts=True, **c.stds)
    errs = {}
    for what, row, n in (("n_b", 2 * KP, first["n_b"]), ("n_g", 2 * KP + 1, first["n_g"])):
        errs[what] = ((dbg[row] - n).abs() / n).max().item()
    for what, rows, lat, n, msg in (("msg_b", slice(0, K), first["lb"], first["n_b"], first["msg_b"]),
                                    ("msg_g", slice(KP, KP + K), first["lg"], first["n_g"], first["msg_g"])):
        scale = n * filter64(lat, n[:, None])[:, 0]          # the message of unit values
        errs[what] = ((dbg[rows].T - msg).abs() / scale[:, None]).max().item()
    print(f"one iteration {name} K={K}: " + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    for what, err in errs.items():
        assert err <= 1e-5, (name, what, err)
    assert not dbg[K:KP].any() and not dbg[KP + K:2 * KP].any()


def _ten_iterations(dev, name, K, seed, **weights):
    from wild_visual_navigation_amd import ops

    c = CASES[name]
    image = c.image(0)
    logits = torch.randn(1, K, c.H, c.W, generator=g(seed)) * 1.5
    lab, Q = ops.dense_crf(logits.to(dev), image[None].to(dev), return_probs=True, **PERM, **c.stds, **weights)
    Q64 = crf_lattice64(logits[0].double().to(dev), image.to(dev), **c.stds, **weights)
    err = (Q[0].double() - Q64).abs().max().item()
    print(f"ten iterations {name} K={K}: max|Q - Q64| = {err:.3e}")
    assert err <= 1e-4, (name, err)
    top2 = Q64.topk(2, 0).values
    bad = (lab[0].long() != Q64.argmax(0)) & (top2[0] - top2[1] >= 1e-4)
    assert not bad.any(), (name, int(bad.sum()))


# ---------------------------------------------------------------- A: more than 256 sort tiles ----------------------------------------
@pytest.mark.gpu
def test_bilateral_lattice_with_257_sort_tiles_is_bit_identical(dev):
    _lattice_identity(dev, "tiles_bilateral", frames=2, which=(True,))


@pytest.mark.gpu
def test_gaussian_lattice_with_259_sort_tiles_is_bit_identical(dev):
    _lattice_identity(dev, "tiles_gaussian", which=(False,))


@pytest.mark.gpu
def test_bilateral_lattice_with_517_sort_tiles_is_bit_identical(dev):
    """The same frame's bilateral lattice: a third round of the scans."""
    _lattice_identity(dev, "tiles_gaussian", which=(True,))


@pytest.mark.gpu
def test_one_iteration_with_257_sort_tiles(dev):
    _one_iteration(dev, "tiles_bilateral", 5, 283)


# ---------------------------------------------------------------- B: pass counts -----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["passes_5", "passes_7", "passes_4"])
def test_pass_counts_lattice_is_bit_identical(dev, name):
    _lattice_identity(dev, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["passes_5", "passes_7", "passes_4"])
def test_pass_counts_one_iteration(dev, name):
    _one_iteration(dev, name, 5, 40)


@pytest.mark.gpu
def test_pydensecrf_defaults_ten_iterations_with_other_weights(dev):
    _ten_iterations(dev, "passes_5", 27, 27, pos_w=2.0, bi_w=6.0)


# ---------------------------------------------------------------- C: contributor extremes --------------------------------------------
C_CASES = ["constant", "flat_blocks", "random", "wide_gaussian", "checker", "checker_narrow"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", C_CASES)
def test_contributor_extremes_lattice_is_bit_identical(dev, name):
    _lattice_identity(dev, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", C_CASES)
def test_contributor_extremes_one_iteration(dev, name):
    _one_iteration(dev, name, 5, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["constant", "checker", "checker_narrow"])
def test_contributor_extremes_ten_iterations(dev, name):
    _ten_iterations(dev, name, 6, 6)


@pytest.mark.gpu
def test_long_contributor_lists_are_deterministic_and_batch_independent(dev):
    """The chunk partial sums of a batch: frames with 63 and up to 31 chunks on a point, together and alone."""
    from wild_visual_navigation_amd import ops

    images = torch.stack([CASES["constant"].image(0), CASES["flat_blocks"].image(0), CASES["constant"].image(1)]).to(dev)
    logits = (torch.randn(3, 6, 64, 64, generator=g(9)) * 2).to(dev)
    lab, Q = ops.dense_crf(logits, images, return_probs=True, **PERM)
    lab_again, Q_again = ops.dense_crf(logits, images, return_probs=True, **PERM)
    assert torch.equal(lab, lab_again) and torch.equal(Q, Q_again)
    for b in range(3):
        lab1, Q1 = ops.dense_crf(logits[b:b + 1], images[b:b + 1], return_probs=True, **PERM)
        assert torch.equal(lab[b:b + 1], lab1) and torch.equal(Q[b:b + 1], Q1)


# ---------------------------------------------------------------- D: tiny frames -----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", TINY)
def test_tiny_frames_lattice_is_bit_identical(dev, name):
    _lattice_identity(dev, name)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 40])
@pytest.mark.parametrize("name", TINY)
def test_tiny_frames_ten_iterations(dev, name, K):
    _ten_iterations(dev, name, K, K)


# ---------------------------------------------------------------- E: the shared pass -------------------------------------------------
def _shared_images(dev, B=3):
    return torch.stack([CASES["shared"].image(b) for b in range(B)]).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("K1,K2", [(7, 20), (27, 27), (7, 30), (32, 32)])
def test_shared_pass_second_group(dev, K1, K2):
    """Group 2 (columns K1.., labels less K1) against float64 on its own logits and against its CRF alone (<= 1e-6, the exact CRF's
    bound for a second group); group 1 bit-identical to its CRF alone.  27 + 27 puts the group boundary inside a wave's 64 lanes."""
    from wild_visual_navigation_amd import ops

    c = CASES["shared"]
    images = _shared_images(dev)
    B = images.shape[0]
    la = (torch.randn(B, K1, c.H, c.W, generator=g(K1)) * 2).to(dev)
    lb = (torch.randn(B, K2, c.H, c.W, generator=g(100 + K2)) * 2).to(dev)
    lab2, Q2 = ops.dense_crf((la, lb), images, return_probs=True, **PERM)
    lab_a, Q_a = ops.dense_crf(la, images, return_probs=True, **PERM)
    lab_b, Q_b = ops.dense_crf(lb, images, return_probs=True, **PERM)
    assert lab2.shape == (B, 2, c.H, c.W) and Q2.shape == (B, K1 + K2, c.H, c.W)
    assert torch.equal(lab2[:, 0], lab_a) and torch.equal(Q2[:, :K1], Q_a)
    alone = (Q2[:, K1:] - Q_b).abs().max().item()
    worst = 0.0
    for b in range(B):
        Q64 = crf_lattice64(lb[b].double(), images[b])
        worst = max(worst, (Q2[b, K1:].double() - Q64).abs().max().item())
        top2 = Q64.topk(2, 0).values
        bad = (lab2[b, 1].long() != Q64.argmax(0)) & (top2[0] - top2[1] >= 1e-4)
        assert not bad.any(), (b, int(bad.sum()))
    print(f"shared pass {K1} + {K2}: group 2 max|Q - Q64| = {worst:.3e}, from its CRF alone {alone:.3e}")
    assert worst <= 1e-4, worst
    assert alone <= 1e-6, alone
    assert int(lab2[:, 1].min()) >= 0 and int(lab2[:, 1].max()) < K2


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [False, True])
def test_relabel_last_compacts_the_last_group_only(dev, pair):
    from wild_visual_navigation_amd import ops

    c = CASES["shared"]
    images = _shared_images(dev)
    B, K1, K2 = images.shape[0], 7, 30
    la = (torch.randn(B, K1, c.H, c.W, generator=g(1)) * 2).to(dev)
    lb = torch.randn(B, K2, c.H, c.W, generator=g(2)) * 2
    lb[:, ::3] -= 12.0                                             # labels that never win: the compaction has gaps to close
    lb = lb.to(dev)
    logits = (la, lb) if pair else lb
    lab, Q = ops.dense_crf(logits, images, return_probs=True, **PERM)
    lab_r, nseg, Q_r = ops.dense_crf(logits, images, return_probs=True, relabel_last=True, **PERM)
    assert torch.equal(Q, Q_r) and nseg.shape == (B,) and nseg.dtype == torch.int32
    if pair:
        assert torch.equal(lab_r[:, 0], lab[:, 0])
    last, last_r = (lab[:, 1], lab_r[:, 1]) if pair else (lab, lab_r)
    for b in range(B):
        ids, inverse = torch.unique(last[b], return_inverse=True)
        assert 1 < ids.numel() < K2 and int(ids.max()) >= ids.numel()      # the relabelling is not the identity
        assert torch.equal(last_r[b].long(), inverse)
        assert int(nseg[b]) == ids.numel()


# ---------------------------------------------------------------- F: the 64-column debug rows ----------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blocky64", "constant"])
def test_one_iteration_debug_rows_of_the_64_column_layout(dev, name):
    _one_iteration(dev, name, 40, 40)
