"""CPU checks of the oracle pieces added with the pixel-resolution STEGO reading: the exact fp32 FMA emulation, the fixed-order
bilinear up-sampling (against ATen's), the three-level centroid summation order, and the supervision oracle's NaN semantics."""
import fractions

import numpy as np
import torch

from oracle import interfaces as OI, supervision as OSV


def _fma_exact(a, b, c):
    v = fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c))
    x = np.float32(float(v))
    cands = [x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))]
    return np.float32(min(cands, key=lambda t: (abs(fractions.Fraction(float(t)) - v), int(np.float32(t).view(np.uint32)) & 1)))


def test_fma32_is_correctly_rounded():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(1500).astype(np.float32), rng.standard_normal(1500).astype(np.float32)
    c = (rng.standard_normal(1500) * rng.choice([1e-6, 1.0, 1e3], 1500)).astype(np.float32)
    got = OI._fma32(a, b, c)
    assert all(_fma_exact(a[i], b[i], c[i]) == got[i] for i in range(1500))
    # products that land exactly on rounding midpoints (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24, shifted by multiples of 2^-25
    a2 = np.full(8, 1 + 2.0 ** -12, np.float32)
    c2 = np.array([0, 2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -23, 2.0 ** -25, -2.0 ** -25, 5 * 2.0 ** -25], np.float32)
    g2 = OI._fma32(a2, a2, c2)
    assert all(_fma_exact(a2[i], a2[i], c2[i]) == g2[i] for i in range(8))


def test_fixed_order_upsampling_is_atens_up_to_rounding():
    code = torch.randn(9, 9, 12, generator=torch.Generator().manual_seed(0)) * 3
    got = torch.from_numpy(OI.upsample_bilinear_fixed(code.numpy(), 70))                                  # [70, 70, 12]
    aten = torch.nn.functional.interpolate(code.permute(2, 0, 1)[None], (70, 70), mode="bilinear", align_corners=True)[0].permute(1, 2, 0)
    assert (got - aten).abs().max().item() < 2e-6
    assert torch.equal(got[0, 0], code[0, 0]) and torch.equal(got[-1, -1], code[-1, -1])                   # corners are exact


def test_kmeans_group_fold_degenerates_for_short_inputs():
    """Up to kmeans_super(P) chunks (512 points) the three-level order IS the flat chunk order (0 + x = x exactly)."""
    code = np.random.default_rng(1).standard_normal((500, 16)).astype(np.float32)
    lab = OI.kmeans_cosine_labels_numpy(code, 4, iters=3)
    keep = OI.KMEANS_SUPER
    try:
        OI.KMEANS_SUPER = 10 ** 6          # one group = the flat order
        assert np.array_equal(OI.kmeans_cosine_labels_numpy(code, 4, iters=3), lab)
    finally:
        OI.KMEANS_SUPER = keep
    lab_pix = OI.kmeans_cosine_labels_pixels(code[:49], 7, 20, 3, iters=2)
    assert lab_pix.shape == (400,) and lab_pix.min() >= 0 and lab_pix.max() < 3


def test_c_restatement_of_the_kmeans_equals_the_numpy_statement():
    """oracle/kmeans_ref.c (fmaf chains, built by oracle.build_oracle) against the numpy definition (exact fp32 fma emulation):
    ragged sizes, more than one group of chunks, near-parallel rows (many close similarities), an empty cluster."""
    from oracle import build_oracle

    build_oracle.build()
    assert OI._oracle_lib() is not None
    rng = np.random.default_rng(5)
    # (9300 points: above 8192 the chunk partials fold in groups of 16 chunks instead of 8 -- kmeans_super)
    for P, C, K, it in ((700, 16, 5, 4), (1500, 90, 20, 3), (64, 90, 3, 10), (1100, 33, 7, 2), (9300, 16, 6, 2)):
        code = (rng.standard_normal((P, C)) + 3.0 * rng.standard_normal(C)).astype(np.float32)      # a strong common component
        a = OI.kmeans_cosine_labels(code, K, it)
        b = OI.kmeans_cosine_labels_numpy(code, K, it)
        assert a.dtype == np.int32 and np.array_equal(a, b), (P, C, K)
    code = np.tile(rng.standard_normal((1, 16)).astype(np.float32), (200, 1))                       # identical rows: clusters 1.. stay empty
    assert np.array_equal(OI.kmeans_cosine_labels(code, 4, 3), OI.kmeans_cosine_labels_numpy(code, 4, 3))


def test_supervision_oracle_nan_scan_lines_and_raw_projection():
    H, W = 40, 50
    poly = np.array([[10.0, 5.0], [30.0, 5.0], [20.0, np.inf], [10.0, 30.0]], dtype=np.float32)           # one vertex at y = inf
    left, right = OSV.convex_edges(poly, H, W)
    # the edge (20, inf) -> (10, 30) is active on every row >= 30 and evaluates to (y - inf) * 0 + 20 = NaN there
    assert np.isnan(left[30:]).all() and np.isnan(right[30:]).all()
    assert not OSV.fill_mask(poly, H, W)[30:].any()                             # torch's min / max propagate the NaN: never filled
    assert OSV.fill_mask(poly, H, W)[6:29].any() and np.isfinite(left[6:29]).all()
    K, T = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = 100.0
    pts = np.array([[0.1, 0.2, 2.0], [0.1, 0.2, -2.0]], dtype=np.float32)
    uv, z = OSV.project_points_raw(K, T, pts)
    assert np.isfinite(uv).all() and z.tolist() == [2.0, -2.0]                  # ImageProjector.project: finite behind the camera too
    assert np.isnan(OSV.project_points(K, T, pts)[1]).all() and np.isfinite(OSV.project_points(K, T, pts)[0]).all()


def test_stego_inference_defaults_are_the_upstream_reading_and_flip_equivariant():
    """oracle.interfaces.stego_inference: the defaults are flip-averaged code + k-means over the code pixels; the flip-averaged
    code of a mirrored frame is the mirrored code of the frame, bit for bit (a + b = b + a); the cheap options are explicit."""
    from oracle import vit as OV

    S, P = 32, 8
    sd = OV.make_vit_state_dict("vit_small", P, pretrain_grid=28, seed=2, depth=1)
    head = OI.make_stego_head_state_dict(384, 90, seed=1)
    img = torch.rand(1, 3, S, S, generator=torch.Generator().manual_seed(4))
    code, seg = OI.stego_inference(sd, head, img, S, P, 6, 4)
    assert code.shape == (1, 90, S, S) and seg.shape == (1, 1, S, S) and seg.dtype == torch.int32
    code_m, _ = OI.stego_inference(sd, head, img.flip(-1), S, P, 6, 4)
    assert torch.allclose(code_m, code.flip(-1), atol=2e-6)        # (the up-sampling weights w / 1 - w swap roles: not bit for bit)
    G = S // P
    x = OI.dino_transform(img, S)
    t, tm = OV.vit_tokens(sd, x, P, 6)[:, 1:], OV.vit_tokens(sd, x.flip(-1), P, 6)[:, 1:]
    c, cm = OI.stego_code_flip_average(head, t, tm, G), OI.stego_code_flip_average(head, tm, t, G)
    assert torch.equal(cm.reshape(1, G, G, 90), c.reshape(1, G, G, 90).flip(2))   # at patch resolution: bit for bit
    code_1, seg_1 = OI.stego_inference(sd, head, img, S, P, 6, 4, flip_tta=False, cluster_resolution="patch")
    assert not torch.equal(code_1, code)
    assert torch.equal(seg_1[0, 0], seg_1[0, 0].reshape(G, P, G, P)[:, :1, :, :1].expand(G, P, G, P).reshape(S, S))   # patch-aligned labels
    tok = OV.vit_tokens(sd, OI.dino_transform(img, S), P, 6)[:, 1:]
    assert torch.equal(OI.upsample_bilinear_ac(OI.stego_code_tokens(head, tok).reshape(1, G, G, 90).permute(0, 3, 1, 2), S), code_1)


def test_linear_form_c_restatement_equals_its_numpy_statement():
    """oracle/kmeans_linear_ref.c against oracle/kmeans_linear.py (exact fp32 fma emulation): labels AND centroids bit for bit, incl.
    fewer pixels than patches per side (bands without rows), many rows per band, K = 27, an empty cluster."""
    from oracle import build_oracle, kmeans_linear as KL

    build_oracle.build()
    rng = np.random.default_rng(7)
    for G, H, C, K in [(8, 64, 90, 5), (7, 50, 16, 4), (5, 33, 90, 6), (12, 9, 16, 3), (6, 100, 16, 27), (9, 70, 90, 17)]:
        code = (rng.standard_normal((G * G, C)) * (1 + rng.random((G * G, 1)))).astype(np.float32)
        if K == 6:
            code[:] = code[:1] + 1e-3 * code            # near-parallel rows: several clusters end up empty and keep their centroid
        lab_c, cent_c = KL.kmeans_pixels_linear(code, G, H, K, iters=4)
        lab_n, cent_n = KL.kmeans_pixels_linear(code, G, H, K, iters=4, force_numpy=True)
        assert KL.kmeans_pixels_linear_c(code, G, H, K, iters=4) is not None
        assert np.array_equal(lab_c, lab_n) and np.array_equal(cent_c, cent_n), (G, H, C, K)


def test_degenerate_kmeans_fixtures_are_degenerate_and_both_statements_agree_on_them(capsys):
    """tests/kmeans_edge_cases.py: piecewise-constant integer codes -- exact ties, clusters that end up empty, zero rows.  On every fixture
    tests/test_gpu_kmeans_edges.py runs: the numpy statement equals its C restatement (the direct oracle on the direct form's fixtures, the
    linear one -- labels AND centroids -- on the linear form's; the numpy side only up to P K C = 4e7), and the input IS degenerate: these
    are conditions on the fixture, not measurements -- a fixture that misses one is to be changed, not the condition."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import kmeans_edge_cases as KE
    from oracle import build_oracle, kmeans_linear as KL

    build_oracle.build(force=False)
    assert OI._oracle_lib() is not None
    for G, H, C, K, nv in sorted(set(KE.DIRECT_FIXTURES + KE.LINEAR_FIXTURES)):
        code = KE.degenerate_code(G, C, nv, seed=0)
        assert code.shape == (G * G, C) and not code[0].any() and np.array_equal(code, np.round(code)) and np.abs(code).max() <= 3
        assert len(np.unique(code, axis=0)) == nv < K
        d = KE.describe(code, G, H, K)
        with capsys.disabled():
            print(f"\n  degenerate fixture G={G} H={H} C={C} K={K}: {d['duplicate_centroids']} duplicate initial centroids, {d['zero_rows']} zero rows, "
                  f"first-pass tie share {d['tie_share']:.3f}, {d['used_clusters']} of {K} clusters used", end="")
        assert d["duplicate_centroids"] >= 1 and d["zero_rows"] >= 100 and d["used_clusters"] < K, (G, H, C, K, d)
        if K == 20:      # the case all five assign forms of the direct kernel run
            assert d["tie_share"] >= 0.5, d
        if H * H * K * C > 4e7:
            continue
        if (G, H, C, K, nv) in KE.DIRECT_FIXTURES:
            dense = OI.upsample_bilinear_fixed(code.reshape(G, G, C), H).reshape(H * H, C)
            assert np.array_equal(OI.kmeans_cosine_labels(dense, K), OI.kmeans_cosine_labels_numpy(dense, K)), (G, H, C, K)
        if (G, H, C, K, nv) in KE.LINEAR_FIXTURES:
            lab_c, cent_c = KL.kmeans_pixels_linear(code, G, H, K)
            lab_n, cent_n = KL.kmeans_pixels_linear(code, G, H, K, force_numpy=True)
            assert np.array_equal(lab_c, lab_n) and np.array_equal(cent_c, cent_n), (G, H, C, K)


def test_linear_and_direct_statements_of_the_pixel_kmeans_agree_within_float_tolerance():
    """The two definitions are the same function in exact arithmetic.  In fp32 every pixel where their maps differ must lie within
    the float tolerance of a decision boundary of the direct statement: its margin there <= 2 (eps_x + eps_c) with eps_x = 0 (the
    points are identical) and eps_c the distance between the two runs' final centroids -- oracle/segmap_agreement.py's criterion."""
    from oracle import build_oracle, kmeans_linear as KL, segmap_agreement as SA

    build_oracle.build()
    gen = torch.Generator().manual_seed(3)
    for G, H, C, K, smooth in [(28, 224, 90, 20, True), (28, 224, 90, 20, False), (9, 70, 16, 7, False)]:
        if smooth:      # code with cluster structure, as a real segmentation's
            code = torch.nn.functional.interpolate(torch.randn(1, C, 7, 7, generator=gen), (G, G), mode="bicubic")[0].permute(1, 2, 0).reshape(G * G, C) * 2 + 0.3
        else:
            code = torch.randn(G * G, C, generator=gen)
        code = code.numpy().astype(np.float32)
        ld, cd, x = SA.kmeans_pixels_full(code, G, H, K, form="direct")
        ll, cl, x2 = SA.kmeans_pixels_full(code, G, H, K, form="linear")
        assert np.array_equal(x, x2)                                       # the same points, bit for bit
        eps_c = float(np.sqrt(((cd.astype(np.float64) - cl) ** 2).sum(1)).max())
        mism = np.nonzero(ld != ll)[0]
        assert mism.size <= 0.002 * ld.size, (G, H, K, mism.size)
        if mism.size:
            sims = x[mism].astype(np.float64) @ cd.astype(np.float64).T
            margin = sims[np.arange(mism.size), ld[mism]] - sims[np.arange(mism.size), ll[mism]]
            assert margin.max() <= 2 * eps_c + 2e-6, (margin.max(), eps_c)


def test_linear_and_direct_statements_at_the_headline_shape_pinned_numbers():
    """VERDICT r5 item 5a.  oracle/kmeans_linear.py is CO-DEFINED with csrc/stego_linear.hip (its summation tiling -- ROW_GROUP, the band chains --
    follows the kernel's; round 5 changed both in one commit), so "bit-exact against the oracle" alone would let the pair drift together.  The
    independent anchor is the DIRECT statement (oracle/interfaces.py::kmeans_cosine_labels_pixels: every pixel's row re-created and multiplied out, no
    tiling of its own to tune).  This test pins their agreement at the headline shape -- G = 56, H = 448, C = 90, K = 20, structured code -- as NUMBERS:
    an edit of the linear definition that changes what it computes moves them."""
    from oracle import build_oracle, segmap_agreement as SA

    build_oracle.build()
    G, H, C, K = 56, 448, 90, 20
    gen = torch.Generator().manual_seed(11)
    code = torch.nn.functional.interpolate(torch.randn(1, C, 9, 9, generator=gen), (G, G), mode="bicubic")[0].permute(1, 2, 0).reshape(G * G, C) * 2 + 0.3
    code = (code + 0.05 * torch.randn(G * G, C, generator=gen)).numpy().astype(np.float32)
    ld, cd, x = SA.kmeans_pixels_full(code, G, H, K, form="direct")
    ll, cl, x2 = SA.kmeans_pixels_full(code, G, H, K, form="linear")
    assert np.array_equal(x, x2)
    eps_c = float(np.sqrt(((cd.astype(np.float64) - cl) ** 2).sum(1)).max())
    mism = np.nonzero(ld != ll)[0]
    worst = 0.0
    if mism.size:
        sims = x[mism].astype(np.float64) @ cd.astype(np.float64).T
        margin = sims[np.arange(mism.size), ld[mism]] - sims[np.arange(mism.size), ll[mism]]
        worst = float(margin.max())
    print(f"direct vs linear at 448^2, K = 20: {mism.size} of {ld.size} pixels differ ({mism.size / ld.size:.2e}), centroid distance {eps_c:.2e}, "
          f"max margin of a differing pixel {worst:.2e} = {worst / max(eps_c, 1e-30):.2f} eps_c")
    assert eps_c < 2e-6                                # the two statements' final centroids: fp32 summation-order noise (measured 2.6e-7)
    assert mism.size <= 10                             # (measured: 0 of 200 704)
    assert worst <= 2 * eps_c + 2e-6                   # every one of them within the float tolerance of a decision boundary


def test_half_pixel_taps_are_atens_align_corners_false_and_both_statements_follow_them():
    """the code interpolation of the absent STEGO package as a switch.  The oracle's align_corners=False taps are ATen's
    (F.interpolate(..., align_corners=False)) up to rounding; the C restatement of the linear form equals its numpy statement bit for bit under them;
    the linear and the direct statement agree within the float tolerance of a decision boundary, as under align_corners=True."""
    from oracle import build_oracle, kmeans_linear as KL, segmap_agreement as SA

    build_oracle.build(force=False)
    code = torch.randn(9, 9, 12, generator=torch.Generator().manual_seed(0)) * 3
    got = torch.from_numpy(OI.upsample_bilinear_fixed(code.numpy(), 70, align_corners=False))
    aten = torch.nn.functional.interpolate(code.permute(2, 0, 1)[None], (70, 70), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    assert (got - aten).abs().max().item() < 1.5e-5          # (values up to ~10: fp32 operation-order noise; a wrong tap would be O(1))
    i0, i1, w0, w1 = OI.bilinear_taps_fixed(9, 70, align_corners=False)
    assert i0[0] == 0 and w1[0] == 0.0 and i0[-1] == 8 and i1[-1] == 8                    # clamped at both edges
    assert not np.array_equal(OI.bilinear_taps_fixed(9, 70)[3], w1)                       # (not the align_corners=True taps)
    rng = np.random.default_rng(9)
    for G, H, C, K in [(8, 64, 90, 5), (7, 50, 16, 4), (12, 9, 16, 3), (9, 70, 90, 17)]:
        c = (rng.standard_normal((G * G, C)) * (1 + rng.random((G * G, 1)))).astype(np.float32)
        lab_c, cent_c = KL.kmeans_pixels_linear(c, G, H, K, iters=4, align_corners=False)
        lab_n, cent_n = KL.kmeans_pixels_linear(c, G, H, K, iters=4, force_numpy=True, align_corners=False)
        assert np.array_equal(lab_c, lab_n) and np.array_equal(cent_c, cent_n), (G, H, C, K)
        assert not np.array_equal(lab_c, KL.kmeans_pixels_linear(c, G, H, K, iters=4)[0]) or H <= G    # the other reading is another map
    gen = torch.Generator().manual_seed(3)
    G, H, C, K = 28, 224, 90, 20
    c = torch.nn.functional.interpolate(torch.randn(1, C, 7, 7, generator=gen), (G, G), mode="bicubic")[0].permute(1, 2, 0).reshape(G * G, C) * 2 + 0.3
    c = c.numpy().astype(np.float32)
    ld, cd, x = SA.kmeans_pixels_full(c, G, H, K, form="direct", align_corners=False)
    ll, cl, x2 = SA.kmeans_pixels_full(c, G, H, K, form="linear", align_corners=False)
    assert np.array_equal(x, x2)
    eps_c = float(np.sqrt(((cd.astype(np.float64) - cl) ** 2).sum(1)).max())
    mism = np.nonzero(ld != ll)[0]
    assert mism.size <= 0.002 * ld.size
    if mism.size:
        sims = x[mism].astype(np.float64) @ cd.astype(np.float64).T
        assert (sims[np.arange(mism.size), ld[mism]] - sims[np.arange(mism.size), ll[mism]]).max() <= 2 * eps_c + 2e-6
