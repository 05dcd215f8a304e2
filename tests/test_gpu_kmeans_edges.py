"""The k-means kernels (csrc/stego.hip, csrc/stego_linear.hip) where Gaussian codes with at most 20 clusters never took them: the
instantiations above 20 clusters, exact ties, clusters that end up empty, zero rows, more clusters than points.  Every comparison is
bit for bit -- against the CPU oracle of the form under test (oracle/interfaces.py for the direct and the patch form,
oracle/kmeans_linear.py for the linear one; the two oracles legitimately differ from each other on degenerate input) and, for the
direct form, against the materialised GPU route.  The one number in this file is the screened kernel's exact-path share.

Which test launches which instantiation (run_kmeans_pixels routes on K; the assign-form switch does not reach K > 20):
  km_pix_assign_kernel<C, 32, false> at 20 < K <= 32, km_pix_partial_kernel<32>
      test_direct_form_above_20_clusters[8-64-*-21 / 27 / 32, 9-96-90-32, 9-97-90-27], test_direct_form_on_degenerate_codes[9-65-90-27]
  km_pix_assign_wide_kernel<C>, km_pix_partial_kernel<KM_MAXK>
      test_direct_form_above_20_clusters[8-64-*-33 / 40 / 64, 9-96-90-64, 9-97-90-40], test_more_clusters_than_pixels,
      test_direct_form_on_degenerate_codes[9-65-16-40, 17-129-90-64], test_no_write_outside_the_outputs_direct_form,
      test_more_than_20_clusters_through_the_class[40-direct]
  km_pix_assign_pk_kernel<C, true / false>, km_pix_assign_kernel<C, 20, true> and <C, 32, false>, km_pix_assign_screen_kernel, km_pix_partial_kernel<20> on ties,
  empty clusters and zero rows
      test_direct_form_on_degenerate_codes_all_assign_forms (9-65-90-20 and 9-65-16-6 under the five forms), test_screen_statistics
  WVN_LIN_RUN(32, 90)
      test_linear_form_slot_edges_and_32_slots_at_90_channels[8-64-90-21 / 27 / 32], test_linear_form_on_degenerate_codes[9-65-90-27],
      test_no_write_outside_the_outputs_linear_form, test_more_than_20_clusters_through_the_class[27-linear]
  lin_kp edges 8 | 9, 20 | 21, 32 at C = 16 and C = 90
      test_linear_form_slot_edges_and_32_slots_at_90_channels
  run_kmeans<90 / 64 / 16> above 20 clusters (km_assign_kernel, km_partial_kernel, km_update_kernel, km_relabel_kernel up to K = 64)
      test_patch_form_above_20_clusters, test_more_clusters_than_patches, test_no_write_outside_the_outputs_patch_form, and the materialised
      route inside every direct-form test
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_edge_cases as KE  # noqa: E402

from oracle import interfaces as OI, kmeans_linear as KL, vit as OV  # noqa: E402
from wild_visual_navigation_amd import ops  # noqa: E402
from wild_visual_navigation_amd._lib import check, lib, ptr, stream  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import StegoInterface  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = dict(argvalues=[1, 2, 0, 4, 5], ids=["screened", "screened-all-exact", "valu-plain", "valu-packed-dots", "valu-packed"])


def g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture
def assign_form(request):
    """The assignment kernels of the direct form at K <= 20 (tests/test_gpu_stego_pixels.py); -1: the default."""
    lib().wvn_debug_kmeans_assign_form(request.param)
    yield request.param
    lib().wvn_debug_kmeans_assign_form(-1)


@pytest.fixture
def band_rows(request):
    lib().wvn_debug_kmeans_linear_rows(request.param)   # (0 is out of range: the default)
    yield request.param
    lib().wvn_debug_kmeans_linear_rows(0)


def random_code(B, G, C, seed):
    """Gaussian codes with varying row norms, as in test_pixel_kmeans_bit_exact."""
    return torch.randn(B, G * G, C, generator=g(seed)) * (1.0 + torch.rand(B, G * G, 1, generator=g(1)))


def c_oracle():
    h = OI._oracle_lib()
    if h is None:
        pytest.skip("oracle/_build/libwvn_oracle.so is not built (python -m oracle.build_oracle): the numpy statement returns no centroids and takes minutes "
                    "above 4e7 multiply-adds per pass")
    return h


def oracle_rows(rows, K, iters=10):
    """(labels, final centroids) of the cosine k-means over ``rows`` [P, C]: the C restatement of kmeans_cosine_labels_numpy."""
    h = c_oracle()
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    P, C = rows.shape
    labels, cent, x = np.empty(P, dtype=np.int32), np.empty((K, C), dtype=np.float32), np.empty((P, C), dtype=np.float32)
    assert h.wvn_oracle_kmeans_cosine_ex(rows.ctypes.data, P, C, K, iters, labels.ctypes.data, cent.ctypes.data, x.ctypes.data) == 0
    return labels, cent


def oracle_direct(code, G, H, K):
    """oracle/segmap_agreement.py::kmeans_pixels_full(form="direct") without its copy of the rows."""
    return oracle_rows(OI.upsample_bilinear_fixed(code.reshape(G, G, -1), H).reshape(H * H, -1), K)


def oracle_linear(code, G, H, K):
    c_oracle()
    return KL.kmeans_pixels_linear(code, G, H, K, iters=10)


def check_pixels(dev, code, G, H, K, form, oracle, same_as=None):
    """code [B, G*G, C] through ops.kmeans_cosine_pixels in ``form``: labels, centroids, nseg and the relabelled map of every frame equal
    ``oracle(frame)`` = (labels, centroids); the direct form also equals the materialised GPU route (up-sample, normalise, cluster the
    H*H rows), labels AND centroids.  same_as: {frame: an earlier frame with the same code} -- its results must be the same bits."""
    B = code.shape[0]
    lab, nseg, cent = ops.kmeans_cosine_pixels(code.to(dev), G, H, K, iters=10, relabel=False, return_centroids=True, form=form)
    lab2, nseg2 = ops.kmeans_cosine_pixels(code.to(dev), G, H, K, iters=10, relabel=True, form=form)
    if form == "direct":
        dense = ops.upsample_bilinear(code.to(dev), G, H).permute(0, 2, 3, 1).reshape(B, H * H, -1).contiguous()
        lab_m, nseg_m, cent_m = ops.kmeans_cosine(dense, K, iters=10, relabel=False, return_centroids=True)
        assert torch.equal(lab, lab_m) and torch.equal(cent, cent_m) and torch.equal(nseg, nseg_m)
    lab, cent, lab2 = lab.cpu().numpy(), cent.cpu().numpy(), lab2.cpu().numpy()
    used = []
    for b in range(B):
        if same_as and b in same_as:
            a = same_as[b]
            assert np.array_equal(lab[b], lab[a]) and np.array_equal(cent[b].view(np.int32), cent[a].view(np.int32)) and np.array_equal(lab2[b], lab2[a])
            assert int(nseg[b]) == int(nseg[a]) == int(nseg2[b])
            used.append(used[a])
            continue
        want, wcent = oracle(b)
        assert np.array_equal(lab[b], want), f"frame {b}: {(lab[b] != want).mean()} of the labels differ"
        assert np.array_equal(cent[b], wcent), f"frame {b}: centroids of clusters {np.nonzero((cent[b] != wcent).any(1))[0].tolist()} differ"
        assert np.array_equal(lab2[b], OI.relabel_ascending(want))
        assert int(nseg[b]) == len(np.unique(want)) == int(nseg2[b])
        used.append(len(np.unique(want)))
    return used, lab2


# ---- instantiations above 20 clusters, random codes ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,H,C,K", [(8, 64, C, K) for C in (16, 90) for K in (21, 27, 32, 33, 40, 64)] + [(9, 96, 90, 32), (9, 96, 90, 64),
                                                                                                           (9, 97, 90, 27), (9, 97, 90, 40)])
def test_direct_form_above_20_clusters(dev, G, H, C, K):
    """(8, 64): 4096 pixels, km_super = 8.  (9, 96): 9216 pixels, km_super = 16, exactly nine groups of sixteen chunks; (9, 97): 9409 pixels -- a
    ragged last group (four chunks) with a ragged last chunk (one pixel).  K = 21 / 27 / 32: the 32-accumulator assign kernel reading past the frame's K
    centroids and the 32-register partial kernel; K = 33 / 40 / 64: the pixel-vector-resident assign kernel (K a multiple of four or not) and the
    64-register partial kernel.  wvn_debug_kmeans_assign_form is left alone: run_kmeans_pixels reads it for K <= 20 only, so the default form is
    the only one there is above 20 clusters."""
    B = 2
    code = random_code(B, G, C, G * H + K)
    check_pixels(dev, code, G, H, K, "direct", lambda b: oracle_direct(code[b].numpy(), G, H, K))


@pytest.mark.parametrize("G,H,C,K,band_rows", [(8, 64, 90, 21, 0), (8, 64, 90, 27, 0), (8, 64, 90, 27, 3), (8, 64, 90, 32, 0), (8, 64, 16, 8, 0), (8, 64, 16, 9, 0),
                                               (8, 64, 16, 20, 0), (8, 64, 16, 21, 0), (8, 64, 16, 32, 0), (8, 64, 90, 8, 0), (8, 64, 90, 9, 0), (8, 64, 90, 20, 0),
                                               (6, 100, 16, 32, 0), (6, 100, 16, 32, 16)], indirect=["band_rows"])
def test_linear_form_slot_edges_and_32_slots_at_90_channels(dev, band_rows, G, H, C, K):
    """lin_kp(K) = 8 | 20 | 32 table slots: both sides of every edge at both code dimensions, the 32-slot instantiation at C = 90 (K = 21, 27 and
    all 32 slots in use: bit 31 of the used-id masks), several chunks of rows per band at (6, 100).  band_rows: chunks of 3 and of 16 image rows on
    one case each (0: the default)."""
    B = 2
    code = random_code(B, G, C, G * H + K)
    check_pixels(dev, code, G, H, K, "linear", lambda b: oracle_linear(code[b].numpy(), G, H, K))


def check_patch_form(dev, code, K):
    lab, nseg, cent = ops.kmeans_cosine(code.to(dev), K, iters=10, relabel=False, return_centroids=True)
    lab2, nseg2 = ops.kmeans_cosine(code.to(dev), K, iters=10, relabel=True)
    used = []
    for b in range(code.shape[0]):
        want, wcent = oracle_rows(code[b].numpy(), K)
        assert np.array_equal(lab[b].cpu().numpy(), want) and np.array_equal(want, OI.kmeans_cosine_labels(code[b].numpy(), K)), f"frame {b}"
        assert np.array_equal(cent[b].cpu().numpy(), wcent), f"frame {b}"
        assert np.array_equal(lab2[b].cpu().numpy(), OI.relabel_ascending(want))
        assert int(nseg[b]) == len(np.unique(want)) == int(nseg2[b])
        used.append(len(np.unique(want)))
    return used, lab2.cpu().numpy()


@pytest.mark.parametrize("P,C,K", [(784, 90, 33), (3136, 90, 64), (784, 64, 40), (200, 16, 64)])
def test_patch_form_above_20_clusters(dev, P, C, K):
    """ops.kmeans_cosine (run_kmeans<90 / 64 / 16>) with more than 20 clusters: 28 x 28 and 56 x 56 patch grids, the 64-d head, a ragged last chunk."""
    code = torch.randn(2, P, C, generator=g(P + K)) * (1.0 + torch.rand(2, P, 1, generator=g(1)))
    check_patch_form(dev, code, K)


# ---- more clusters than points: duplicate initial centroids without crafted data ------------------------------------------------------------------

def test_more_clusters_than_patches(dev):
    """40 points, 64 clusters: every point is the initial centroid of one or two clusters; of two equal centroids the lower id takes the
    members, the other one stays empty and keeps its centroid; the relabelled ids close the gaps."""
    P, C, K = 40, 90, 64
    code = torch.randn(2, P, C, generator=g(4)) * (1.0 + torch.rand(2, P, 1, generator=g(1)))
    used, lab2 = check_patch_form(dev, code, K)
    for b in range(2):
        assert used[b] < K and np.array_equal(np.unique(lab2[b]), np.arange(used[b]))


def test_more_clusters_than_pixels(dev):
    """The direct pixel form on 25 pixels with 40 clusters (the pixel-vector-resident assign kernel, one ragged chunk)."""
    G, H, C, K = 3, 5, 16, 40
    code = random_code(2, G, C, 7)
    used, lab2 = check_pixels(dev, code, G, H, K, "direct", lambda b: oracle_direct(code[b].numpy(), G, H, K))
    for b in range(2):
        assert used[b] < K and np.array_equal(np.unique(lab2[b]), np.arange(used[b]))


# ---- ties, empty clusters, zero rows: tests/kmeans_edge_cases.py -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def degenerate_batch(G, H, C, K, nv, form):
    """Frames 0 and 1: the degenerate code (twice the same), frame 2: a Gaussian code -- a degenerate neighbour must not disturb a normal frame
    nor the other way round.  Returns (code [3, G*G, C], the oracle's (labels, centroids) of frames 0 and 2); computed once per fixture and form."""
    deg = torch.from_numpy(KE.degenerate_code(G, C, nv, seed=0))
    code = torch.stack([deg, deg, random_code(1, G, C, G * H + K)[0]])
    orc = oracle_direct if form == "direct" else oracle_linear
    return code, {0: orc(code[0].numpy(), G, H, K), 2: orc(code[2].numpy(), G, H, K)}


def check_degenerate(dev, G, H, C, K, nv, form):
    code, want = degenerate_batch(G, H, C, K, nv, form)
    used, lab2 = check_pixels(dev, code, G, H, K, form, lambda b: want[b], same_as={1: 0})
    assert used[0] < K and np.array_equal(np.unique(lab2[0]), np.arange(used[0]))      # empty clusters: the relabelled ids have no gaps


@pytest.mark.parametrize("assign_form", **FORMS, indirect=True)
@pytest.mark.parametrize("G,H,C,K,nv", KE.DIRECT_FIXTURES[:2], ids=["9-65-90-20", "9-65-16-6"])
def test_direct_form_on_degenerate_codes_all_assign_forms(dev, assign_form, G, H, C, K, nv):
    """Piecewise-constant integer codes (tests/test_oracle_stego.py proves them degenerate: at K = 20 twelve duplicate initial centroids, 578 zero
    rows, an exact tie between the two best similarities at 79 % of the pixels in the first pass, 15 clusters in use at the end): the tie-break
    between the halves of v_pk_fma_f32 and against the packed copy's mirror slots, the screened form's margin of exactly 0, cnt_s > 0 in
    km_update_kernel with its cpk mirror, the gap-closing lut of km_relabel_kernel."""
    check_degenerate(dev, G, H, C, K, nv, "direct")


@pytest.mark.parametrize("G,H,C,K,nv", KE.DIRECT_FIXTURES[2:], ids=["9-65-90-27", "9-65-16-40", "17-129-90-64"])
def test_direct_form_on_degenerate_codes(dev, G, H, C, K, nv):
    """The same above 20 clusters (the default form is the only one there): 22 of 27, 31 of 40 and 12 of 64 clusters in use at the end."""
    check_degenerate(dev, G, H, C, K, nv, "direct")


@pytest.mark.parametrize("G,H,C,K,nv", KE.LINEAR_FIXTURES, ids=["9-65-90-20", "9-65-90-27", "5-33-16-6"])
def test_linear_form_on_degenerate_codes(dev, G, H, C, K, nv):
    """The linear form's similarity table on zero-norm pixels (rinv = 1e12 enters the summed tap weights of cluster 0 and meets zero code), exact
    ties between interpolated table values, the member masks of empty clusters -- against the linear oracle."""
    check_degenerate(dev, G, H, C, K, nv, "linear")


# ---- the screened kernel's statistics --------------------------------------------------------------------------------------------------------

def screen_stats(dev, code, G, H, K):
    """(exact, seen, labels) of one direct-form call under wvn_debug_kmeans_assign_form(3): the screened kernel counting its 64-pixel row groups."""
    out = (ctypes.c_ulonglong * 2)()
    try:
        lib().wvn_debug_kmeans_assign_form(3)
        torch.cuda.synchronize()
        check(lib().wvn_debug_kmeans_screen_stats(out, 1), "wvn_debug_kmeans_screen_stats")     # (reset)
        lab, _ = ops.kmeans_cosine_pixels(code.to(dev), G, H, K, iters=10, relabel=False, form="direct")
        torch.cuda.synchronize()
        check(lib().wvn_debug_kmeans_screen_stats(out, 1), "wvn_debug_kmeans_screen_stats")
    finally:
        lib().wvn_debug_kmeans_assign_form(-1)
    return int(out[0]), int(out[1]), lab.cpu().numpy()


def test_screen_statistics(dev):
    """wvn_debug_kmeans_screen_stats.  `seen`: a workgroup of km_pix_assign_screen_kernel owns the run [yb, ye) of image rows whose upper source
    row is its patch row -- the runs of a frame's G workgroups partition its H image rows -- and walks it in items of (two rows, 64 pixels of x),
    counting the item's distinct rows: H * ceil(H / 64) per frame and pass, 11 passes.  On the degenerate fixture 0 < exact <= seen (margins of
    exactly 0 take the exact path); on a code with well-separated clusters exact < seen STRICTLY -- a screen that sent every row down the exact
    path would still give the right labels, only this count shows it.
    Measured on the MI355X: 1290 of 2860 row groups exact on the degenerate fixture (0.451), 154 of 9856 on the structured code (0.0156).  The share is a
    function of the data, not of timing: the structured code may take twice the measured share."""
    G, H, C, K, nv = KE.DIRECT_FIXTURES[0]
    code, want = degenerate_batch(G, H, C, K, nv, "direct")
    exact, seen, lab = screen_stats(dev, code[:2], G, H, K)
    print(f"\n  screened kernel, degenerate K = {K} fixture: {exact} of {seen} row groups exact ({exact / max(seen, 1):.4f})")
    assert seen == 11 * 2 * H * ((H + 63) // 64)
    assert 0 < exact <= seen
    assert np.array_equal(lab[0], want[0][0]) and np.array_equal(lab[1], want[0][0])
    G, H, C, K = 28, 224, 90, 20        # smooth code with cluster structure, as test_linear_and_direct_forms_agree_up_to_rounding_ties builds it
    code = torch.randn(1, C, 7, 7, generator=g(0))
    code = torch.nn.functional.interpolate(code, (G, G), mode="bicubic").permute(0, 2, 3, 1).reshape(1, G * G, C).contiguous() * 2 + 0.3
    exact, seen, lab = screen_stats(dev, code, G, H, K)
    print(f"  screened kernel, structured code at {H}^2: {exact} of {seen} row groups exact ({exact / max(seen, 1):.4f})")
    assert seen == 11 * H * ((H + 63) // 64)
    assert exact < seen
    assert exact <= 2 * 154      # (measured 154)
    assert np.array_equal(lab[0], oracle_direct(code[0].numpy(), G, H, K)[0])


# ---- no write outside the outputs --------------------------------------------------------------------------------------------------------------

GUARD, FILL = 4096, 0xA5


def guarded(nbytes, dev):
    buf = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0 and nbytes % 4 == 0
    return buf


def check_guards(K, labels, scratch, nlab, nscr):
    torch.cuda.synchronize()
    assert bool((labels[nlab:] == FILL).all()), "bytes behind the labels were written"
    assert bool((scratch[nscr:] == FILL).all()), "bytes behind the scratch area were written"
    lab = labels[:nlab].view(torch.int32)
    assert int(lab.min()) >= 0 and int(lab.max()) < K


@pytest.mark.parametrize("K", [33, 64])
def test_no_write_outside_the_outputs_direct_form(dev, K):
    """wvn_kmeans_cosine_pixels called as a C host would: `labels` exactly B * H * H int32 and `scratch` exactly wvn_kmeans_pixels_scratch_bytes, each
    followed by a 4 KB guard of 0xA5 that must come back untouched."""
    B, G, H, C = 2, 8, 64, 90
    code = random_code(B, G, C, K).to(dev)
    nlab, nscr = B * H * H * 4, lib().wvn_kmeans_pixels_scratch_bytes(B, G, H, C, K)
    labels, scratch, nseg = guarded(nlab, dev), guarded(nscr, dev), torch.empty(B, dtype=torch.int32, device=dev)
    check(lib().wvn_kmeans_cosine_pixels(ptr(code), ptr(labels), ptr(nseg), ptr(scratch), B, G, H, C, K, 10, 0, stream()), "wvn_kmeans_cosine_pixels")
    check_guards(K, labels, scratch, nlab, nscr)


def test_no_write_outside_the_outputs_patch_form(dev):
    B, P, C, K = 2, 784, 90, 64
    xn = torch.nn.functional.normalize(torch.randn(B, P, C, generator=g(5)), dim=2).contiguous().to(dev)
    nlab, nscr = B * P * 4, lib().wvn_kmeans_scratch_bytes(B, P, C, K)
    labels, scratch, nseg = guarded(nlab, dev), guarded(nscr, dev), torch.empty(B, dtype=torch.int32, device=dev)
    check(lib().wvn_kmeans_cosine(ptr(xn), ptr(labels), ptr(nseg), ptr(scratch), B, P, C, K, 10, 1, stream()), "wvn_kmeans_cosine")
    check_guards(K, labels, scratch, nlab, nscr)


def test_no_write_outside_the_outputs_linear_form(dev):
    B, G, H, C, K = 2, 8, 64, 90, 32
    code = random_code(B, G, C, K).to(dev)
    nlab, nscr = B * H * H * 4, lib().wvn_kmeans_pixels_linear_scratch_bytes(B, G, H, C, K)
    labels, scratch, nseg = guarded(nlab, dev), guarded(nscr, dev), torch.empty(B, dtype=torch.int32, device=dev)
    check(lib().wvn_kmeans_cosine_pixels_linear(ptr(code), ptr(labels), ptr(nseg), ptr(scratch), B, G, H, C, K, 10, 1, stream()), "wvn_kmeans_cosine_pixels_linear")
    check_guards(K, labels, scratch, nlab, nscr)


# ---- through the class ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,form", [(40, "direct"), (27, "linear")])
def test_more_than_20_clusters_through_the_class(dev, K, form):
    """StegoInterface(n_image_clusters=40, cluster_resolution="pixel"): the linear form stops at 32 clusters, so the class takes the direct form and
    its pixel-vector-resident kernel without a word -- the map must be the direct oracle's on the GPU's own code; at 27 clusters the linear oracle's."""
    S, G = 64, 8
    sd = OV.make_vit_state_dict("vit_small", 8, pretrain_grid=28, seed=11, depth=1)
    head = OI.make_stego_head_state_dict(384, 90, seed=2)
    img = torch.rand(2, 3, S, S, generator=g(13))
    st = StegoInterface(dev, input_size=S, n_image_clusters=K, run_clustering=True, run_crf=False, backbone_weights=sd, head_weights=head,
                        precision="exact", flip_tta=False, cluster_resolution="pixel", allow_synthetic=True)
    assert ops.kmeans_pixels_linear_supported(G, S, 90, K) == (form == "linear")
    _, cluster = st.inference(img.to(dev))
    assert cluster.shape == (1, 2, S, S) and cluster.dtype == torch.int32
    code = st.feature_tokens.cpu()
    for b in range(2):
        if form == "direct":
            want = OI.kmeans_cosine_labels_pixels(code[b].numpy(), G, S, K)
        else:
            want = KL.kmeans_cosine_labels_pixels_linear(code[b].numpy(), G, S, K)
        assert np.array_equal(cluster[0, b].cpu().numpy().reshape(-1), OI.relabel_ascending(want))
        assert int(st._n_segments[b]) == len(np.unique(want))
