"""The overlay statement (tests/visu_ref.py) against what it restates -- PIL's alpha composite, matplotlib's colour map -- and the
parts of the overlay path that need no GPU: argument validation of the C entry points and of ops, the package import."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import visu_ref as VR
from wild_visual_navigation_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA_BYTES = (0, 1, 76, 127, 128, 153, 254, 255)


@pytest.mark.parametrize("masked", [False, True])
def test_blend_formula_equals_pil_alpha_composite_for_every_byte_pair(masked):
    """visualizer.py:329-344 with PIL itself, against visu_ref.blend: foreground byte = column, background byte = row, every alpha
    byte the issue names; with a mask, ``fore[overlay_mask] = 0`` clears colour AND alpha of the masked pixels."""
    Image = pytest.importorskip("PIL.Image")
    fg = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (256, 256, 3))
    bg = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None], (256, 256, 3))
    mask = (np.add.outer(np.arange(256), np.arange(256)) % 3 == 0) if masked else None
    for a in ALPHA_BYTES:
        back = np.zeros((256, 256, 4))
        back[:, :, :3] = bg
        back[:, :, 3] = 255
        fore = np.zeros((256, 256, 4))
        fore[:, :, :3] = fg
        fore[:, :, 3] = a
        if masked:
            fore[mask] = 0
        want = np.array(Image.alpha_composite(Image.fromarray(np.uint8(back)), Image.fromarray(np.uint8(fore))).convert("RGB"), dtype=np.uint8)
        al = torch.full((256, 256, 1), a, dtype=torch.int64)
        if masked:
            al[torch.from_numpy(mask)] = 0
        got = VR.blend(torch.from_numpy(fg.copy()), torch.from_numpy(bg.copy()), al)
        assert torch.equal(got, torch.from_numpy(want)), a


def test_alpha_byte_is_the_reference_cast():
    for alpha, byte in ((0, 0), (0.3, 76), (0.5, 127), (0.6, 153), (1.0, 255), (1, 255)):
        assert VR.alpha_byte(alpha) == byte == ops.alpha_byte(alpha) == int(np.uint8(np.float64(alpha) * 255))


def test_packaged_default_table_equals_the_reference_construction():
    """visualizer.py:379-384, then plot_segmentation's (c_map * 255).type(torch.uint8) on the fp32 table (:384 ``.to(seg)``, :505)."""
    matplotlib = pytest.importorskip("matplotlib")
    from wild_visual_navigation_amd.visu import colour_table, default_classification_table

    s = 0.3
    cmap = matplotlib.colormaps["RdYlBu"].resampled(256)            # cm.get_cmap("RdYlBu", 256)
    c = np.concatenate([cmap(np.linspace(0, s, 128)), cmap(np.linspace(1 - s, 1.0, 128))])
    want = (torch.from_numpy(c).to(torch.float32)[:, :3] * 255).type(torch.uint8)
    got = default_classification_table()
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    # the second packaged table: seaborn's sampling rule for "RdYlBu" with 256 entries (unpinned against seaborn itself)
    full = matplotlib.colormaps["RdYlBu"]
    want2 = (torch.tensor(full(np.linspace(0, 1, 258)[1:-1])[:, :3].tolist(), dtype=torch.float32) * 255).type(torch.uint8)
    assert torch.equal(colour_table("RdYlBu", 256), want2)
    # a qualitative map is cycled, any other sampled at interior points
    set2 = colour_table("Set2", 40)
    assert set2.shape == (40, 3) and set2.dtype == torch.float32 and torch.equal(set2[:8], set2[8:16])
    blues = colour_table("Blues", 256)
    assert torch.equal(blues, torch.tensor(matplotlib.colormaps["Blues"](np.linspace(0, 1, 258)[1:-1])[:, :3].tolist(), dtype=torch.float32))


def test_unknown_colour_map_names_the_missing_package():
    from wild_visual_navigation_amd.visu import colour_table

    with pytest.raises(_lib.WvnError, match="seaborn"):
        colour_table("no_such_colour_map", 7)


def _desc(**kw):
    words = (C.c_longlong * 8)()
    p = C.addressof(words)   # (never dereferenced: every call below is refused before a launch)
    d = _lib.OverlayDesc()
    d.img, d.out, d.lut = p, p, p
    d.maps[0] = p
    d.B, d.H, d.W, d.N, d.nmaps, d.plain, d.alpha, d.unit_range = 1, 8, 8, 256, 1, 0, 127, 1
    d.out_row_bytes, d.out_frame_bytes = 24, 192
    for k, v in kw.items():
        setattr(d, k, v)
    return d, words


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    h = _lib.lib()
    bad = [dict(N=1025), dict(N=0), dict(nmaps=5), dict(H=0), dict(W=0), dict(B=0), dict(B=65536), dict(alpha=256), dict(alpha=-1),
           dict(boundary_alpha=256), dict(kind=3), dict(out_row_bytes=23), dict(unit_range=-1), dict(img=None), dict(out=None),
           dict(lut=None), dict(kind=_lib.OVERLAY_LABELS, id_bytes=2), dict(kind=_lib.OVERLAY_SEGMENTS, S=4, seg_bytes=4),
           dict(plain=1), dict(nmaps=2)]
    for kw in bad:
        d, words = _desc(**kw)
        assert h.wvn_overlay(C.byref(d), None) == _lib.ERR_ARG, kw
        assert all(w == 0 for w in words)
    for kw in (dict(plain=0), dict(plain=1, nmaps=5, out_row_bytes=24 * 6), dict(plain=1, nmaps=1, out_row_bytes=47),
               dict(plain=1, nmaps=1, out_row_bytes=48, N=1025), dict(plain=2)):
        d, _ = _desc(**kw)
        assert h.wvn_overlay_panels(C.byref(d), None) == _lib.ERR_ARG, kw
    assert h.wvn_overlay(None, None) == _lib.ERR_ARG and h.wvn_overlay_panels(None, None) == _lib.ERR_ARG
    p = C.addressof((C.c_longlong * 2)())
    assert h.wvn_frame_max(None, 0, 1, 12, p, None) == _lib.ERR_ARG and h.wvn_frame_max(p, 0, 1, 12, None, None) == _lib.ERR_ARG
    assert h.wvn_frame_max(p, 0, 0, 12, p, None) == _lib.ERR_ARG and h.wvn_frame_max(p, 0, 1, 0, p, None) == _lib.ERR_ARG
    assert C.sizeof(_lib.OverlayDesc) == 11 * 8 + 2 * 8 + 16 * 4


def test_ops_refuse_mismatched_shapes_and_cpu_tensors():
    img = torch.zeros(2, 3, 8, 8)
    lut = torch.zeros(256, 3, dtype=torch.uint8)
    with pytest.raises(_lib.WvnError, match="shape"):
        ops.overlay(torch.zeros(2, 4, 8, 8), values=torch.zeros(2, 8, 8), lut=lut)
    with pytest.raises(_lib.WvnError, match="GPU"):
        ops.overlay(img, values=torch.zeros(2, 8, 8), lut=lut)      # no CPU fallback
    with pytest.raises(_lib.WvnError):
        ops.overlay(img, lut=lut)                                    # neither values nor labels
    with pytest.raises(_lib.WvnError):
        ops.overlay(img, values=torch.zeros(2, 8, 8), labels=torch.zeros(2, 8, 8, dtype=torch.int32), lut=lut)
    with pytest.raises(_lib.WvnError, match="at most 4"):
        ops.overlay_panels(img, [torch.zeros(2, 8, 8)] * 5, lut)
    with pytest.raises(_lib.WvnError, match="GPU"):
        ops.image_to_u8(img)


def test_visu_imports_without_pil_and_matplotlib():
    code = ("import sys; sys.modules['PIL'] = None; sys.modules['matplotlib'] = None; sys.modules['seaborn'] = None\n"
            "import wild_visual_navigation_amd.visu as v\n"
            "assert v.LearningVisualizer()._store is False and v.default_classification_table().shape == (256, 3)\n"
            "assert 'PIL' not in [m for m, o in sys.modules.items() if o is not None] and 'matplotlib.pyplot' not in sys.modules\n"
            "import wild_visual_navigation_amd.dropin as d\n"
            "assert d.install(force_synthetic=True) == 'synthetic'\n"
            "from wild_visual_navigation.visu import LearningVisualizer\n"
            "assert LearningVisualizer is v.LearningVisualizer\n"
            "import pickle\n"
            "lv = v.LearningVisualizer(); lv._tables['x'] = object()\n"
            "assert pickle.loads(pickle.dumps(lv))._tables == {}\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_estimator_holds_a_visualizer_and_the_reference_methods():
    from wild_visual_navigation_amd.cfg import ExperimentParams
    from wild_visual_navigation_amd.traversability_estimator import MissionNode, TraversabilityEstimator
    from wild_visual_navigation_amd.visu import LearningVisualizer

    p = ExperimentParams()
    p.model.simple_mlp_cfg.input_size = 16
    te = TraversabilityEstimator(p, device="cpu")
    assert isinstance(te._visualizer, LearningVisualizer) and te._visualizer._tables == {}
    n = MissionNode()
    assert te.plot_mission_node_prediction(n) is None and te.plot_mission_node_training(n) is None   # no image: as the reference
