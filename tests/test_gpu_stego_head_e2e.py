"""StegoInterface with the head run off the backbone's residual rows (VitBackbone.forward_tokens_pair(head=): final LayerNorm on load, no
token tensor) against the oracle and against the separate launches it replaces (fuse_head=False), on a depth-2 ViT-S/8 at 448^2 with the flip
pass: 2 frames + 2 mirrors = 12 608 token rows, above the 8192-row threshold of the split-operand block kernels.  Also: the code of a frame
does not depend on the batch or the chunking (the kernel's per-element summation order depends neither on M nor on the unit split), and
below the threshold the existing path runs, bit for bit, whatever the switch says."""
import pytest
import torch

from oracle import interfaces as OI, vit as OV
from wild_visual_navigation_amd.backbone import StegoHead
from wild_visual_navigation_amd.feature_extractor.stego_interface import StegoInterface

pytestmark = pytest.mark.gpu

S, P, HEADS = 448, 8, 6


@pytest.fixture(scope="module")
def setup():
    sd = OV.make_vit_state_dict("vit_small", P, pretrain_grid=28, seed=21, depth=2)
    head = OI.make_stego_head_state_dict(384, 90, seed=5)
    img = torch.rand(3, 3, S, S, generator=torch.Generator().manual_seed(22))
    x = OI.dino_transform(img[:2], S)
    tok, tok_m = OV.vit_tokens(sd, x, P, HEADS)[:, 1:], OV.vit_tokens(sd, x.flip(-1), P, HEADS)[:, 1:]
    return sd, head, img, OI.stego_code_flip_average(head, tok, tok_m, S // P), OI.stego_code_tokens(head, tok)    # reference codes of frames 0 - 1, computed once


def _si(dev, sd, head, prec, fuse, size=S, flip_tta=True, **kw):
    return StegoInterface(dev, input_size=size, n_image_clusters=6, run_crf=False, run_clustering=True, backbone_weights=sd, head_weights=head,
                          precision=prec, flip_tta=flip_tta, fuse_head=fuse, **kw)


@pytest.fixture
def separate_products(monkeypatch):
    """Counts the chunks on which the library declined the fused route (StegoHead.apply: tokens + three separate products)."""
    calls = []
    apply = StegoHead.apply

    def counted(self, *a, **k):
        calls.append(1)
        return apply(self, *a, **k)

    monkeypatch.setattr(StegoHead, "apply", counted)
    return calls


_CODES = {}


def _codes(dev, setup, prec):
    """(code with the head fused, code with the separate launches) of frames 0 - 1, computed once per precision."""
    if prec not in _CODES:
        sd, head, img = setup[:3]
        x = img[:2].to(dev)
        declined, apply = [], StegoHead.apply
        StegoHead.apply = lambda self, *a, **k: (declined.append(1), apply(self, *a, **k))[1]
        try:
            fused = _si(dev, sd, head, prec, True).code_tokens(x).cpu()
        finally:
            StegoHead.apply = apply
        assert not declined, "12 608 rows: the fused route must have run"
        plain_si = _si(dev, sd, head, prec, False)
        assert plain_si._head is None
        _CODES[prec] = (fused, plain_si.code_tokens(x).cpu())
    return _CODES[prec]


@pytest.mark.parametrize("prec", ["mixed", "exact"])
def test_fused_head_against_oracle(dev, setup, prec):
    fused, plain = _codes(dev, setup, prec)
    ref = setup[3]
    e_fused, e_plain = (fused - ref).abs().max().item(), (plain - ref).abs().max().item()
    print(f"[{prec}] code vs oracle: fused {e_fused:.3e}, separate launches {e_plain:.3e}")
    assert e_fused <= 1.25 * e_plain + 1e-5, (e_fused, e_plain)
    assert e_fused < 1e-3


@pytest.mark.parametrize("prec", ["mixed", "exact"])
def test_fused_head_against_separate_launches(dev, setup, prec):
    """The fused route computes what the separate launches compute: the statistics pass has the LayerNorm kernel's arithmetic, the tokens are formed
    on load in its operation order, and the A-stationary launch sums hi*lo + lo*hi + hi*hi per k-step from a zero accumulator with the bias behind
    it, as the tiled kernel does.  Required: closer than 1e-5; measured on MI355X: bit-identical (0.0) in both precisions, which is also asserted
    -- the benchmark's outputs then do not depend on the switch."""
    fused, plain = _codes(dev, setup, prec)
    e_pair = (fused - plain).abs().max().item()
    print(f"[{prec}] fused vs separate launches {e_pair:.3e}")
    assert e_pair < 1e-5
    assert torch.equal(fused, plain)


@pytest.mark.parametrize("prec", ["mixed", "exact"])
def test_code_does_not_depend_on_batch_or_chunking(dev, setup, prec):
    """Frames 0 - 1 of a three-frame run, in one chunk and in chunks of two, are the two-frame run bit for bit."""
    sd, head, img = setup[:3]
    fused, _ = _codes(dev, setup, prec)
    for chunk in (3, 2):
        got = _si(dev, sd, head, prec, True, max_chunk=chunk).code_tokens(img.to(dev)).cpu()
        assert torch.equal(got[:2], fused), (prec, chunk)


@pytest.mark.parametrize("prec", ["mixed", "exact"])
def test_single_pass_form(dev, setup, separate_products, prec):
    """flip_tta=False: one backbone pass (forward_tokens(head=)), the padded rows narrowed by the flip-average kernel's no-mirror form.  Three frames
    = 9456 token rows; frames 0 - 1 against the oracle, with the bounds of the paired form."""
    sd, head, img, ref = setup[0], setup[1], setup[2], setup[4]
    x = img.to(dev)
    fused = _si(dev, sd, head, prec, True, flip_tta=False).code_tokens(x).cpu()[:2]
    assert not separate_products
    plain = _si(dev, sd, head, prec, False, flip_tta=False).code_tokens(x).cpu()[:2]
    e_fused, e_plain = (fused - ref).abs().max().item(), (plain - ref).abs().max().item()
    print(f"[{prec}] single pass, code vs oracle: fused {e_fused:.3e}, separate launches {e_plain:.3e}")
    assert e_fused <= 1.25 * e_plain + 1e-5 and e_fused < 1e-3, (e_fused, e_plain)


@pytest.mark.parametrize("prec", ["mixed", "exact"])
def test_below_the_threshold_the_existing_path_runs(dev, setup, separate_products, prec):
    sd, head, img = setup[:3]
    x = img[:1, :, :224, :224].contiguous().to(dev)          # 224^2, one frame + its mirror: 1600 token rows
    with_head = _si(dev, sd, head, prec, True, size=224).code_tokens(x)
    assert len(separate_products) == 1, "the library must decline and the separate products run"
    assert torch.equal(with_head, _si(dev, sd, head, prec, False, size=224).code_tokens(x))


def test_off_switch_is_read_at_construction(dev, setup, monkeypatch):
    sd, head = setup[:2]
    monkeypatch.setenv("WVN_NO_HEAD_FUSE", "1")
    si = _si(dev, sd, head, "mixed", None, size=224)
    assert si._head is None
    monkeypatch.delenv("WVN_NO_HEAD_FUSE")
    assert si._head is None and _si(dev, sd, head, "mixed", None, size=224)._head is not None
