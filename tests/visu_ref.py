"""The overlay pictures of wild_visual_navigation_amd (csrc/overlay.hip, ops.overlay / overlay_panels / image_to_u8, visu/) stated
plainly in torch on whatever device the inputs live on: the reference's lines (visu/visualizer.py: plot_image :516-537,
plot_segmentation :488-512, plot_detectron :313-364, plot_detectron_classification :368-421, plot_traversability_graph_on_seg
:208-237, plot_list :69-70) with the PIL alpha composite written as its integer formula.  No PIL, matplotlib or reference import.

Where the reference's casts are undefined the behaviour is DEFINED here (and in include/wvn_hip.h):
  * frame / colour-table values outside [0, 255] are clamped, NaN -> 0 (np.uint8 of such floats is undefined);
  * a value map's index is (v * 255) in fp32, truncated and clipped to [0, 255]; a non-finite PRODUCT gives 0 (what torch's CPU
    float -> long conversion followed by clip yields for NaN and +-inf);
  * a per-segment index is (pred[seg] * 255) truncated toward zero and NOT clipped, segment ids in [-S, 0) wrapping as torch
    indexing does; a non-finite product, an id outside [-S, S) and any index outside the colour table leave the plain pixel (the
    reference raises IndexError or wraps there);
  * a uint8 frame that is scaled (all values <= 1, or unit_range=True) saturates: non-zero -> 255;
  * boundaries: a pixel one of whose in-image 4-neighbours carries another label (parity with skimage's mark_boundaries, whose
    default mode="outer" may mark the other side of an edge, is unpinned: scikit-image is absent here).
"""
import torch


def alpha_byte(alpha) -> int:
    """np.uint8(alpha * 255) of ``fore[:, :, 3] = alpha * 255`` (float64), clamped to a byte."""
    return max(0, min(255, int(float(alpha) * 255)))


def blend(s: torch.Tensor, d: torch.Tensor, a) -> torch.Tensor:
    """PIL.Image.alpha_composite(opaque d, s with alpha byte a).convert("RGB"), per channel; uint8 in, uint8 out; a: int or tensor."""
    s, d = s.to(torch.int64), d.to(torch.int64)
    a = torch.as_tensor(a, device=d.device).to(torch.int64)
    t = s * (a * 128) + d * ((255 - a) * 128) + (0x80 << 7)
    o = (((t >> 8) + t) >> 8) >> 7
    return torch.where(a == 0, d, o).to(torch.uint8)


def to_u8(v: torch.Tensor) -> torch.Tensor:
    """float -> uint8 by truncation; clamp outside [0, 255], NaN -> 0."""
    v = torch.where(v != v, torch.zeros_like(v), v).clamp(0, 255)
    return v.to(torch.uint8)


def _frames(img):
    return img[None] if img.dim() == 3 else img


def image_to_u8(img: torch.Tensor, unit_range=None) -> torch.Tensor:
    """plot_image: [B,3,H,W] or [3,H,W] fp32 / uint8 -> uint8 [B,H,W,3]; the "max <= 1 -> * 255" decision per frame."""
    img = _frames(img)
    out = []
    for f in img:
        if f.dtype == torch.uint8:
            scale = bool(f.max() <= 1) if unit_range is None else bool(unit_range)
            o = torch.where(f != 0, torch.full_like(f, 255), f) if scale else f
        else:
            f = f.float()
            scale = bool(f.max() <= 1) if unit_range is None else bool(unit_range)   # (torch.max propagates NaN as numpy's does: no scaling)
            o = to_u8(f * 255 if scale else f)
        out.append(o.permute(1, 2, 0))
    return torch.stack(out).contiguous()


def lut_u8(lut: torch.Tensor) -> torch.Tensor:
    """c_map = (c_map * 255).type(torch.uint8) (visualizer.py:505); a uint8 table is used as it is."""
    return lut if lut.dtype == torch.uint8 else to_u8(lut * 255)


def index_values(v: torch.Tensor) -> torch.Tensor:
    """(seg * 255).type(torch.long).clip(0, 255) (visualizer.py:388), non-finite product -> 0."""
    t = v.float() * 255
    t = torch.where(torch.isfinite(t), t, torch.zeros_like(t)).clamp(0, 255)
    return t.to(torch.int64)


def index_segments(pred: torch.Tensor, seg: torch.Tensor, N: int) -> torch.Tensor:
    """(prediction[seg] * 255).type(torch.long) (visualizer.py:222) for one frame: pred [S], seg [H,W]; -1 = no colour."""
    S = pred.shape[0]
    s = seg.to(torch.int64)
    s = torch.where(s < 0, s + S, s)
    ok = (s >= 0) & (s < S)
    t = pred.float()[s.clamp(0, S - 1)] * 255
    fin = torch.isfinite(t)
    tt = torch.trunc(torch.where(fin, t, torch.zeros_like(t)))
    ok = ok & fin & (tt >= 0) & (tt < N)
    return torch.where(ok, tt, torch.full_like(tt, -1)).to(torch.int64)


def boundaries(seg: torch.Tensor) -> torch.Tensor:
    """[H,W] labels -> bool [H,W]: one of the in-image 4-neighbours carries another label."""
    e = torch.zeros(seg.shape, dtype=torch.bool, device=seg.device)
    dx = seg[:, 1:] != seg[:, :-1]
    dy = seg[1:, :] != seg[:-1, :]
    e[:, 1:] |= dx
    e[:, :-1] |= dx
    e[1:, :] |= dy
    e[:-1, :] |= dy
    return e


def overlay(img, values=None, labels=None, seg=None, lut=None, alpha=0.5, overlay_mask=None, boundary_seg=None, boundary_alpha=0,
            unit_range=None) -> torch.Tensor:
    """ops.overlay: uint8 [B,H,W,3]."""
    base = image_to_u8(img, unit_range)
    B, H, W, _ = base.shape
    table = lut_u8(lut)
    N = table.shape[0]
    a = alpha_byte(alpha)
    out = []
    for b in range(B):
        if labels is not None:
            idx = _frames3(labels, B)[b].to(torch.int64)
        elif seg is not None:
            v = values[None] if values.dim() == 1 else values
            idx = index_segments(v[b], _frames3(seg, B)[b], N)
        else:
            idx = index_values(_frames3(values, B)[b])
        painted = (idx >= 0) & (idx < N)
        col = table[idx.clamp(0, N - 1)]                                     # [H,W,3]
        al = torch.where(painted, torch.full_like(idx, a), torch.zeros_like(idx))
        if overlay_mask is not None:
            al = torch.where(_frames3(overlay_mask, B)[b].bool(), torch.zeros_like(al), al)   # fore[overlay_mask] = 0
        o = blend(col, base[b], al[..., None])
        if boundary_seg is not None and int(boundary_alpha) > 0:
            e = boundaries(_frames3(boundary_seg, B)[b])
            o = blend(torch.full_like(o, 255), o, torch.where(e, int(boundary_alpha), 0)[..., None])
        out.append(o)
    return torch.stack(out)


def _frames3(t, B):
    return t[None] if t.dim() == 2 else t


def overlay_panels(img, maps, lut, alpha=0.5, labels=False, seg=None, **kw) -> torch.Tensor:
    """ops.overlay_panels: [plain | overlay of maps[0] | ...] along the width (plot_list's np.concatenate(imgs, axis=1))."""
    unit_range = kw.get("unit_range")
    parts = [image_to_u8(img, unit_range)]
    for m in maps:
        if labels:
            parts.append(overlay(img, labels=m, lut=lut, alpha=alpha, **kw))
        else:
            parts.append(overlay(img, values=m, seg=seg, lut=lut, alpha=alpha, **kw))
    return torch.cat(parts, dim=2)
