"""LearningVisualizer with the reference's signatures and return types (visu/visualizer.py), composed on the GPU.

Every overlay method is one launch of csrc/overlay.hip on the tensors where they are, and returns the finished picture as a
np.uint8 HWC array -- one device -> host copy of 3 bytes per pixel -- or, with ``as_tensor=True``, the uint8 tensor on the
device.  Inputs that live on the host (numpy arrays, CPU tensors) are uploaded; there is no CPU composition path.

On the GPU path: plot_image, plot_segmentation, plot_detectron, plot_detectron_classification, plot_list,
plot_traversability_graph_on_seg, plot_mission_node_prediction, plot_mission_node_training.  plot_traversability_graph draws its
lines and ellipses with PIL.ImageDraw on the downloaded 8-bit frame as the reference does (per debug node, not per frame).
plot_roc, plot_histogram and the optical-flow plots (matplotlib figures) are not provided.

tests/visu_ref.py states the pictures; DESIGN.md section 4 "Overlays" the arithmetic and what is defined beyond the reference."""
import os
from typing import Optional

import numpy as np
import torch

from .. import ops
from .._lib import WvnError
from .colormaps import colour_table, default_classification_table
from .image_functionality import image_functionality

__all__ = ["LearningVisualizer"]


class LearningVisualizer:
    def __init__(self, p_visu: Optional[str] = None, store: Optional[bool] = False, pl_model=None, epoch: int = 0, log: bool = False):
        self._p_visu = p_visu
        self._pl_model = pl_model
        self._epoch = epoch
        self._store = store
        self._log = log
        self._tables = {}   # (name, n, device) -> colour table on that device; nothing is uploaded until first use
        if p_visu is not None:
            os.makedirs(p_visu, exist_ok=True)
        else:
            self._store = False

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_tables"] = {}   # device caches are rebuilt on first use
        return state

    epoch = property(lambda s: s._epoch, lambda s, v: setattr(s, "_epoch", v))
    store = property(lambda s: s._store, lambda s, v: setattr(s, "_store", v))

    # ---- helpers -------------------------------------------------------------------------------------------------------
    @staticmethod
    def _dev(x, device=None) -> torch.Tensor:
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if x.is_cuda:
            return x
        if not torch.cuda.is_available():
            raise WvnError("the overlays are composed on the GPU and none is available (there is no CPU fallback)")
        return x.to(device if device is not None else "cuda")

    def _table(self, colormap, n: int, device) -> torch.Tensor:
        """A colour map given by name (``sns.color_palette(name, n)``), as a tensor [N,3] / array, or None = the default of
        plot_detectron_classification, on ``device``."""
        if colormap is None or isinstance(colormap, str):
            key = (colormap, int(n), str(device))
            if key not in self._tables:
                t = default_classification_table() if colormap is None else colour_table(colormap, n)
                self._tables[key] = t.to(device)
            return self._tables[key]
        t = colormap if torch.is_tensor(colormap) else torch.from_numpy(np.asarray(colormap))
        return t.to(device)[:, :3]

    def _frame(self, img) -> torch.Tensor:
        """plot_image's accepted layouts: HWC (tested first, as the reference does) or CHW -> [3,H,W] on the device."""
        img = self._dev(img)
        if img.dim() != 3:
            raise WvnError(f"Invalid Shape: {tuple(img.shape)} (an image is CHW or HWC)")
        if img.shape[2] == 3:
            return img.permute(2, 0, 1)
        if img.shape[0] == 3:
            return img
        raise WvnError(f"Invalid Shape: {tuple(img.shape)} (an image is CHW or HWC)")

    @staticmethod
    def _map(seg, device) -> torch.Tensor:
        seg = LearningVisualizer._dev(seg, device)
        return seg[0] if seg.dim() == 3 and seg.shape[0] == 1 else seg

    @staticmethod
    def _result(t: torch.Tensor, kwargs):
        return t if kwargs.get("as_tensor", False) else t.cpu().numpy()

    # ---- pictures ------------------------------------------------------------------------------------------------------
    @image_functionality
    def plot_list(self, imgs, **kwargs):
        if all(torch.is_tensor(i) for i in imgs):
            return self._result(torch.cat(list(imgs), dim=1), kwargs)
        return np.concatenate([i.cpu().numpy() if torch.is_tensor(i) else i for i in imgs], axis=1)

    @image_functionality
    def plot_image(self, img, **kwargs):
        """img: CHW or HWC, tensor or array, range 0-1 or 0-255 -> uint8 HWC."""
        return self._result(ops.image_to_u8(self._frame(img))[0], kwargs)

    @image_functionality
    def plot_segmentation(self, seg, max_seg=40, colormap="Set2", **kwargs):
        seg = self._map(seg, None)
        if seg.dtype == torch.bool:
            max_seg = 2
        lut = self._table(colormap, max_seg, seg.device)
        H, W = seg.shape
        black = torch.zeros(1, 3, H, W, dtype=torch.uint8, device=seg.device)   # an id outside the table stays black
        return self._result(ops.overlay(black, labels=seg, lut=lut, alpha=1.0, unit_range=False)[0], kwargs)

    @image_functionality
    def plot_detectron(self, img, seg, alpha=0.5, draw_bound=True, max_seg=40, colormap="Set2", overlay_mask=None, boundary_seg=None,
                       boundary_alpha=0, **kwargs):
        img = self._frame(img)
        seg = self._map(seg, img.device)
        if seg.dtype == torch.bool:
            max_seg = 2
        lut = self._table(colormap, max_seg, img.device)
        bseg = None
        if draw_bound and boundary_alpha:   # boundary_alpha = 0 (the default): the second composite is the identity
            bseg = self._map(boundary_seg if boundary_seg is not None else seg, img.device)
        mask = None if overlay_mask is None else self._map(overlay_mask, img.device)
        out = ops.overlay(img, labels=seg, lut=lut, alpha=alpha, overlay_mask=mask, boundary_seg=bseg,
                          boundary_alpha=int(boundary_alpha))
        return self._result(out[0], kwargs)

    @image_functionality
    def plot_detectron_classification(self, img, seg, alpha=0.5, overlay_mask=None, **kwargs):
        img = self._frame(img)
        cmap = kwargs.get("cmap", None)
        lut = self._table(cmap, 256, img.device)
        mask = None if overlay_mask is None else self._map(overlay_mask, img.device)
        out = ops.overlay(img, values=self._map(seg, img.device), lut=lut, alpha=alpha, overlay_mask=mask)
        return self._result(out[0], kwargs)

    @image_functionality
    def plot_traversability_graph_on_seg(self, prediction, seg, graph, center, img, max_val=1.0, colormap="RdYlBu",
                                         colorize_invalid_centers=False, **kwargs):
        img = self._frame(img)
        lut = self._table(colormap, 256, img.device)
        out = ops.overlay(img, values=self._dev(prediction, img.device).reshape(1, -1), seg=self._map(seg, img.device), lut=lut, alpha=0.6)
        return self._result(out[0], kwargs)

    @image_functionality
    def plot_traversability_graph(self, prediction, graph, center, img, max_val=1.0, colormap="RdYlBu", colorize_invalid_centers=False,
                                  **kwargs):
        """The segment graph drawn on the frame (host side, PIL.ImageDraw): grey edges, one filled ellipse per segment centre in
        the colour of its prediction."""
        from PIL import Image, ImageDraw

        prediction = torch.as_tensor(prediction).detach().cpu()
        assert prediction.max() <= max_val and prediction.min() >= 0, \
            f"Pred out of Bounds: 0-1, Given: {prediction.min()}-{prediction.max()}"
        radius = 5
        index = (prediction.float() * 255).to(torch.uint8)
        frame = ops.image_to_u8(self._frame(img), unit_range=True)[0].cpu().numpy()   # np.uint8(img * 255)
        pil = Image.fromarray(frame)
        draw = ImageDraw.Draw(pil)
        edges = torch.as_tensor(graph.edge_index).cpu()
        center = torch.as_tensor(center).cpu()
        valid = getattr(graph, "y_valid", None)
        valid = [True] * center.shape[0] if valid is None else torch.as_tensor(valid).cpu().tolist()
        table = self._table(colormap, 256, "cpu")
        table = table if table.dtype == torch.uint8 else (table * 255).to(torch.uint8)
        for i in range(edges.shape[1]):
            a, b = int(edges[0, i]), int(edges[1, i])
            draw.line(center[a].tolist() + center[b].tolist(), fill=(127, 127, 127))
        for i in range(center.shape[0]):
            c = center[i].tolist()
            box = [p - radius for p in c] + [p + radius for p in c]
            if valid[i] or colorize_invalid_centers:
                draw.ellipse(box, width=10, fill=tuple(table[int(index[i])].tolist()))
            else:
                draw.ellipse(box, width=1, fill=(127, 127, 127))
        out = np.array(pil)
        return torch.from_numpy(out) if kwargs.get("as_tensor", False) else out

    # ---- mission nodes (TraversabilityEstimator.plot_mission_node_prediction / _training) -------------------------------------
    def plot_mission_node_prediction(self, node, **kwargs):
        if node._image is None or node._prediction is None:
            return None
        pred = self._dev(node._prediction)
        trav = pred[:, 0]
        # get_confidence (utils/get_confidence.py of the reference), on the device: min / max normalised reconstruction loss
        res = torch.nn.functional.mse_loss(pred[:, 1:], self._dev(node._features, pred.device), reduction="none").mean(1)
        res = res - res.min()
        conf = 1 - res / res.max()
        common = dict(colormap="RdYlBu", colorize_invalid_centers=True, not_log=True, store=False, as_tensor=kwargs.get("as_tensor", False))
        trav_img = self.plot_traversability_graph_on_seg(trav, node.feature_segments, None, node.feature_positions, node.image, **common)
        conf_img = self.plot_traversability_graph_on_seg(conf, node.feature_segments, None, node.feature_positions, node.image, **common)
        return trav_img, conf_img

    def plot_mission_node_training(self, node, **kwargs):
        if node._image is None or node._prediction is None:
            return None
        as_tensor = kwargs.get("as_tensor", False)
        if node.supervision_signal is None:
            sa = node.image.shape
            supervision_img = np.zeros((sa[1], sa[2], sa[0]), dtype=np.uint8)
            if as_tensor:
                supervision_img = torch.from_numpy(supervision_img)
        else:
            supervision_img = self.plot_traversability_graph(node.supervision_signal, node.as_pyg_data(), node.feature_positions,
                                                             node.image, colormap="RdYlBu", store=False, as_tensor=as_tensor)
        sm = self._dev(node.supervision_mask)
        mask = torch.isnan(sm)
        labels = torch.round(torch.clamp(255 * torch.where(mask, torch.zeros_like(sm), sm)[0], 0, 255)).to(torch.int32)
        mask_img = self.plot_detectron(node.image, labels, max_seg=256, colormap="RdYlBu", overlay_mask=mask[0], draw_bound=False,
                                       store=False, as_tensor=as_tensor)
        return supervision_img, mask_img
