"""LearningVisualizer with the reference's signatures and return types (visu/visualizer.py), composed on the GPU.

Every overlay method is one launch of csrc/overlay.hip on the tensors where they are, and returns the finished picture as a
np.uint8 HWC array -- one device -> host copy of 3 bytes per pixel -- or, with ``as_tensor=True``, the uint8 tensor on the
device.  Inputs that live on the host (numpy arrays, CPU tensors) are uploaded; there is no CPU composition path.

On the GPU path: plot_image, plot_segmentation, plot_detectron, plot_detectron_classification, plot_list,
plot_traversability_graph_on_seg, plot_mission_node_prediction, plot_mission_node_training, and the views that draw lines and
ellipses -- plot_traversability_graph, plot_graph_result, plot_optical_flow, plot_sparse_optical_flow: the reference draws them with
PIL.ImageDraw, primitive by primitive on the host; here the primitive list is assembled with torch operations on the device and one
launch of csrc/draw.hip paints it, bit for bit what PIL paints (ops.draw).  No method needs PIL at run time (only ``store=True``
writes its PNG with it), every ``as_tensor=True`` result is a device tensor.  plot_roc and plot_histogram (matplotlib figures) are
not provided.

tests/visu_ref.py and tests/visu_draw_ref.py state the pictures; DESIGN.md section 4 "Overlays" and "Overlays: vector primitives" the
arithmetic and what is defined beyond the reference."""
import os
from typing import Optional

import numpy as np
import torch

from .. import ops
from .._lib import WvnError
from .colormaps import colour_table, default_classification_table, graph_result_table
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
                                         colorize_invalid_centers=False, draw_graph=False, **kwargs):
        """``draw_graph=True`` (not in the reference, whose tail doing this is commented out): the segment graph of
        plot_traversability_graph drawn on the overlay bytes in a second launch."""
        img = self._frame(img)
        lut = self._table(colormap, 256, img.device)
        prediction = self._dev(prediction, img.device)
        out = ops.overlay(img, values=prediction.reshape(1, -1), seg=self._map(seg, img.device), lut=lut, alpha=0.6)
        if draw_graph:
            self._draw(out, *self._traversability_graph_list(prediction, graph, center, max_val, colormap, colorize_invalid_centers, 1))
        return self._result(out[0], kwargs)

    # ---- vector primitives (csrc/draw.hip): the lists are assembled with torch operations on the device ------------------------
    @staticmethod
    def _draw(canvas, kinds, points, colours, frame, panel, panel_width=None):
        step = ops._lib.DRAW_MAX_PRIMITIVES   # a longer list goes in index order, so the painter's order holds across launches
        for i in range(0, max(int(kinds.shape[0]), 1), step):
            ops.draw(canvas, kinds[i:i + step], points[i:i + step], colours[i:i + step], frame[i:i + step], panel[i:i + step], panel_width)
        return canvas

    @staticmethod
    def _graph_list(edges, center, node_colours, edge_colour):
        """edges [2,E], center [B,N,2], node_colours: one uint8 [B,N,3] per panel -> per (panel, frame): the E edges as thin lines in
        edge order, then the N discs in node order."""
        dev = center.device
        B, N, _ = center.shape
        E, P = edges.shape[1], len(node_colours)
        center = center.float()
        lines = torch.cat([center[:, edges[0]], center[:, edges[1]]], dim=2)                                   # [B,E,4]
        discs = torch.cat([center, torch.zeros_like(center)], dim=2)                                           # [B,N,4]
        points = torch.cat([lines, discs], dim=1)[None].expand(P, B, E + N, 4)
        grey = torch.tensor(edge_colour, dtype=torch.uint8, device=dev).expand(B, E, 3)
        colours = torch.stack([torch.cat([grey, c], dim=1) for c in node_colours])                             # [P,B,E+N,3]
        kinds = torch.cat([torch.full((E,), ops._lib.DRAW_LINE, dtype=torch.int32, device=dev),
                           torch.full((N,), ops._lib.DRAW_DISC, dtype=torch.int32, device=dev)]).expand(P, B, E + N)
        frame = torch.arange(B, dtype=torch.int32, device=dev)[None, :, None].expand(P, B, E + N)
        panel = torch.arange(P, dtype=torch.int32, device=dev)[:, None, None].expand(P, B, E + N)
        return kinds.reshape(-1), points.reshape(-1, 4), colours.reshape(-1, 3), frame.reshape(-1), panel.reshape(-1)

    def _u8_table(self, table):
        return table if table.dtype == torch.uint8 else (table * 255).to(torch.uint8)

    def _traversability_graph_list(self, prediction, graph, center, max_val, colormap, colorize_invalid_centers, B):
        assert prediction.max() <= max_val and prediction.min() >= 0, \
            f"Pred out of Bounds: 0-1, Given: {prediction.min()}-{prediction.max()}"
        dev = prediction.device
        center = self._dev(center, dev)
        center = center.reshape(B, -1, 2)
        N = center.shape[1]
        index = (prediction.detach().float() * 255).to(torch.uint8).reshape(B, N)
        colours = self._u8_table(self._table(colormap, 256, dev))[index.long()]                                # [B,N,3]
        valid = getattr(graph, "y_valid", None)
        if valid is not None and not colorize_invalid_centers:
            valid = self._dev(valid, dev).bool().reshape(-1, N).expand(B, N)
            colours = torch.where(valid[..., None], colours, torch.full_like(colours, 127))
        return self._graph_list(self._dev(graph.edge_index, dev).long(), center, [colours], (127, 127, 127))

    @image_functionality
    def plot_traversability_graph(self, prediction, graph, center, img, max_val=1.0, colormap="RdYlBu", colorize_invalid_centers=False,
                                  **kwargs):
        """The segment graph drawn on the frame: grey edges in edge order, then one filled ellipse per segment centre in node
        order, in the colour of its prediction (grey for an invalid node unless ``colorize_invalid_centers``).  One frame
        (img [3,H,W], center [N,2], prediction [N]) or a batch sharing one graph (img [B,3,H,W], center [B,N,2], prediction [B,N])."""
        img = self._dev(img)
        batched = img.dim() == 4
        img = img if batched else self._frame(img)[None]
        prediction = self._dev(prediction, img.device)
        canvas = ops.image_to_u8(img, unit_range=True)   # np.uint8(img * 255)
        self._draw(canvas, *self._traversability_graph_list(prediction, graph, center, max_val, colormap, colorize_invalid_centers,
                                                            img.shape[0]))
        return self._result(canvas if batched else canvas[0], kwargs)

    def _graph_result_table(self, colormap, device) -> torch.Tensor:
        key = ("graph_result", colormap, str(device))
        if key not in self._tables:
            self._tables[key] = graph_result_table(colormap).to(device)
        return self._tables[key]

    @image_functionality
    def plot_graph_result(self, graph, center, img, seg, res, use_seg=False, colormap="RdYlBu", **kwargs):
        """[prediction | ground truth | (segmentation)] side by side: the frame (the third panel: plot_segmentation(seg, max_seg=100))
        with the graph on top -- red edges, discs coloured by ``res.clip(0, 1)`` and ``graph.y`` -- drawn by one launch."""
        img = self._frame(img)[None]
        dev = img.device
        _, _, H, W = img.shape
        P = 3 if use_seg else 2
        canvas = torch.empty(1, H, P * W, 3, dtype=torch.uint8, device=dev)
        ops.image_to_u8(img, unit_range=True, out=canvas[:, :, :W])
        canvas[:, :, W:2 * W] = canvas[:, :, :W]
        if use_seg:
            seg = self._map(seg, dev)
            black = torch.zeros(1, 3, H, W, dtype=torch.uint8, device=dev)
            ops.overlay(black, labels=seg, lut=self._table("Set2", 2 if seg.dtype == torch.bool else 100, dev), alpha=1.0, unit_range=False,
                        out=canvas[:, :, 2 * W:])
        table = self._graph_result_table(colormap, dev)
        y = (self._dev(graph.y, dev).float() / 1.0 * 255).to(torch.uint8)
        y_pred = (self._dev(res, dev).detach().float().clip(0, 1.0) / 1.0 * 255).to(torch.uint8)
        c_y, c_pred = table[y.long()].reshape(1, -1, 3), table[y_pred.long()].reshape(1, -1, 3)
        center = self._dev(center, dev).reshape(1, -1, 2)
        lists = self._graph_list(self._dev(graph.edge_index, dev).long(), center, [c_pred, c_y] + ([c_y] if use_seg else []), (255, 0, 0))
        self._draw(canvas, *lists, panel_width=W)
        return self._result(canvas[0], kwargs)

    def _flow_canvas(self, img1, img2):
        """[plot_image(img1) | plot_image(img2)] as one panel, and the width of the second frame."""
        img1, img2 = self._frame(img1), self._frame(img2)
        if img1.shape[1] != img2.shape[1]:
            raise WvnError(f"the two frames of a flow plot share a height, got {tuple(img1.shape)} and {tuple(img2.shape)}")
        H, W1, W2 = img1.shape[1], img1.shape[2], img2.shape[2]
        canvas = torch.empty(1, H, W1 + W2, 3, dtype=torch.uint8, device=img1.device)
        ops.image_to_u8(img1, out=canvas[:, :, :W1])
        ops.image_to_u8(img2, out=canvas[:, :, W1:])
        return canvas, W2

    def _flow_lines(self, canvas, points):
        n, dev = points.shape[0], canvas.device
        green = torch.tensor((0, 255, 0), dtype=torch.uint8, device=dev).expand(n, 3)
        zeros = torch.zeros(n, dtype=torch.int32, device=dev)
        return self._draw(canvas, torch.full((n,), ops._lib.DRAW_LINE2, dtype=torch.int32, device=dev), points, green, zeros, zeros)

    @image_functionality
    def plot_optical_flow(self, flow, img1, img2, s=10, **kwargs):
        """Both frames side by side and, for every s-th pixel (v, u), a green 2-pixel line to (v + flow[1, u, v] + W, u + flow[0, u, v]).
        The sample positions are generated on the device."""
        canvas, W2 = self._flow_canvas(img1, img2)
        dev = canvas.device
        flow = self._dev(flow, dev)
        u = (torch.arange(int(flow.shape[1] / s), dtype=torch.float64, device=dev) * s).trunc().long()   # int(k * s)
        v = (torch.arange(int(flow.shape[2] / s), dtype=torch.float64, device=dev) * s).trunc().long()
        uu, vv = (t.reshape(-1) for t in torch.meshgrid(u, v, indexing="ij"))
        du = flow[0, uu, vv].float().double()
        dv = (flow[1, uu, vv].float() + W2).double()   # the reference adds the width in fp32, the sample position in double
        # a double sum goes into the fp32 record as its own truncation (exact below 2^24; anything else is skipped either way)
        ends = [torch.where(t.abs() < 2.0 ** 24, t.trunc(), t).float() for t in (vv.double() + dv, uu.double() + du)]
        self._flow_lines(canvas, torch.stack([vv.float(), uu.float()] + ends, dim=1))
        return self._result(canvas[0], kwargs)

    @image_functionality
    def plot_sparse_optical_flow(self, pre_pos, cur_pos, img1, img2, **kwargs):
        """Both frames side by side and a green 2-pixel line from every (p0, p1) to (W + c0, c1)."""
        canvas, W2 = self._flow_canvas(img1, img2)
        pre, cur = self._dev(pre_pos, canvas.device).float().reshape(-1, 2), self._dev(cur_pos, canvas.device).float().reshape(-1, 2)
        self._flow_lines(canvas, torch.stack([pre[:, 0], pre[:, 1], W2 + cur[:, 0], cur[:, 1]], dim=1))
        return self._result(canvas[0], kwargs)

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
