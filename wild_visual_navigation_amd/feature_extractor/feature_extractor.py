"""FeatureExtractor -- same public surface as
wild_visual_navigation/feature_extractor/feature_extractor.py:19-398 (constructor, ``extract`` 5-tuple,
``compute_segments`` / ``compute_features`` / ``sparsify_features``, properties), re-designed for
MI355X: the ViT runs on MFMA kernels, and the per-segment features come from ONE fused
up-sample + segment-mean kernel pair that reads the 4.8 MB patch map instead of writing and
re-reading the 308 MB dense map (dino_interface.py:87-90 -> feature_extractor.py:390-396).
``extract_batch`` is the batched (B > 1) entry point with per-image semantics identical to B = 1.
"""
from typing import Optional, Tuple

import torch

from .. import _lib, ops
from .dino_interface import DinoInterface
from .segment_extractor import SegmentExtractor
from .stego_interface import StegoInterface
from .torchvision_interface import TorchVisionInterface


class FeatureExtractor:
    def __init__(self, device: str, segmentation_type: str = "slic", feature_type: str = "dino",
                 input_size: int = 448, **kwargs):
        if feature_type == "torchvision":   # refused before anything is moved to the GPU
            self._check_torchvision_args(device, segmentation_type, input_size, kwargs)
        self._device = torch.device(device)
        self._segmentation_type = segmentation_type
        self._feature_type = feature_type
        self._input_size = input_size
        self._stego_features_already_computed_in_segmentation = False
        self._tokens = None  # patch-resolution features of the frame(s) being processed
        # extract_batch's random segmentation: image b of a call draws from the key (random_seed, frame index + b) (ops.random_pixels)
        self._random_seed = int(kwargs.get("random_seed", 0))
        self._random_frame = 0   # frames drawn so far without an explicit frame_index
        self.segment_extractor = SegmentExtractor().to(self._device)
        precision = kwargs.get("precision", "mixed")   # the <= 1e-3 mode (the reference is fp32 end to end); "fp16" / "bf16" are opt-in speed paths

        if self._feature_type == "stego":
            self._feature_dim = 90
            self._extractor = StegoInterface(
                device=device, input_size=input_size,
                n_image_clusters=kwargs.get("n_image_clusters", 20),
                run_clustering=kwargs.get("run_clustering", True),
                run_crf=kwargs.get("run_crf", False),
                backbone_type=kwargs.get("backbone_type", "vit_small" if kwargs.get("model_path") is None else None),
                patch_size=kwargs.get("patch_size", 8), precision=precision,
                backbone_weights=kwargs.get("pretrained_weights"), head_weights=kwargs.get("head_weights"),
                probe_weights=kwargs.get("probe_weights"), model_path=kwargs.get("model_path"),
                max_chunk=kwargs.get("max_chunk", 16), flip_tta=kwargs.get("flip_tta", True),
                cluster_resolution=kwargs.get("cluster_resolution", "pixel"), kmeans_form=kwargs.get("kmeans_form", "linear"),
                allow_synthetic=kwargs.get("allow_synthetic", False), fuse_mlp=kwargs.get("fuse_mlp"), fuse_qkv=kwargs.get("fuse_qkv"), fuse_proj=kwargs.get("fuse_proj", True),
                pos_embed_rule=kwargs.get("pos_embed_rule", "dino"), code_align_corners=kwargs.get("code_align_corners", True),
                crf=kwargs.get("crf"), fuse_head=kwargs.get("fuse_head"),
            )
        elif "dino" in self._feature_type:
            self._feature_dim = 384  # the reference hard-codes 384 for any dino type (feature_extractor.py:56)
            self._extractor = DinoInterface(
                device=device, input_size=input_size, patch_size=kwargs.get("patch_size", 8),
                backbone=kwargs.get("backbone", "dinov2" if self._feature_type == "dinov2" else "dino"),
                backbone_type=kwargs.get("backbone_type", "vit_small"),
                pretrained_weights=kwargs.get("pretrained_weights"), precision=precision,
                max_chunk=kwargs.get("max_chunk", 16), allow_synthetic=kwargs.get("allow_synthetic", False),
                fuse_mlp=kwargs.get("fuse_mlp"), fuse_qkv=kwargs.get("fuse_qkv"), fuse_proj=kwargs.get("fuse_proj", True),
                pos_embed_rule=kwargs.get("pos_embed_rule", "dino"),
            )
            self._feature_dim = self._extractor.feature_dim
        elif self._feature_type == "sift":
            # dense SIFT (csrc/dense_sift.hip): no backbone, no weights.  The reference sets 128 here (feature_extractor.py:65-67) but its
            # compute_sift concatenates the three colour channels' 128-d maps (:276-286): 384 is the width the features really have
            self._feature_dim = 3 * ops.DENSE_SIFT_DIM
            self._extractor = None
        elif self._feature_type == "torchvision":
            # the CNN baseline of the paper's ablation (slic100_resnet18.yaml): ResNet-18 stage maps pooled per segment at four scales
            # (csrc/resnet.hip, csrc/pyramid_pool.hip).  The reference leaves feature_dim unset; 64 + 128 + 256 + 512 is what it yields
            self._feature_dim = ops.PYRAMID_DIM
            self._extractor = TorchVisionInterface(
                device=device, model_type=kwargs.get("model_type", "resnet18"), input_size=input_size,
                pretrained=kwargs.get("pretrained", True), pretrained_weights=kwargs.get("pretrained_weights"),
                allow_synthetic=kwargs.get("allow_synthetic", False))
        elif self._feature_type == "none":
            self._extractor = None
        else:
            # the histogram ablation extractor raises NotImplementedError in the reference itself
            raise TypeError(f"Extractor[{self._feature_type}] not supported!")

        if self.segmentation_type == "slic":
            # The reference round-trips through the CPU package fast_slic (feature_extractor.py:84-90, 221-225); here SLIC runs on
            # the GPU in integer arithmetic (csrc/slic.hip; parity with fast_slic's own variant is unpinned)
            self._slic_num_components = kwargs.get("slic_num_components", 100)
            self._slic_compactness = kwargs.get("slic_compactness", 10)
            # fast_slic's Slic(...) enforces connectivity by default; here it is an opt-in pass after the k-means (csrc/slic_connectivity.hip):
            # off, the labels are the k-means result as before
            self._slic_enforce_connectivity = bool(kwargs.get("slic_enforce_connectivity", False))
            self._slic_min_size_factor = float(kwargs.get("slic_min_size_factor", 0.25))
        elif self.segmentation_type == "stego" and self._feature_type != "stego":
            raise TypeError("segmentation_type 'stego' requires feature_type 'stego' (as in the reference)")

    # ------------------------------------------------------------------------------------------ props
    @property
    def feature_type(self):
        return self._feature_type

    @property
    def feature_dim(self):
        return self._feature_dim

    @property
    def segmentation_type(self):
        return self._segmentation_type

    def change_device(self, device):
        """feature_extractor.py:130-139: move every member to ``device`` (another GPU)."""
        self._device = torch.device(device)
        self.segment_extractor = self.segment_extractor.to(self._device)
        if self._extractor is not None:
            self._extractor.change_device(device)

    def decode(self, frames, rectify=None, **kwargs) -> torch.Tensor:
        """Compressed camera frames (JPEG bytes, or a list of them, all of one size and sampling) -> uint8 [B,3,H,W] on the
        extractor's device: ops.jpeg_decode with strict=True.  ``fe.predict_and_extract(fe.decode(msgs), model, cg)`` is the whole
        image callback of a node that subscribes to a .../compressed topic.  ``rectify``: a RectifyMap (ops.rectify_map) -- the
        decoded frames are undistorted, [B,3,h,w] at the map's output size."""
        kwargs.setdefault("strict", True)
        rgb = ops.jpeg_decode(frames, self._device, **kwargs)[0]
        return rgb if rectify is None else ops.rectify(rgb, rectify, "planar")

    def decode_raw(self, frames, encoding: str, height: int, width: int, step=None, rectify=None) -> torch.Tensor:
        """Raw camera frames of ONE camera (``msg.data`` of sensor_msgs/Image messages, or a list of them; ``encoding``, ``height``,
        ``width``, ``step`` are the messages' fields) -> uint8 [B,3,H,W] RGB on the extractor's device: one upload, one launch
        (mono8, rgb8, bgr8, bayer_*8; utils.image_to_torch is the single-message form).  ``rectify``: a RectifyMap -- [B,3,h,w],
        demosaiced and undistorted in that launch.  ``fe.predict_and_extract(fe.decode_raw(msgs, "bayer_gbrg8", 1080, 1440,
        rectify=m), model, cg)`` is the whole image callback for the camera driver's own topic."""
        from ..utils.image_io import check_raw_geometry

        step = check_raw_geometry(encoding, height, width, step, rectify, "decode_raw")
        raw = ops.upload_raw_frames(frames, height * step, self._device, "decode_raw").view(-1, height, step)
        if rectify is None:
            return ops.unpack_frames(raw, encoding, step=step, width=width, channels=3)
        return ops.rectify(raw, rectify, encoding, step=step, width=width, channels=3)

    # ------------------------------------------------------------------------------------------ extract
    @torch.no_grad()
    def extract(self, img: torch.Tensor, **kwargs):
        """feature_extractor.py:95-128.  img [1,3,H,W] fp32 in [0,1], or the raw uint8 frame (then x/255 is fused into
        the backbone's patch gather: same features, a quarter of the upload).
        Returns (edges [2,E] i64, feat [S,D] f32, seg [H,W] i64, center [S,2] f32, dense [1,D,H,H] | None)."""
        if self._feature_type == "torchvision":
            self._extractor.check_frames(img, "extract")
        img = img.to(self._device)
        want_dense = kwargs.get("return_dense_features", False)
        if self._feature_type == "sift":
            return self._extract_sift(img, want_dense, **kwargs)
        if self._feature_type == "torchvision":
            return self._extract_pyramid(img, want_dense, **kwargs)
        if self._segmentation_type == "random":
            tokens = self._feature_tokens(img)
            H, W = img.shape[2:]
            nr = kwargs.get("n_random_pixels", 100)
            seg = torch.full((H * W,), -1, dtype=torch.long, device=self._device)
            indices = torch.randperm(H * W, device=self._device)[:nr]
            seg[indices] = torch.arange(0, nr, device=self._device)
            seg = seg.reshape(H, W)
            # a one-pixel segment's "mean" is the interpolated feature at that pixel
            feat = ops.segpool_bilinear_mean(seg[None], tokens, self._grid(), nr)[0]
            dense = ops.upsample_bilinear(tokens, self._grid(), H) if want_dense else None
            return None, feat, seg, None, dense

        edges, seg, center = self.compute_segments(img, **kwargs)
        tokens = self._feature_tokens(img)
        n_seg = center.shape[0]
        feat = ops.segpool_bilinear_mean(seg[None], tokens, self._grid(), n_seg)[0]
        dense = ops.upsample_bilinear(tokens, self._grid(), img.shape[2]) if want_dense else None
        return edges, feat, seg, center, dense

    @torch.no_grad()
    def backbone_stage(self, img: torch.Tensor) -> torch.Tensor:
        """First stage of ``extract_batch`` on its own: the ViT (and, for stego features, the STEGO head) -> the
        patch-resolution feature tokens [B, G*G, D].  Everything after it (clustering, pooling, the MLP step) consists of
        small kernels that do not fill the GPU; a throughput pipeline runs this stage for batch i+1 on one HIP stream while
        the rest of batch i runs on another (``extract_batch(img, backbone_out=...)``, bench.py)."""
        self._refuse_sift("backbone_stage")
        self._refuse_pyramid("backbone_stage")
        img = img.to(self._device)
        if self._feature_type == "stego":
            return self._extractor.code_tokens(img)
        return self._extractor.inference_tokens(img)

    def _refuse_sift(self, who):
        """Dense SIFT has no patch tokens: the per-pixel kernels interpolate patch-resolution features through a window of at most
        4 x 4 tokens (csrc/pixel_mlp.hip), and a pixel-resolution map does not fit that scheme.  Refused before any GPU work."""
        if self._feature_type == "sift":
            raise _lib.WvnError(f"{who}: feature_type 'sift' has no patch-token stage (its features are computed at pixel resolution); "
                                f"use predict_per_segment")

    @staticmethod
    def _check_torchvision_args(device, segmentation_type, input_size, kwargs):
        """What feature_type "torchvision" does not serve, each refusal naming its argument (TorchVisionInterface refuses model_type and
        input_size the same way; they are repeated here so that nothing is moved to the GPU first)."""
        model_type = kwargs.get("model_type", "resnet18")
        if model_type != "resnet18":
            raise _lib.WvnError(f"feature_type 'torchvision': model_type '{model_type}' is not supported: only 'resnet18' (resnet50, "
                                f"resnet50_dino and the EfficientNets need bottleneck or depthwise blocks)")
        if not isinstance(input_size, int) or input_size < 32 or input_size % 32:
            raise _lib.WvnError(f"feature_type 'torchvision': input_size={input_size} must be a positive multiple of 32")
        if segmentation_type not in ("grid", "slic"):
            raise _lib.WvnError(f"feature_type 'torchvision': segmentation_type '{segmentation_type}' is not supported: the multi-scale "
                                f"pooling needs segments ('grid' or 'slic'), not 'random', 'stego' or 'none'")
        if torch.device(device).type != "cuda":
            raise _lib.WvnError(f"feature_type 'torchvision': device '{device}' is not a GPU; the HIP path has no CPU fallback")

    def _refuse_pyramid(self, who):
        """The ResNet-18 pyramid has four maps at four resolutions, not one patch-token map: the token stage and the per-pixel kernels
        built on it do not apply.  Refused before any GPU work."""
        if self._feature_type == "torchvision":
            raise _lib.WvnError(f"{who}: feature_type 'torchvision' has no patch-token stage (its features are four maps at strides 4 to "
                                f"32, pooled per segment); use predict_per_segment")

    def _pyramid_dense(self):
        """The reference's dict of dense maps (NCHW copies of the level maps of the last forward pass)."""
        return {f"feat{i + 1}": m.permute(0, 3, 1, 2).contiguous() for i, m in enumerate(self._extractor._levels)}

    def _extract_pyramid(self, img, want_dense, **kwargs):
        """``extract`` for feature_type "torchvision": feat [S,960] from the pooling kernel on the level maps in the workspace; the dict
        of dense maps is built only on request."""
        edges, seg, center = self.compute_segments(img, **kwargs)
        n_seg = center.shape[0]
        levels = self._extractor.forward_levels(img)
        feat = ops.segpool_pyramid(levels, seg[None], n_seg)[0]
        return edges, feat, seg, center, (self._pyramid_dense() if want_dense else None)

    def _extract_batch_pyramid(self, img, **kwargs):
        """``extract_batch`` for feature_type "torchvision" (grid or slic segmentation): feat [B,S,960]."""
        B, _, H, W = img.shape
        if self._segmentation_type == "grid":
            cell = kwargs.get("cell_size", 32)
            seg = self.segment_grid(img, **kwargs)[0, 0].to(torch.int32)[None].expand(B, H, W).contiguous()
            n_seg = (H // cell) * (W // cell)
        else:
            seg = ops.slic(img, self._slic_num_components, self._slic_compactness, enforce_connectivity=self._slic_enforce_connectivity,
                           min_size_factor=self._slic_min_size_factor)
            n_seg = ops.slic_num_clusters(H, W, self._slic_num_components)
        feat = ops.segpool_pyramid(self._extractor.forward_levels(img), seg, n_seg)
        return feat, seg, torch.full((B,), n_seg, dtype=torch.int32, device=self._device)

    def _extract_sift(self, img, want_dense, **kwargs):
        """``extract`` for feature_type "sift": the segment map as for every other feature type, feat from the fused descriptor +
        segment-mean kernel (the [1,384,H,W] map is built only on request)."""
        if self._segmentation_type == "random":
            edges, center = None, None
            seg = self.segment_random(img, **kwargs)[0, 0]
            n_seg = kwargs.get("n_random_pixels", 100)
        else:
            edges, seg, center = self.compute_segments(img, **kwargs)
            n_seg = center.shape[0]
        feat = ops.dense_sift_segpool(img, seg[None], n_seg)[0]
        return edges, feat, seg, center, (ops.dense_sift(img) if want_dense else None)

    def _extract_batch_sift(self, img, **kwargs):
        """``extract_batch`` for feature_type "sift" (grid, slic or random segmentation; H x W frames): the same segment maps as for
        the ViT features, feat [B,S,384] from ops.dense_sift_segpool.  Random: the -1 / id map of ops.random_pixels goes through the
        same kernel, which skips every tile without a sample."""
        B, _, H, W = img.shape
        if self._segmentation_type == "grid":
            cell = kwargs.get("cell_size", 32)
            seg = self.segment_grid(img, **kwargs)[0, 0].to(torch.int32)[None].expand(B, H, W).contiguous()
            n_seg = (H // cell) * (W // cell)
        elif self._segmentation_type == "slic":
            seg = ops.slic(img, self._slic_num_components, self._slic_compactness, enforce_connectivity=self._slic_enforce_connectivity,
                           min_size_factor=self._slic_min_size_factor)
            n_seg = ops.slic_num_clusters(H, W, self._slic_num_components)
        elif self._segmentation_type == "random":
            n_seg = kwargs.get("n_random_pixels", 100)
            frame = kwargs.get("frame_index")
            if frame is None:
                frame = self._random_frame
                self._random_frame = (frame + B) & 0xFFFFFFFF
            _, seg = ops.random_pixels(B, H, W, n_seg, seed=self._random_seed, frame0=frame, device=self._device)
        else:
            raise TypeError(f"extract_batch: segmentation_type [{self._segmentation_type}] not supported with feature_type 'sift'")
        feat = ops.dense_sift_segpool(img, seg, n_seg)
        return feat, seg, torch.full((B,), n_seg, dtype=torch.int32, device=self._device)

    @torch.no_grad()
    def extract_batch(self, img: torch.Tensor, backbone_out: Optional[torch.Tensor] = None,
                      **kwargs) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Batched hot path (no graph structure): img [B,3,H,H] -> (feat [B,S,D], seg [B,H,H] int32,
        n_segments [B] int32).  Rows of ids that do not occur in an image are NaN (the reference's empty
        mean).  Supported segmentations: grid, slic, stego, random.  Random (``n_random_pixels=100``, ``frame_index=None``): image b
        draws n_random_pixels distinct pixels from the key (``random_seed`` of the constructor, frame_index + b), so a frame index reproduces
        its draw whatever the batching; ``frame_index=None`` counts the frames of the calls so far.  seg is -1 off the samples, sample j carries
        id j, feat[b, j] is the interpolated feature at that pixel (ops.random_pixels, ops.gather_bilinear: no permutation of the frame, no
        pooling pass, no host synchronisation; the single-frame ``extract`` keeps its torch.randperm draw).  SLIC with ``slic_enforce_connectivity=True`` adds one batched
        connectivity pass over the B maps (ops.slic_enforce_connectivity: fragments below slic_min_size_factor of a superpixel go to a
        neighbour; ids stay cluster ids, emptied ids give NaN rows); the pass has no host synchronisation.  ``backbone_out``: the tokens ``backbone_stage(img)`` returned.
        feature_type "sift": grid, slic or random segmentation on H x W frames, feat [B,S,384] from the fused descriptor + segment-mean kernel
        (``_extract_batch_sift``); there is no backbone stage, so ``backbone_out`` is refused.
        feature_type "torchvision": grid or slic segmentation on input_size x input_size frames, feat [B,S,960] from the ResNet-18 level
        maps and the pyramid pooling kernel (``_extract_batch_pyramid``); ``backbone_out`` is refused."""
        if self._feature_type == "torchvision":
            if backbone_out is not None:
                self._refuse_pyramid("extract_batch(backbone_out=...)")
            self._extractor.check_frames(img, "extract_batch")
        img = img.to(self._device)
        if self._feature_type == "sift":
            if backbone_out is not None:
                self._refuse_sift("extract_batch(backbone_out=...)")
            return self._extract_batch_sift(img, **kwargs)
        if self._feature_type == "torchvision":
            return self._extract_batch_pyramid(img, **kwargs)
        B, _, H, W = img.shape
        G = self._grid()
        labels_patch = None  # [B,G,G] ids when the segment map is constant on every ViT patch
        if self._segmentation_type == "grid":
            cell = kwargs.get("cell_size", 32)
            seg = self.segment_grid(img, **kwargs)[0, 0].to(torch.int32)[None].expand(B, H, W).contiguous()
            n_seg = (H // cell) * (W // cell)
            nseg = torch.full((B,), n_seg, dtype=torch.int32, device=self._device)
            tokens = backbone_out if backbone_out is not None else self._feature_tokens(img)
            P = H // G
            if H == W and G * P == H and cell % P == 0:
                labels_patch = seg[:, ::P, ::P]
        elif self._segmentation_type == "stego":
            if backbone_out is not None and self._feature_type != "stego":
                raise _lib.WvnError("extract_batch: backbone_out with stego segmentation needs feature_type='stego'")
            self._extractor.inference(img, code=backbone_out)
            seg = self._extractor.cluster_segments[0]
            nseg = self._extractor._n_segments
            if nseg is None:
                raise _lib.WvnError("extract_batch with stego segmentation needs run_clustering=True (per-image k-means)")
            n_seg = self._extractor._cfg.n_image_clusters
            tokens = self._extractor.feature_tokens
            labels_patch = self._extractor._labels_patch
        elif self._segmentation_type == "slic":
            seg = ops.slic(img, self._slic_num_components, self._slic_compactness, enforce_connectivity=self._slic_enforce_connectivity,
                           min_size_factor=self._slic_min_size_factor)   # (the enforcement is one batched call)
            n_seg = ops.slic_num_clusters(H, W, self._slic_num_components)
            nseg = torch.full((B,), n_seg, dtype=torch.int32, device=self._device)
            tokens = backbone_out if backbone_out is not None else self._feature_tokens(img)
        elif self._segmentation_type == "random":
            if H != W:
                raise _lib.WvnError(f"extract_batch: square frames only (the feature map is H x H); got H={H}, W={W}")
            nr = kwargs.get("n_random_pixels", 100)
            frame = kwargs.get("frame_index")
            if frame is None:
                frame = self._random_frame
                self._random_frame = (frame + B) & 0xFFFFFFFF
            idx, seg = ops.random_pixels(B, H, W, nr, seed=self._random_seed, frame0=frame, device=self._device)
            tokens = backbone_out if backbone_out is not None else self.backbone_stage(img)
            # a one-pixel segment's "mean" is the interpolated feature at that pixel (feature_extractor.py:96-111)
            return ops.gather_bilinear(tokens, idx, G, H), seg, torch.full((B,), nr, dtype=torch.int32, device=self._device)
        else:
            raise TypeError(f"extract_batch: segmentation_type [{self._segmentation_type}] not supported")
        feat = None
        if labels_patch is not None and kwargs.get("patch_aligned_pooling", True):
            feat = ops.segpool_patch_labels(labels_patch, tokens, G, H, n_seg)  # None if geometry does not allow
        if feat is None:
            feat = ops.segpool_bilinear_mean(seg, tokens, G, n_seg)
        return feat, seg, nseg

    # ------------------------------------------------------------------------------------------ pieces
    @torch.no_grad()
    def predict_per_pixel(self, img: torch.Tensor, model, confidence_generator=None, want_loss: bool = False):
        """The live node's per-frame prediction with ``prediction_per_pixel`` (wvn_feature_extractor_node.py:311-363;
        quick_start.py:176-210) in one call: img [B,3,H,W] (fp32 in [0,1] or uint8) -> (trav [B,H,H], conf [B,H,H],
        loss_reco | None).  Equivalent to ``extract(..., return_dense_features=True)`` -> ``model.forward(Data(x=dense
        rows))`` -> column 0 / ``confidence_generator.inference_without_update(mse(pred[:, 1:], x))``, but the dense
        [B,D,H,H] tensor is never built and layer 1 runs at patch resolution (csrc/pixel_mlp.hip).  DINO / DINOv2 ViT-S (384-d),
        ViT-Base (768-d: DINO ViT-B/8, DINOv2 ViT-B/14) or STEGO (90-d code) features; bf16 / fp8 / fp16 extractor -> bf16 MFMA
        kernel (fp16 tokens are rounded to bf16 once), fp32 (exact) extractor -> the hi + lo split form (<= 1e-3 of the reference).
        ``model.input_size`` must equal the extractor's ``feature_dim`` (WvnError otherwise).  Like the reference
        (dino_interface.py:87-90) the map is H x H for an H x W frame."""
        self._refuse_sift("predict_per_pixel")
        self._refuse_pyramid("predict_per_pixel")
        img = img.to(self._device)
        self._check_per_pixel_model(model, "predict_per_pixel")
        rows, _ = self._per_pixel_tokens(img, model)
        return self._per_pixel_maps(rows, model, img.shape[0], img.shape[2], *self._confidence_scalars(confidence_generator), want_loss)

    @torch.no_grad()
    def predict_and_extract(self, img: torch.Tensor, model, confidence_generator=None, want_loss: bool = False, **kwargs):
        """The live node's whole image callback with ``prediction_per_pixel`` (wvn_feature_extractor_node.py:305-393) from ONE backbone
        pass: img [B,3,H,H] -> (trav [B,H,H], conf [B,H,H], loss_reco | None, feat [B,S,D], seg [B,H,H] int32, nseg [B]), the tuple
        shape of ``predict_per_segment``.  The three maps are ``predict_per_pixel(img, model, confidence_generator, want_loss)``'s and
        feat / seg / nseg are ``extract_batch(img, **kwargs)``'s (the ImageFeatures training message), bit for bit; the tokens of the one
        ViT run (for stego features with flip TTA: of the one paired run, and its one STEGO head) feed both.  grid, slic, stego or random
        segmentation; dino, dinov2 or stego features; every precision.  SimpleMLP or LinearRnvp (trav = conf = confidence(-score), third map
        -score), anything else is refused before the backbone runs."""
        self._refuse_sift("predict_and_extract")
        self._refuse_pyramid("predict_and_extract")
        img = img.to(self._device)
        self._check_per_pixel_model(model, "predict_and_extract")
        rows, tokens = self._per_pixel_tokens(img, model)
        trav, conf, loss = self._per_pixel_maps(rows, model, img.shape[0], img.shape[2], *self._confidence_scalars(confidence_generator),
                                                want_loss)
        feat, seg, nseg = self.extract_batch(img, backbone_out=tokens, **kwargs)
        return trav, conf, loss, feat, seg, nseg

    @staticmethod
    def _confidence_scalars(confidence_generator):
        if confidence_generator is None:
            return 0.0, 1.0, 0.5
        return float(confidence_generator.mean), float(confidence_generator.std), float(confidence_generator.std_factor)

    def _check_per_pixel_model(self, model, who):
        """What the fused per-pixel kernel cannot serve is refused before the backbone runs."""
        if not hasattr(model, "ZX_COLS") and not self._flow_model(model):
            raise _lib.WvnError(f"{who}: fused per-pixel inference is not implemented for {type(model).__name__} "
                                f"(SimpleMLP and LinearRnvp only); use predict_per_segment")
        if self.feature_dim != model.input_size:
            raise _lib.WvnError(f"{who}: the extractor's feature_dim is {self.feature_dim}, the model's input_size is "
                                f"{model.input_size}")

    def _exact(self) -> bool:
        return self._extractor._precision in ("exact", "fp32", "mixed")

    @staticmethod
    def _flow_model(model) -> bool:
        """LinearRnvp (anomaly detection): its per-pixel kernel (csrc/rnvp.hip) reads the fp32 tokens whatever the extractor's
        precision; trav = conf = confidence(-score), the third map is -score."""
        return getattr(model, "PER_PIXEL_FP32_TOKENS", False)

    def _per_pixel_tokens(self, img, model):
        """First half of the per-pixel prediction: the one backbone pass -> (rows, tokens).  ``rows`` is what ``_per_pixel_maps`` reads:
        the fp32 tokens themselves for an fp32 extractor, the bf16 zx rows [B*G*G, ZX_COLS] with the features from column X_COL
        otherwise.  ``tokens`` [B, G*G, D] fp32 is the same pass's ``backbone_stage(img)`` (for ``extract_batch(backbone_out=...)``)."""
        B, G = img.shape[0], self._grid()
        if self._exact() or self._flow_model(model):   # fp32 extractor: hi + lo split MFMA operands in the fused kernel
            tokens = self.backbone_stage(img)
            return tokens, tokens
        if self._feature_type == "stego":   # 90-d code (the live node's default feature_type), zero-padded to the 128 columns the layer-1 GEMM reads
            tokens = self._extractor.code_tokens(img)
            code = tokens.reshape(B * G * G, -1)
            zx = torch.zeros(B * G * G, model.ZX_COLS, dtype=torch.bfloat16, device=self._device)
            zx[:, model.X_COL: model.X_COL + code.shape[1]] = code
            return zx, tokens
        zx = torch.empty(B * G * G, model.ZX_COLS, dtype=torch.bfloat16, device=self._device)
        if self._extractor._model.lowp_dtype != torch.bfloat16:   # (fp16) the kernel takes bf16 features: the fp32 tokens rounded once
            tokens = self._extractor._model.forward_tokens(img)
            ops.cast_rows_bf16(tokens.reshape(B * G * G, -1), zx[:, model.X_COL:])
        else:   # the final LayerNorm writes its result twice: fp32 tokens, and bf16 straight into the zx rows
            tokens = self._extractor._model.forward_tokens(img, lowp_out=zx[:, model.X_COL:])
        return zx, tokens

    def _per_pixel_maps(self, rows, model, B, H, mean, std, f, want_loss):
        """Second half: the fused up-sample + MLP + confidence kernel on ``_per_pixel_tokens``' rows -> (trav, conf, loss_reco | None)."""
        G = self._grid()
        if self._exact() or self._flow_model(model):
            return model.forward_per_pixel_exact(rows.reshape(B * G * G, -1), B, G, (H, H), mean, std, f, want_loss=want_loss)
        return model.forward_per_pixel(rows, B, G, (H, H), mean, std, f, want_loss=want_loss)

    @torch.no_grad()
    def predict_per_segment(self, img: torch.Tensor, model, confidence_generator=None, want_loss: bool = False,
                            backbone_out: Optional[torch.Tensor] = None, **kwargs):
        """The live node's per-frame prediction WITHOUT ``prediction_per_pixel`` (wvn_feature_extractor_node.py:320-366;
        quick_start.py:184-210) for a batch: img [B,3,H,W] -> (trav [B,H,W], conf [B,H,W], loss_reco | None, feat [B,S,D],
        seg [B,H,W] int32, nseg [B]).  ``extract_batch(img, backbone_out, **kwargs)`` (grid, slic or stego segmentation), then
        ``model.forward_per_segment(feat, seg)``: equivalent to ``feat[seg.reshape(-1)]`` -> ``model.forward`` -> column 0 /
        ``confidence_generator.inference_without_update(mse(pred[:, 1:], x))`` per frame, with the MLP run once per segment
        (csrc/segment_predict.hip).  ``feat`` / ``seg`` / ``nseg`` are extract_batch's, for the training messages of the same pass.
        A confidence generator on the GPU is read from device memory: no host synchronisation beyond extract_batch's own.
        A model that declares ``NEEDS_GRAPH`` (SimpleGCN) also gets the segment graph of every frame, as the adjacency bitmaps
        ``ops.seg_adjacency_batched(seg, S)`` (grid, slic or stego segmentation; "random" samples have no graph and are refused
        before the backbone runs)."""
        graph = getattr(model, "NEEDS_GRAPH", False)
        if graph and self._segmentation_type == "random":
            raise _lib.WvnError(f"predict_per_segment: {type(model).__name__} needs the segment graph, and segmentation_type 'random' "
                                f"has none; use grid, slic or stego segmentation")
        feat, seg, nseg = self.extract_batch(img, backbone_out=backbone_out, **kwargs)
        mean, std, f, conf_state = 0.0, 1.0, 0.5, None
        if confidence_generator is not None:
            cg = confidence_generator
            if cg.mean.device == feat.device:
                conf_state = torch.cat([cg.mean.detach().reshape(1).float(), cg.std.detach().reshape(1).float(),
                                        torch.full((1,), float(cg.std_factor), dtype=torch.float32, device=feat.device)])
            else:
                mean, std, f = float(cg.mean), float(cg.std), float(cg.std_factor)
        extra = {"adjacency": ops.seg_adjacency_batched(seg, feat.shape[1])} if graph else {}
        trav, conf, loss = model.forward_per_segment(feat, seg, mean, std, f, want_loss=want_loss, conf_state=conf_state, **extra)
        return trav, conf, loss, feat, seg, nseg

    def _grid(self) -> int:
        return self._extractor.grid

    def _feature_tokens(self, img: torch.Tensor) -> torch.Tensor:
        """Patch-resolution features [B, G*G, D] of the configured feature type."""
        if self._feature_type == "stego":
            if self._stego_features_already_computed_in_segmentation:
                self._stego_features_already_computed_in_segmentation = False
                return self._extractor.feature_tokens
            self._extractor.inference(img.clone())
            return self._extractor.feature_tokens
        return self._extractor.inference_tokens(img)

    def compute_segments(self, img: torch.Tensor, **kwargs):
        """feature_extractor.py:151-177 -> (edges [2,E], seg [H,W] i64, centers [S,2])."""
        if self._segmentation_type == "none" or self._segmentation_type is None:
            edges, seg, centers = self.segment_pixelwise(img, **kwargs)
            return edges.T, seg[0, 0], centers
        if self._segmentation_type == "grid":
            seg = self.segment_grid(img, **kwargs)
        elif self._segmentation_type == "slic":
            seg = self.segment_slic(img, **kwargs)
        elif self._segmentation_type == "stego":
            seg = self.segment_stego(img, **kwargs)
        elif self._segmentation_type == "random":
            seg = self.segment_random(img, **kwargs)
        else:
            raise TypeError(f"segmentation_type [{self._segmentation_type}] not supported")
        edges = self.segment_extractor.adjacency_list(seg)
        centers = self.segment_extractor.centers(seg)
        return edges.T, seg[0, 0], centers

    def segment_pixelwise(self, img, **kwargs):
        B, C, H, W = img.shape
        seg = torch.arange(0, H * W, 1, device=self._device).reshape(H, W)
        ys, xs = torch.meshgrid(torch.arange(H, device=self._device), torch.arange(W, device=self._device),
                                indexing="ij")
        centers = torch.stack([ys.reshape(-1), xs.reshape(-1)], dim=1)
        hor = torch.stack([seg[:, :-1].reshape(-1), seg[:, 1:].reshape(-1)], dim=1)
        ver = torch.stack([seg[:-1, :].reshape(-1), seg[1:, :].reshape(-1)], dim=1)
        return torch.cat([hor, ver], dim=0), seg[None, None], centers

    def segment_grid(self, img, **kwargs):
        """feature_extractor.py:198-219: id = row-major index of the cell_size cell (index arithmetic only)."""
        cell = kwargs.get("cell_size", 32)
        H, W = img.shape[2:]
        gy = torch.arange(H, device=self._device) // cell
        gx = torch.arange(W, device=self._device) // cell
        return (gy[:, None] * (W // cell) + gx[None, :])[None, None].to(torch.int64)

    def segment_slic(self, img, **kwargs):
        """feature_extractor.py:221-225 without the host round trip: [1,3,H,W] (float in [0,1], truncated to 8 bits like the
        reference's np.uint8(img * 255), or uint8) -> [1,1,H,W] int64 ids in [0, number of SLIC clusters); with
        ``slic_enforce_connectivity=True`` after the connectivity pass (fast_slic's default post-processing)."""
        seg = ops.slic(img[0].to(self._device), self._slic_num_components, self._slic_compactness,
                       enforce_connectivity=self._slic_enforce_connectivity, min_size_factor=self._slic_min_size_factor)
        return seg[None, None].to(torch.long)

    def segment_random(self, img, **kwargs):
        H, W = img.shape[2:]
        nr = kwargs.get("n_random_pixels", 100)
        seg = torch.full((H * W,), -1, dtype=torch.long, device=self._device)
        indices = torch.randperm(H * W, device=self._device)[:nr]
        seg[indices] = torch.arange(0, nr, device=self._device)
        return seg.reshape(H, W)[None, None]

    def segment_stego(self, img, **kwargs):
        """feature_extractor.py:237-249; the ascending relabel is done inside the k-means kernel."""
        self._extractor.inference(img.clone())
        seg = self._extractor.cluster_segments.to(torch.long)  # [1,1,H,H]
        if self._extractor._n_segments is None:  # cluster-probe ids are not compacted: relabel ascending (:245-246)
            _, inv = torch.unique(seg, return_inverse=True)
            seg = inv.reshape(seg.shape)
        self._stego_features_already_computed_in_segmentation = True
        return seg

    @torch.no_grad()
    def compute_features(self, img: torch.Tensor, seg: torch.Tensor, center: torch.Tensor, **kwargs):
        """feature_extractor.py:251-274: dense per-pixel features [B,D,H,H] (materialised on request only)."""
        if self._feature_type == "none":
            return None
        if self._feature_type == "sift":   # feature_extractor.py:276-286: [B,384,H,W], the frame as it is (no resize, crop or normalisation)
            return ops.dense_sift(img.to(self._device))
        if self._feature_type == "torchvision":   # the dict feat1 .. feat4 of NCHW maps, as the reference's interface returns it
            return self._extractor.inference(img)
        if self._feature_type == "stego":
            if self._stego_features_already_computed_in_segmentation:
                self._stego_features_already_computed_in_segmentation = False
                return self._extractor.features
            self._extractor.inference(img.clone())
            return self._extractor.features
        return self._extractor.inference(img.clone())

    @torch.no_grad()
    def sparsify_features(self, dense_features: torch.Tensor, seg: torch.Tensor, cumsum_trick=False):
        """feature_extractor.py:310-398 (default branch) on an explicit dense map: identity resampling
        through the same segment-mean kernels (grid == image size)."""
        if self._feature_type in ["histogram"] or self._segmentation_type in ["none"]:
            return dense_features
        if isinstance(dense_features, dict):   # feature_extractor.py:314-366: the multi-scale branch (feat1 .. feat4, NCHW, one frame)
            levels = [dense_features[f"feat{i + 1}"].permute(0, 2, 3, 1).contiguous() for i in range(4)]
            return ops.segpool_pyramid(levels, seg[None], int(seg.max().item()) + 1)[0]
        _lib.require_cuda(dense_features, "dense_features")
        _, D, H, W = dense_features.shape
        if H != W:
            raise _lib.WvnError("sparsify_features expects the square [1,D,H,H] map DinoInterface produces")
        n_seg = int(seg.max().item()) + 1
        tokens = dense_features[0].permute(1, 2, 0).reshape(1, H * W, D).contiguous()
        return ops.segmean_tokens(seg[None], tokens, n_seg)[0]
