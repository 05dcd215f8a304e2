"""TraversabilityGridMap and SmartCarrot: what the reference leaves to elevation_mapping_cupy (the ``sem_wvn_*_traversability`` image
subscribers with ``image_channel_fusions: exponential`` and the ``mask_elevation_semantics`` plugin of
wild_visual_navigation_anymal/config/elevation_mapping_cupy) and to wild_visual_navigation_ros/scripts/smart_carrot.py, on the three
kernels of csrc/grid_map.hip.  Every layer and every result lives on the device; nothing here reads one back.

Grid convention (smart_carrot.py:140-150): N = round(length / resolution) cells a side, axis 0 = map x, axis 1 = map y, cell (i, j)
centred at (cx + (i - N/2) r, cy + (j - N/2) r); a layer is fp32 [N,N] and NaN means unknown."""
import torch

from .. import _lib, ops


def layer_from_message(data, n_rows: int, n_cols: int) -> torch.Tensor:
    """The flattened ``data`` of one grid_map_msgs/GridMap layer -> [N,N] in the convention above: smart_carrot.py:106-107,
    ``np.reshape(data, (n_rows, n_cols))[::-1, ::-1].transpose()`` (plumbing; host or device tensors alike)."""
    t = torch.as_tensor(data)
    return t.reshape(n_rows, n_cols).flip(0, 1).t().contiguous()


def layer_to_message(layer) -> torch.Tensor:
    """The inverse, smart_carrot.py:164: ``layer[::-1, ::-1].transpose().ravel()``."""
    return torch.as_tensor(layer).flip(0, 1).t().reshape(-1)


class TraversabilityGridMap:
    def __init__(self, length: float = 8.0, resolution: float = 0.04, device="cuda",
                 layers=("visual_traversability", "visual_confidence"), alpha: float = 0.5, min_depth: float = 0.1, max_range=None,
                 occlusion_margin: float = 0.05, center=(0.0, 0.0)):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.WvnError(f"TraversabilityGridMap: device must be a GPU (got {self.device}); the HIP path has no CPU fallback")
        self.resolution = float(resolution)
        self.N = int(round(float(length) / self.resolution))
        if not (1 <= self.N <= _lib.GRID_MAX_N):
            raise _lib.WvnError(f"TraversabilityGridMap: {self.N} cells a side; 1 to {_lib.GRID_MAX_N}")
        self.layer_names = tuple(layers)
        if not (1 <= len(self.layer_names) <= _lib.GRID_MAX_CHANNELS):
            raise _lib.WvnError(f"TraversabilityGridMap: {len(self.layer_names)} image layers; 1 to {_lib.GRID_MAX_CHANNELS}")
        self.alpha, self.min_depth, self.max_range, self.occlusion_margin = float(alpha), float(min_depth), max_range, float(occlusion_margin)
        self.center = (float(center[0]), float(center[1]))
        self.semantics_threshold = 0.5
        nan = float("nan")
        self._layers = {name: torch.full((self.N, self.N), nan, dtype=torch.float32, device=self.device)
                        for name in ("elevation",) + self.layer_names + ("sdf",)}
        self.hits = torch.zeros(self.N, self.N, dtype=torch.int32, device=self.device)
        self.sdf_d2 = torch.zeros(self.N, self.N, dtype=torch.int32, device=self.device)

    # ---- layers ----
    def __getitem__(self, name: str) -> torch.Tensor:
        if name == "elevation_with_semantics":   # the mask_elevation_semantics plugin: elevation where the semantic layer says traversable
            t = self._layers[self.layer_names[0]]
            return torch.where(t >= self.semantics_threshold, self._layers["elevation"], torch.full_like(t, float("nan")))
        if name == "hits":
            return self.hits
        return self._layers[name]

    def __contains__(self, name: str) -> bool:
        return name in self._layers or name in ("elevation_with_semantics", "hits")

    def set_elevation(self, elevation: torch.Tensor) -> None:
        """The elevation layer from any source (fp32 [N,N] in the grid convention, NaN = unknown)."""
        if tuple(elevation.shape) != (self.N, self.N):
            raise _lib.WvnError(f"set_elevation: expected [{self.N},{self.N}], got {tuple(elevation.shape)}")
        self._layers["elevation"].copy_(elevation.to(self.device, torch.float32))

    def move_to(self, x: float, y: float) -> None:
        """Re-centre the map on (x, y) snapped to the cell raster: every layer is shifted by whole cells, vacated cells become NaN
        (hits 0).  Torch plumbing, no kernel."""
        r, N = self.resolution, self.N
        si, sj = int(round((float(x) - self.center[0]) / r)), int(round((float(y) - self.center[1]) / r))
        if si == 0 and sj == 0:
            return
        self.center = (self.center[0] + si * r, self.center[1] + sj * r)

        def shift(t, fill):
            out = torch.full_like(t, fill)
            if abs(si) < N and abs(sj) < N:   # new cell (i, j) is old cell (i + si, j + sj)
                out[max(-si, 0):N - max(si, 0), max(-sj, 0):N - max(sj, 0)] = t[max(si, 0):N - max(-si, 0), max(sj, 0):N - max(-sj, 0)]
            return out

        for name in self._layers:
            self._layers[name] = shift(self._layers[name], float("nan"))
        self.hits = shift(self.hits, 0)
        self.sdf_d2 = shift(self.sdf_d2, 0)

    # ---- kernel 1 ----
    def fuse_images(self, maps: torch.Tensor, intrinsics: torch.Tensor, pose_cam_in_world: torch.Tensor) -> None:
        """maps [B,C,H,W] (channel c -> image layer c), every camera of the callback in one launch, cameras applied in order."""
        ops.grid_fuse_images(maps, intrinsics, pose_cam_in_world, self._layers["elevation"], [self._layers[n] for n in self.layer_names],
                             self.hits, self.center, self.resolution, alpha=self.alpha, min_depth=self.min_depth,
                             max_range=self.max_range, occlusion_margin=self.occlusion_margin)

    def fuse_prediction(self, trav: torch.Tensor, conf, image_projector, pose_cam_in_world: torch.Tensor) -> None:
        """The outputs of FeatureExtractor.predict_per_pixel ([B,H,W] or [H,W] each; ``conf`` may be None for a one-layer map) with the
        ImageProjector of the camera(s): its scaled intrinsics are the ones the images were predicted at."""
        planes = [p if p.dim() == 3 else p[None] for p in ([trav] if conf is None else [trav, conf])]
        maps = torch.stack([p.to(torch.float32) for p in planes], dim=1)
        K = image_projector.camera.intrinsics
        B = maps.shape[0]
        pose = pose_cam_in_world if pose_cam_in_world.dim() == 3 else pose_cam_in_world[None]
        self.fuse_images(maps, K.expand(B, 4, 4) if K.shape[0] != B else K, pose)

    # ---- kernel 2 ----
    def sdf(self, layer: str = "visual_traversability", threshold: float = 0.5, unknown: str = "obstacle") -> torch.Tensor:
        """Signed distance (metres, positive = free) to the cells of ``layer`` below ``threshold``; also stored as layer "sdf"."""
        ops.grid_sdf(self._layers[layer], threshold, self.resolution, unknown, out=(self._layers["sdf"], self.sdf_d2))
        return self._layers["sdf"]


class CarrotGoal:
    """Device-resident result of SmartCarrot.goal: ``cell`` int32 [3] = (i, j, found), ``value`` fp32 [3] = (score, x, y), ``masked`` the
    masked score layer (or None).  The properties read from the device on demand."""

    def __init__(self, cell: torch.Tensor, value: torch.Tensor, masked):
        self.cell, self.value, self.masked = cell, value, masked

    @property
    def found(self) -> bool:
        return bool(self.cell[2].item())

    @property
    def index(self):
        i, j, _ = self.cell.tolist()
        return i, j

    @property
    def score(self) -> float:
        return self.value[0].item()

    @property
    def position(self):
        _, x, y = self.value.tolist()
        return x, y


class SmartCarrot:
    """smart_carrot.py's goal selection: the arg-max of sdf + distance force - centre force inside three discs ahead of the robot."""

    def __init__(self, distance_force_factor: float = 0.0, center_force_factor: float = 0.0, discs=ops.GRID_DEFAULT_DISCS, debug: bool = False):
        self.distance_force_factor, self.center_force_factor = float(distance_force_factor), float(center_force_factor)
        self.discs, self.debug = tuple(discs), bool(debug)

    def goal(self, grid_map: TraversabilityGridMap, yaw: float) -> CarrotGoal:
        """Uses the map's "sdf" and "elevation" layers (call ``grid_map.sdf`` first); ``debug`` also returns the masked score layer."""
        cell, value, masked = ops.grid_carrot(grid_map["sdf"], grid_map["elevation"], yaw, grid_map.center, grid_map.resolution,
                                              self.distance_force_factor, self.center_force_factor, self.discs, want_masked=self.debug)
        return CarrotGoal(cell, value, masked)
