"""TraversabilityGridMap and SmartCarrot: what the reference leaves to elevation_mapping_cupy (the ``sem_wvn_*_traversability`` image
subscribers with ``image_channel_fusions: exponential`` and the ``mask_elevation_semantics`` plugin of
wild_visual_navigation_anymal/config/elevation_mapping_cupy) and to wild_visual_navigation_ros/scripts/smart_carrot.py, on the three
kernels of csrc/grid_map.hip, and the elevation layer itself from depth images and point clouds on the two kernels of
csrc/elevation.hip (add_depth / add_points).  Every layer and every result lives on the device; nothing here reads one back.

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
                 occlusion_margin: float = 0.05, center=(0.0, 0.0), time_variance: float = 1e-4, **elevation_params):
        """``elevation_params``: the noise and range parameters of add_points / add_depth under the names of the reference's
        anymal_parameters.yaml (ops.GRID_ELEVATION_DEFAULTS: sensor_noise_factor, mahalanobis_thresh, outlier_variance,
        min_valid_distance, max_height_range, ramped_height_range_a / _b / _c, initial_variance, max_variance, max_ray_length) and
        clear_margin, clear_min_rays for the ray clearing."""
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
        self.elevation_params = ops.grid_elevation_params(**elevation_params)
        self.time_variance = float(time_variance)
        self.initial_variance, self.max_variance = self.elevation_params.initial_variance, self.elevation_params.max_variance
        self._layers["variance"] = torch.full((self.N, self.N), self.initial_variance, dtype=torch.float32, device=self.device)
        self._elevation_workspace = None      # allocated by the first add_points / add_depth; the kernels leave it zero
        self._elevation_stats = torch.zeros(len(_lib.GRID_ELEVATION_STATS), dtype=torch.int32, device=self.device)

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

    def set_elevation(self, elevation: torch.Tensor, variance=None) -> None:
        """The elevation layer from any source (fp32 [N,N] in the grid convention, NaN = unknown).  The finite cells take ``variance``
        (default: initial_variance clamped to max_variance, i.e. no confidence in the supplied height), the others initial_variance."""
        if tuple(elevation.shape) != (self.N, self.N):
            raise _lib.WvnError(f"set_elevation: expected [{self.N},{self.N}], got {tuple(elevation.shape)}")
        self._layers["elevation"].copy_(elevation.to(self.device, torch.float32))
        known = min(self.initial_variance, self.max_variance) if variance is None else float(variance)
        e = self._layers["elevation"]
        v = self._layers["variance"]          # in place, like the elevation: a caller that holds gm["variance"] keeps seeing the layer
        v.fill_(self.initial_variance)
        v.masked_fill_(torch.isfinite(e), known)

    # ---- elevation from depth (csrc/elevation.hip) ----
    def _add(self, op, *source, **kw):
        if self._elevation_workspace is None:
            self._elevation_workspace = ops.grid_elevation_workspace(self.N, self.device)
        self._elevation_stats = op(*source, self._layers["elevation"], self._layers["variance"], [self._layers[n] for n in self.layer_names],
                                   self.hits, self.center, self.resolution, params=self.elevation_params,
                                   workspace=self._elevation_workspace, **kw)

    def add_points(self, points: torch.Tensor, pose_sensor_in_map: torch.Tensor, counts=None, z_ref=None, clear_rays: bool = False) -> None:
        """Fuse point clouds into the elevation and variance layers: points [B,Pmax,3] (or [P,3] with one [4,4] pose) fp32 in the sensor
        frames, ``counts`` [B] int32 on the GPU for padded clouds.  All sensors of the callback in two launches; every point is judged
        against the map as it was on entry, so the order of points and sensors does not matter.  ``z_ref``: the height the
        fixed-point sums are relative to (default: sensor 0's t_z, taken on the device); points further than 128 m from it in z are
        dropped.  ``clear_rays``: cells whose elevation contradicts a ray and that received no inlier become unknown."""
        if points.dim() == 2:
            points = points[None]
        pose = pose_sensor_in_map if pose_sensor_in_map.dim() == 3 else pose_sensor_in_map[None]
        self._add(ops.grid_elevation_points, points, pose, counts=counts, z_ref=z_ref, clear_rays=clear_rays)

    def add_depth(self, depth: torch.Tensor, intrinsics: torch.Tensor, pose_cam_in_world: torch.Tensor, z_ref=None,
                  clear_rays: bool = False) -> None:
        """The same from depth images [B,H,W] (or [H,W]), fp32 metres or uint16 millimetres (ROS 32FC1 / 16UC1; 0, NaN, inf: no
        point), with the scaled intrinsics [B,4,4] as for fuse_images.  The points are formed on load; no cloud is written."""
        if depth.dim() == 2:
            depth = depth[None]
        B = depth.shape[0]
        K = intrinsics if intrinsics.dim() == 3 else intrinsics[None]
        pose = pose_cam_in_world if pose_cam_in_world.dim() == 3 else pose_cam_in_world[None]
        self._add(ops.grid_elevation_depth, depth, K.expand(B, 4, 4) if K.shape[0] != B else K, pose, z_ref=z_ref, clear_rays=clear_rays)

    def update_variance(self) -> None:
        """elevation_mapping_cupy's update_variance: var = min(var + time_variance, max_variance) on the known cells (torch plumbing)."""
        v = self._layers["variance"]
        grown = torch.clamp(v + self.time_variance, max=self.max_variance)
        torch.where(torch.isfinite(self._layers["elevation"]), grown, v, out=v)      # in place: gm["variance"] stays the same tensor

    @property
    def elevation_stats(self) -> dict:
        """The points of the last add_points / add_depth by class (reads eight int32 from the device: on demand only)."""
        return dict(zip(_lib.GRID_ELEVATION_STATS, self._elevation_stats.tolist()))

    def move_to(self, x: float, y: float) -> None:
        """Re-centre the map on (x, y) snapped to the cell raster: every layer is shifted by whole cells, vacated cells become NaN
        (hits 0, variance initial_variance).  Torch plumbing, no kernel."""
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
            self._layers[name] = shift(self._layers[name], self.initial_variance if name == "variance" else float("nan"))
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
