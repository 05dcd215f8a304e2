"""ConfidenceGenerator -- wild_visual_navigation/utils/confidence_generator.py:13-212, all four methods.

State = non-trainable parameters with the reference's names, dtypes and shapes, so ``state_dict()`` / the
``.tmp_state_dict.pt`` hand-off (wvn_learning_node.py:381-394) stay compatible:
  every method        mean [1], var [1,1], std [1]                                   fp32
  running_mean        running_n, running_sum, running_sum_of_squares [1]             fp64
  kalman_filter       _kalman_filter.{proc_model, proc_cov, control_model, meas_model, meas_cov, eye} [1,1]   fp32
  moving_average      a window of the last 5 steps' positives (not saved: empty after a load)
Inside ``TraversabilityEstimator.train`` the statistic is produced by the HIP training step (csrc/mlp_device.h) on a device copy
of this state; the methods here are the caller-facing API (quick_start.py:207-210) on small vectors.

``reset()`` (the reference raises TypeError for latest_measurement and moving_average): latest_measurement,
moving_average and kalman_filter reset mean / var / std (moving_average also empties its window); running_mean resets its
running sums only."""
from collections import deque

import torch

from .kalman_filter import KalmanFilter

METHODS = ("latest_measurement", "running_mean", "kalman_filter", "moving_average")
WINDOW = 5


class ConfidenceGenerator(torch.nn.Module):
    def __init__(self, std_factor, method="latest_measurement", log_enabled: bool = False, log_folder: str = "/tmp"):
        super().__init__()
        if method not in METHODS:
            raise ValueError(f"Unknown method {method!r} (one of {', '.join(METHODS)})")
        self.method = method
        self.std_factor = std_factor
        self.log_enabled = log_enabled
        self.log_folder = log_folder
        self.mean = torch.nn.Parameter(torch.zeros(1, dtype=torch.float32), requires_grad=False)
        self.var = torch.nn.Parameter(torch.ones((1, 1), dtype=torch.float32), requires_grad=False)
        self.std = torch.nn.Parameter(torch.ones(1, dtype=torch.float32), requires_grad=False)
        if method == "kalman_filter":
            self._kalman_filter = KalmanFilter(dim_state=1, dim_control=1, dim_meas=1)
            self._kalman_filter.init_process_model(proc_model=torch.eye(1) * 1, proc_cov=torch.eye(1) * 0.2)
            self._kalman_filter.init_meas_model(meas_model=torch.eye(1), meas_cov=torch.eye(1) * 1.0)
        elif method == "running_mean":
            for name in ("running_n", "running_sum", "running_sum_of_squares"):
                setattr(self, name, torch.nn.Parameter(torch.zeros(1, dtype=torch.float64), requires_grad=False))
        elif method == "moving_average":
            self.data_window = deque(maxlen=WINDOW)
        # bumped whenever the state changes here (update, reset, load): the HIP training step keeps a device copy of the state and
        # re-reads it when this differs from what it last read
        self._version = 0

    # ------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, x: torch.Tensor, x_positive: torch.Tensor, step: int = 0, log_step: bool = False):
        """Update the statistic with this step's positives and return the confidence of every row of ``x``."""
        self._version += 1
        if self.method == "running_mean":
            self.running_n += x_positive.numel()
            self.running_sum += x_positive.sum()
            self.running_sum_of_squares += (x_positive ** 2).sum()
            self.mean[0] = self.running_sum[0] / self.running_n
            self.var[0] = self.running_sum_of_squares / self.running_n - self.mean ** 2
            self.std[0] = torch.sqrt(self.var)
            if x.device != self.mean.device:
                return torch.zeros_like(x)
            return self._interval(x)
        if self.method == "kalman_filter":
            if x_positive.shape[0] != 0:
                mean, var = self._kalman_filter(self.mean, self.var, x_positive.mean())
                self.var[0, 0] = var[0, 0]
                self.mean[0] = mean[0]
            self.std[0] = torch.sqrt(self.var)[0, 0]
            conf = torch.exp(-(((x - self.mean) / (self.std * self.std_factor)) ** 2) * 0.5)
            conf[x < self.mean] = 1.0
            return conf.type(torch.float32)
        if self.method == "moving_average":
            self.data_window.append(x_positive)
            window = torch.cat(list(self.data_window), dim=0)
            self.mean[0] = window.mean()
            self.std[0] = window.std()
            xc = torch.clip(x, self.mean - 2 * self.std, self.mean + 2 * self.std)
            return ((xc - torch.min(xc)) / (torch.max(xc) - torch.min(xc))).type(torch.float32)
        self.mean[0] = x_positive.mean()
        self.std[0] = x_positive.std()
        return self.inference_without_update(x)

    def _interval(self, x: torch.Tensor) -> torch.Tensor:
        shifted = self.mean + self.std * self.std_factor
        lo = torch.where(torch.isnan(shifted - self.std), shifted - self.std, torch.clamp(shifted - self.std, min=0.0))
        hi = shifted + self.std
        xc = torch.minimum(torch.maximum(x, lo), hi)
        return (1 - ((xc - lo) / (hi - lo))).type(torch.float32)

    @torch.no_grad()
    def inference_without_update(self, x: torch.Tensor):
        """The same formula for every method (confidence_generator.py:182-193)."""
        if x.device != self.mean.device:
            return torch.zeros_like(x)
        return self._interval(x)

    def forward(self, x: torch.Tensor):
        return self.inference_without_update(x)

    def reset(self):
        with torch.no_grad():
            if self.method == "running_mean":
                self.running_n[0] = 0
                self.running_sum[0] = 0
                self.running_sum_of_squares[0] = 0
            else:
                self.mean[0] = 0
                self.var[0] = 1
                self.std[0] = 1
                if self.method == "moving_average":
                    self.data_window.clear()
        self._version += 1

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        if self.method == "moving_average":
            self.data_window.clear()
        self._version += 1

    def window_sums(self):
        """moving_average: the window as per-step (n, sum, sum of squares), oldest first (n as a Python int, the sums as fp64
        tensors on the parameters' device) -- what the device state of the training step keeps instead of the rows."""
        return [(int(t.numel()), t.detach().double().sum().to(self.mean.device),
                 (t.detach().double() ** 2).sum().to(self.mean.device)) for t in getattr(self, "data_window", ())]

    def get_dict(self):
        return {"mean": self.mean, "var": self.var, "std": self.std}
