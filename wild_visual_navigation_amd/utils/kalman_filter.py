"""KalmanFilter -- wild_visual_navigation/utils/kalman_filter.py, the linear filter the ``kalman_filter`` confidence method
keeps its statistic with.

The parameter names and shapes are the reference's (they appear in ``traversability_loss_state_dict`` as
``_confidence_generator._kalman_filter.*``).  Outlier rejection is not implemented: ConfidenceGenerator never enables it.
Inside ``TraversabilityEstimator.train`` the same scalar filter runs on the device (csrc/mlp_device.h, conf_post)."""
import torch
import torch.nn as nn


class KalmanFilter(nn.Module):
    def __init__(self, dim_state: int = 1, dim_control: int = 1, dim_meas: int = 1):
        super().__init__()
        self.dim_state, self.dim_control, self.dim_meas = dim_state, dim_control, dim_meas

        def p(t):
            return nn.Parameter(t, requires_grad=False)

        self.proc_model = p(torch.eye(dim_state))
        self.proc_cov = p(torch.eye(dim_state))
        self.control_model = p(torch.eye(dim_state, dim_control))
        self.meas_model = p(torch.eye(dim_meas, dim_state))
        self.meas_cov = p(torch.eye(dim_meas, dim_meas))
        self.eye = p(torch.eye(dim_state, dim_state))

    def init_process_model(self, proc_model=None, proc_cov=None, control_model=None):
        for name, t in (("proc_model", proc_model), ("proc_cov", proc_cov), ("control_model", control_model)):
            if t is not None:
                assert getattr(self, name).shape == t.shape, f"{name}: {tuple(t.shape)} != {tuple(getattr(self, name).shape)}"
                setattr(self, name, nn.Parameter(t, requires_grad=False))

    def init_meas_model(self, meas_model=None, meas_cov=None):
        for name, t in (("meas_model", meas_model), ("meas_cov", meas_cov)):
            if t is not None:
                assert getattr(self, name).shape == t.shape, f"{name}: {tuple(t.shape)} != {tuple(getattr(self, name).shape)}"
                setattr(self, name, nn.Parameter(t, requires_grad=False))

    def prediction(self, state, state_cov, control=None):
        F = self.proc_model
        state = F @ state if control is None else F @ state + self.control_model @ control
        return state, F @ state_cov @ F.t() + self.proc_cov

    def correction(self, state, state_cov, meas):
        H = self.meas_model
        innovation = meas - H @ state
        gain = state_cov @ H.t() @ (H @ state_cov @ H.t() + self.meas_cov).inverse()
        return state + gain @ innovation, (self.eye - gain @ H) @ state_cov

    def forward(self, state, state_cov, meas, control=None):
        state, state_cov = self.prediction(state, state_cov, control)
        return self.correction(state, state_cov, meas)
