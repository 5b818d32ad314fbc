"""Delay-and-sum, ML and MVDR beamformers on MI355X -- drop-ins for `bss.beamform` of the reference
(src/bss/beamform.py:5-139).  NumPy in, NumPy out; device tensors in, device tensors out.  The per-bin filter (a general
complex inverse for ML / MVDR), the plain covariance of MVDR and the one streaming pass that applies the filter run on
the device (assx_bf_ds_weights, assx_bf_ml_weights, assx_cov_accumulate, assx_bf_apply).  float64, one utterance,
2 <= n_channels <= 8, 1 <= n_sources <= 8; anything else is a ValueError before a device is touched.

Three deliberate deviations from the reference: `MVDRBeamformer.__call__` works (the reference's
passes `covariance=` to a function that does not take it and always raises TypeError): it calls `mvdr_beamform`, or
`ml_beamform` when a covariance is given; `MaxSNRBeamformer.__call__` raises NotImplementedError where the reference's
falls off its end and returns None; importing this module emits no "in progress" warning.
"""
import numpy as np

from .. import _lib
from .. import _spatial as sp

EPS = 1e-12

__all__ = ["delay_sum_beamform", "ml_beamform", "mvdr_beamform", "DelaySumBeamformer", "MVDRBeamformer",
           "MaxSNRBeamformer"]


def delay_sum_beamform(input, steering_vector, reference_id=0, *, dtype='float64', device=None):
    """
    Args:
        input (n_channels, n_bins, n_frames)
        steering_vector (n_bins, n_channels, n_sources)
    Returns:
        output (n_sources, n_bins, n_frames)
    """
    sp.check_dtype("delay_sum_beamform", dtype)
    sp.check_steering("delay_sum_beamform", input, steering_vector, None, reference_id)
    eng = sp.engine(device)
    Wf, s = eng.bf_ds_weights(sp.on_device(steering_vector, eng), int(reference_id))
    return sp.give_back(input, eng.bf_apply(sp.on_device(input, eng), Wf, s))


def _ml(what, eng, X, A, R, reference_id, eps):
    status = eng.new_status(1)
    Wf, s = eng.bf_ml_weights(A, R, int(reference_id), eps, status)
    Y = eng.bf_apply(X, Wf, s)
    if int(status.item()) & _lib.STATUS_SINGULAR:
        raise np.linalg.LinAlgError("Singular matrix")
    return Y


def ml_beamform(input, steering_vector, covariance, reference_id=0, eps=EPS, *, dtype='float64', device=None):
    """
    Args:
        input (n_channels, n_bins, n_frames)
        steering_vector (n_bins, n_channels, n_sources)
        covariance (n_bins, n_channels, n_channels); need not be Hermitian
    Returns:
        output (n_sources, n_bins, n_frames)
    """
    sp.check_dtype("ml_beamform", dtype)
    sp.check_steering("ml_beamform", input, steering_vector, covariance, reference_id)
    eng = sp.engine(device)
    Y = _ml("ml_beamform", eng, sp.on_device(input, eng), sp.on_device(steering_vector, eng),
            sp.on_device(covariance, eng), reference_id, float(eps))
    return sp.give_back(input, Y)


def mvdr_beamform(input, steering_vector, reference_id=0, eps=EPS, *, dtype='float64', device=None):
    """
    Args:
        input (n_channels, n_bins, n_frames)
        steering_vector (n_bins, n_channels, n_sources)
    Returns:
        output (n_sources, n_bins, n_frames)
    """
    sp.check_dtype("mvdr_beamform", dtype)
    M, _, F, _ = sp.check_steering("mvdr_beamform", input, steering_vector, None, reference_id)
    eng = sp.engine(device)
    X = sp.on_device(input, eng)
    R = eng.cov_accumulate(X.unsqueeze(0)).reshape(F, M, M)  # mean_t x x^H
    return sp.give_back(input, _ml("mvdr_beamform", eng, X, sp.on_device(steering_vector, eng), R, reference_id, float(eps)))


class _Steered:
    """The constructor arguments and the steering-vector check that the three classes share."""

    def _setup(self, steering_vector, reference_id, dtype, device):
        sp.check_dtype(type(self).__name__, dtype)
        self.steering_vector = steering_vector
        self.reference_id = reference_id
        self._dtype, self._device = dtype, device

    def _steering(self, steering_vector):
        if steering_vector is not None:
            self.steering_vector = steering_vector
        elif self.steering_vector is None:
            raise ValueError("Specify steering vector.")


class DelaySumBeamformer(_Steered):
    def __init__(self, steering_vector=None, reference_id=0, *, dtype='float64', device=None):
        """
        Args:
            steering_vector (n_bins, n_channels, n_sources)
            reference_id <int>
        """
        self._setup(steering_vector, reference_id, dtype, device)

    def __call__(self, input, steering_vector=None):
        """
        Args:
            input (n_channels, n_bins, n_frames)
            steering_vector (n_bins, n_channels, n_sources)
        Returns:
            output (n_sources, n_bins, n_frames)
        """
        self.input = input
        self._steering(steering_vector)
        output = delay_sum_beamform(input, self.steering_vector, reference_id=self.reference_id, dtype=self._dtype,
                                    device=self._device)
        self.estimation = output
        return output


class MVDRBeamformer(_Steered):
    def __init__(self, steering_vector, reference_id=0, eps=EPS, *, dtype='float64', device=None):
        self._setup(steering_vector, reference_id, dtype, device)
        self.eps = eps

    def __call__(self, input, steering_vector=None, covariance=None):
        """
        Args:
            input (n_channels, n_bins, n_frames)
            steering_vector (n_bins, n_channels, n_sources)
            covariance (n_bins, n_channels, n_channels) or None: the input's own mean_t x x^H
        Returns:
            output (n_sources, n_bins, n_frames)
        """
        self.input = input
        self._steering(steering_vector)
        kw = dict(reference_id=self.reference_id, eps=self.eps, dtype=self._dtype, device=self._device)
        if covariance is None:
            output = mvdr_beamform(input, self.steering_vector, **kw)
        else:
            output = ml_beamform(input, self.steering_vector, covariance, **kw)
        self.estimation = output
        return output


class MaxSNRBeamformer(_Steered):
    def __init__(self, steering_vector, reference_id=0, eps=EPS, *, dtype='float64', device=None):
        self._setup(steering_vector, reference_id, dtype, device)
        self.eps = eps

    def __call__(self, input, steering_vector=None):
        self._steering(steering_vector)
        raise NotImplementedError("MaxSNRBeamformer has no body in the reference (src/bss/beamform.py:128-138)")
