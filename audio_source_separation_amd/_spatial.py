"""What the closed-form spatial functions share (bss/beamform.py, transform/pca.py,
algorithm/minimum_distortion_principle.py): the argument checks, which raise ValueError before a device is touched, the
engine cache and the NumPy / tensor front door.  float64, one utterance; nothing here computes.
"""
import numpy as np

from ._device import Precision, to_device, to_numpy, torch

_ENGINES = {}


def engine(device):
    from .ops import Engine
    key = str(device)
    if key not in _ENGINES:
        _ENGINES[key] = Engine(dtype="float64", device=device)
    return _ENGINES[key]


def is_tensor(a):
    return isinstance(a, torch.Tensor)


def shape(a):
    return tuple(int(d) for d in (a.shape if is_tensor(a) else np.shape(a)))


def is_complex(a):
    return a.is_complex() if is_tensor(a) else np.iscomplexobj(a)


def check_dtype(what, dtype):
    if Precision(dtype).name != "float64":
        raise ValueError("%s: float64 only, got dtype=%r" % (what, dtype))


def check_signal(what, name, a, lo, hi=8):
    """`a` is a complex (channels, n_bins, n_frames) array with lo <= channels <= hi and no empty axis."""
    s = shape(a)
    if len(s) != 3:
        raise ValueError("%s: %s must be one utterance (n_channels, n_bins, n_frames), got shape %s" % (what, name, s))
    if not is_complex(a):
        raise ValueError("%s: %s must be complex" % (what, name))
    if not lo <= s[0] <= hi:
        raise ValueError("%s: n_channels of %s must be in [%d, %d], got %d" % (what, name, lo, hi, s[0]))
    if s[1] < 1 or s[2] < 1:
        raise ValueError("%s: %s is empty, shape %s" % (what, name, s))
    if max(s[0], 1) * s[1] * s[2] >= 2 ** 28:
        raise ValueError("%s: %s must stay below 4 GiB in complex128" % (what, name))
    return s


def check_steering(what, input, steering_vector, covariance, reference_id):
    """(M, N, F, T) of a beamformer call whose shapes fit each other."""
    M, F, T = check_signal(what, "input", input, 2)
    a = shape(steering_vector)
    if len(a) != 3 or a[0] != F or a[1] != M:
        raise ValueError("%s: steering_vector must have shape (n_bins, n_channels, n_sources) = (%d, %d, n_sources), got %s"
                         % (what, F, M, a))
    if not 1 <= a[2] <= 8:
        raise ValueError("%s: n_sources must be in [1, 8], got %d" % (what, a[2]))
    if a[2] * F * T >= 2 ** 28:
        raise ValueError("%s: the output must stay below 4 GiB in complex128" % what)
    if covariance is not None and shape(covariance) != (F, M, M):
        raise ValueError("%s: covariance must have shape (n_bins, n_channels, n_channels) = %s, got %s"
                         % (what, (F, M, M), shape(covariance)))
    if isinstance(reference_id, bool) or not isinstance(reference_id, (int, np.integer)) or not 0 <= reference_id < M:
        raise ValueError("%s: reference_id must be an integer in [0, %d), got %r" % (what, M, reference_id))
    return M, a[2], F, T


def on_device(a, eng):
    return to_device(a, eng.prec.cplx, eng.dev)


def give_back(like, t, np_dtype=np.complex128):
    """A tensor for a tensor input, a NumPy array otherwise."""
    return t if is_tensor(like) else to_numpy(t, np_dtype)
