"""minimum_distortion_principle on MI355X -- drop-in for
`algorithm.minimum_distortion_principle.minimum_distortion_principle` of the reference
(src/algorithm/minimum_distortion_principle.py:3-31).  NumPy in, NumPy out; device tensors in, a device tensor out.  One
streaming pass over Y and the reference channels, reduced along t on the device (assx_mdp_scale).  float64, one
utterance, at most 8 sources and 8 reference channels.  The division is plain IEEE: a silent source bin gives NaN, as in
the reference.
"""
from .. import _spatial as sp

__all__ = ["minimum_distortion_principle"]


def minimum_distortion_principle(Y, reference, *, dtype='float64', device=None):
    """
    Args:
        Y: (n_sources, n_bins, n_frames)
        reference: (n_bins, n_frames) or (n_channels, n_bins, n_frames)
    Returns:
        scale: (n_sources, n_bins) or (n_channels, n_sources, n_bins)
    """
    what = "minimum_distortion_principle"
    n_dims = len(sp.shape(reference))
    if n_dims not in (2, 3):
        raise ValueError("reference.ndim is expected 2 or 3, but given {}.".format(n_dims))
    sp.check_dtype(what, dtype)
    _, F, T = sp.check_signal(what, "Y", Y, 1)
    ref3 = reference if n_dims == 3 else reference[None]
    r = sp.check_signal(what, "reference", ref3, 1)
    if r[1:] != (F, T):
        raise ValueError("%s: reference has (n_bins, n_frames) = %s, Y has %s" % (what, r[1:], (F, T)))
    eng = sp.engine(device)
    scale = eng.mdp_scale(sp.on_device(Y, eng), sp.on_device(ref3, eng))
    return sp.give_back(Y, scale[0] if n_dims == 2 else scale)
