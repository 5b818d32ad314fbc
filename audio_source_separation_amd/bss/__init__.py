"""Blind source separation classes (mirror of the reference's src/bss for the HIP hot path)."""

_EXPORTS = {"GaussIPSDTA": "ipsdta", "IPSDTAbase": "ipsdta", "tIPSDTA": "ipsdta",
            "GradIVAbase": "iva", "GradLaplaceIVA": "iva", "NaturalGradLaplaceIVA": "iva",
            "FDICAbase": "fdica", "GradFDICAbase": "fdica", "GradLaplaceFDICA": "fdica",
            "NaturalGradLaplaceFDICA": "fdica", "PDSBSSbase": "prox", "ProxLaplaceIVA": "iva",
            "DelaySumBeamformer": "beamform", "MVDRBeamformer": "beamform", "MaxSNRBeamformer": "beamform"}
__all__ = sorted(_EXPORTS)


def __getattr__(name):
    """`from audio_source_separation_amd.bss import GaussIPSDTA`: the module is imported on first use."""
    if name in _EXPORTS:
        from importlib import import_module
        return getattr(import_module("." + _EXPORTS[name], __name__), name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
