"""MI355X TDOA localizer -- Python host side over libtdoa.so.

    from tdoa import Localizer
    loc = Localizer()                       # reference config: 3 mics, 1024, 50 kHz
    out = loc.localize(frames_int16_cuda)   # lags, gate, cell, xy, max_L

See include/tdoa.h for the C ABI and DESIGN.md for the kernels.
"""
from ._lib import (ENGINE_DIRECT, ENGINE_GCC_PHAT, EXPORTED_SYMBOLS, LIB_PATH,  # noqa: F401
                   MAX_TRACKS, TRACK_DEFAULTS, TRACK_FIELDS, TdoaError, Track, TrackOutputs, TrackParams,
                   BeamGeometry, BeamOutputs, band_weights, beam_fir, beam_geometry, beam_host, beam_latency,
                   decay_us, dpss_q15, load, sep_check, sep_window, track_host, track_params,
                   SEP_LOADING, SEP_MAX_TARGETS)

__all__ = ["Localizer", "TdoaError", "load", "dpss_q15", "decay_us", "band_weights", "track_host", "track_params",
           "TrackParams", "TrackOutputs", "TRACK_DTYPE", "beam_fir", "beam_geometry", "beam_latency", "beam_host",
           "BeamGeometry", "BeamOutputs", "sep_window", "sep_check", "SEP_LOADING", "SEP_MAX_TARGETS"]


def __getattr__(name):
    # torch-dependent pieces load lazily so the ABI helpers work without torch
    if name == "TRACK_DTYPE":  # numpy loads lazily, as torch does
        import numpy as np
        return np.dtype(TRACK_FIELDS)
    if name == "Localizer":
        from .localizer import Localizer
        return Localizer
    if name in ("synth", "localizer", "stream", "shard"):
        import importlib
        return importlib.import_module(f".{name}", __name__)
    raise AttributeError(name)
