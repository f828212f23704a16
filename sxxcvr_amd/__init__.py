"""sxxcvr_amd -- MI355X-native polyphase FIR resampling path behind the
SoapySDR ``driver=sx`` Device/Stream surface of tejeez/sxxcvr.

The product is native: hand-written HIP kernels (gfx950) behind a C ABI
(include/sxfir.h, include/sxfir_complex.h, include/sxfir_channelizer.h,
include/sxfir_channelizer_os.h, include/sxfir_synthesizer.h, include/sxfir_synthesizer_os.h, include/sxfir_rational.h,
include/sxfir_translate.h, include/sxfir_translate_tx.h, include/sxfir_arbitrary.h, include/sx_device.h).
This package only loads those
libraries and mirrors the reference's Python-facing call pattern; there is no
CPU implementation and nothing here imports the oracle.
"""
from ._native import NativeError, load_sxfir  # noqa: F401
from .resampler import ArbitraryResampler, Channelizer, ComplexInterpolator, PipelinedResampler, RationalResampler, Resampler, Synthesizer, TranslatingBank, TranslatingCombiner, TranslatingDecimator, TranslatingInterpolator, design_arbitrary, design_bandpass, design_lowpass, design_rational, design_rotator, pin_array, synth_fill, unpin_array  # noqa: F401

__all__ = ["NativeError", "load_sxfir", "Resampler", "ComplexInterpolator", "RationalResampler", "ArbitraryResampler", "TranslatingDecimator", "TranslatingInterpolator", "TranslatingBank", "TranslatingCombiner", "Channelizer", "Synthesizer", "PipelinedResampler", "design_lowpass", "design_bandpass", "design_rational", "design_arbitrary", "design_rotator", "synth_fill", "pin_array", "unpin_array"]
