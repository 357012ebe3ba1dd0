"""audioflux_amd -- MI355X-native backend for audioFlux's batched
time-frequency hot path (BFT/STFT -> filter bank -> MFCC/xxcc, CWT, CQT,
cepstrogram).  The product is the C-ABI library lib/libaudioflux_mi355x.so
(hand-written gfx950 HIP kernels behind the reference's own C API); the
classes here mirror the reference's ctypes wrapper for that path."""
from . import _lib
from ._lib import LIB_PATH, build, get_lib, last_error, runtime_status
from .types import *  # noqa: F401,F403
from .bft import BFT
from .xxcc import XXCC
from .spectral import Spectral
from .cepstrogram import Cepstrogram
from .cqt import CQT
from .cwt import CWT
from .fst import FST
from .pwt import PWT
from .nsgt import NSGT
from .reassign import Reassign
from .resample import Resample, WindowResample
from .st import ST
from .stft import STFT
from .harmonic_ratio import HarmonicRatio
from .hpss import HPSS, median_filter_device
from .onset import NoveltyParam, Onset, max_filter_device, peak_pick_device, power_to_db, power_to_db_device
from .pitchshift import PitchShift
from .pitch import PitchCEP, PitchHPS, PitchLHS, PitchNCF, PitchPEF, PitchYIN
from .synsq import Synsq
from .timestretch import TimeStretch
from .wsst import WSST
from .spectrogram import (Bark, BarkSpectrogram, Chroma, Erb, ErbSpectrogram, Linear, Mel, MelSpectrogram,
                          Spectrogram, SpectrogramBase, SpectralFilterBankType)
from .batch import mel_mfcc_device

__all__ = ["BFT", "XXCC", "Spectral", "SpectralNoveltyMethodType", "SpectralNoveltyDataType", "Cepstrogram", "CQT", "CWT", "FST", "PWT", "NSGT", "Reassign", "Resample", "WindowResample", "ResampleQualityType", "ST", "STFT", "HarmonicRatio", "HPSS", "median_filter_device", "Onset", "NoveltyParam", "NoveltyType", "power_to_db", "power_to_db_device",
           "max_filter_device", "peak_pick_device", "PitchYIN", "PitchHPS", "PitchLHS", "PitchPEF", "PitchNCF", "PitchCEP", "PitchShift", "TimeStretch", "Synsq", "WSST", "Spectrogram", "SpectrogramBase", "MelSpectrogram", "BarkSpectrogram", "ErbSpectrogram",
           "Linear", "Mel", "Bark", "Erb", "Chroma", "SpectralFilterBankType", "mel_mfcc_device", "get_lib", "build", "runtime_status",
           "last_error", "LIB_PATH"]
