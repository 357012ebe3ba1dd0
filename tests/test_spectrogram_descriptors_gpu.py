"""GPU parity of the spectrogram object's descriptor methods: they forward to the descriptor object with num / freBandArr of
the spectrogram object, the frame count of its last spectrogram call and isPower from its dataType."""
import numpy as np
import pytest

import audioflux_amd as af
from oracle import ref
from tests import spectral_cases as sc
from tests.conftest import HOSTSTUB, assert_parity
from tests.spectral_check import check_output
from tests.test_spectral_gpu import py_call, set_edge

pytestmark = pytest.mark.gpu


def clip(n=16000, seed=3):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.3 * np.sin(2 * np.pi * (300 + 900 * t) * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("data_type", [af.SpectralDataType.POWER, af.SpectralDataType.MAG])
def test_mel_spectrogram_descriptors_equal_the_descriptor_object(data_type):
    x = clip()
    sg = af.MelSpectrogram(num=64, samplate=16000, radix2_exp=10, data_type=data_type)
    spec = sg.spectrogram(x)  # (num, time)
    fre = sg.get_fre_band_arr()
    o = af.Spectral(64, fre)
    for edge in (None, (3, 50), [9, 2, 30, 30, 7]):
        set_edge(sg, edge)
        set_edge(o, edge)
        for case in sc.names_for(None):
            kind = sc.PARAMS[case][0]
            got, want = py_call(sg, case, spec.T, None), py_call(o, case, spec.T, None)
            for g, w in zip(got, want):
                if HOSTSTUB:
                    continue
                if kind == "energy" and data_type == af.SpectralDataType.POWER:
                    continue  # isPower: checked below
                assert np.array_equal(g, w, equal_nan=True), (case, edge)
    # energy of power rows is their mean, not the mean of their squares (spectrogram_algorithm.c:2648-2662)
    if data_type == af.SpectralDataType.POWER and not HOSTSTUB:
        set_edge(sg, (0, 63))
        assert_parity(sg.energy(spec), spec.mean(0), 1e-5, "spectrogram energy of power rows")


def test_linear_spectrogram_descriptors_against_the_compiled_reference():
    if not ref.available():
        pytest.skip("the compiled reference is not here")
    from tests.spectral_ref import RefSpectral
    x = clip(seed=8)
    sg = af.Spectrogram(samplate=16000, radix2_exp=9, data_type=af.SpectralDataType.MAG)
    spec, phase = sg.spectrogram(x, is_phase_arr=True)
    fre = sg.get_fre_band_arr()
    num = spec.shape[0]
    s_t, p_t = np.ascontiguousarray(spec.T), np.ascontiguousarray(phase.T)
    r = RefSpectral(ref.lib(), num, fre, None)
    for case in sc.PARAMS:
        kind, iarg, farg = sc.PARAMS[case]
        want = r.run(kind, iarg, farg, s_t, p_t)
        got = py_call(sg, case, s_t, p_t)
        for k in range(len(want)):
            check_output(f"linear spectrogram {case}[{k}]", case, got[k], want[k], s_t, p_t, fre, np.arange(num), num, second=bool(k))


def test_preprocess_divides_by_the_window_sum():
    x = clip()
    for data_type in (af.SpectralDataType.MAG, af.SpectralDataType.POWER):
        sg = af.Spectrogram(samplate=16000, radix2_exp=9, data_type=data_type)
        spec = sg.spectrogram(x)
        got = sg.preprocess(spec)
        w = np.float32(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(512) / 512)).sum(dtype=np.float64)
        value = 0.5 * w if data_type == af.SpectralDataType.MAG else 0.5 * w * w
        want = spec / value
        want[0] *= 0.5
        want[256] *= 0.5
        assert_parity(got, want, 1e-5, f"preprocess {data_type.name}")


def test_flux_defaults_are_the_reference_spectrogram_wrapper_s():
    """the reference's spectrogram wrapper passes is_no_exp=True as the C isExp argument (python/audioflux/spectrogram.py:
    624-680): a bare sg.flux(spec) is the p-th ROOT of the sum, p = 2 -- unlike Spectral.flux, whose is_exp defaults to False"""
    x = clip(seed=11)
    sg = af.MelSpectrogram(num=40, samplate=16000, radix2_exp=10)
    spec = sg.spectrogram(x)
    got = sg.flux(spec)
    s_t = np.ascontiguousarray(spec.T)
    fre = sg.get_fre_band_arr()
    if ref.available():
        from tests.spectral_ref import RefSpectral
        want = RefSpectral(ref.lib(), 40, fre, None).run("flux", (1, 0, 1, 0), (2.0,), s_t)[0]
    else:
        want = np.zeros(s_t.shape[0], np.float32)
        want[1:] = np.sqrt((np.diff(s_t.astype(np.float64), axis=0) ** 2).sum(1))
    assert_parity(got, want, 1e-5, "spectrogram flux, defaults")
    if not HOSTSTUB:
        assert_parity(sg.flux(spec, is_no_exp=False), want.astype(np.float64) ** 2, 1e-5, "spectrogram flux, is_no_exp=False")
        assert_parity(af.Spectral(40, fre).flux(spec), want.astype(np.float64) ** 2, 1e-5, "Spectral.flux, defaults")
    with pytest.raises(TypeError):
        sg.broadband(spec)  # no default threshold on the spectrogram classes


def test_descriptor_input_must_have_the_frames_of_the_last_spectrogram_call():
    sg = af.MelSpectrogram(num=40, samplate=16000, radix2_exp=10)
    with pytest.raises(ValueError):
        sg.centroid(np.ones((40, 5), np.float32))
    spec = sg.spectrogram(clip())
    sg.centroid(spec)
    with pytest.raises(ValueError):
        sg.centroid(spec[:, :-3])
    with pytest.raises(ValueError):
        sg.preprocess(spec[:, :-3])
