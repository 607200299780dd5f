"""GPU: recording preparation (csrc/resample.hip, csrc/trim.hip; utils.audio.resample / trim / prepare_recording,
utils.data.drop_silent_frames) against the float64 restatements of tests/recording_ref.py."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import recording_ref as R
from conftest import WAVE_TOL
from melspec_ref import voiced

pytestmark = pytest.mark.gpu

MFMA_FRAMES = 64                     # frames per block of the MFMA kernel (csrc/resample.hip)
# route 2 must take at least these; 44 100 -> 22 050 (n = 1) must refuse it
MUST_BE_ELIGIBLE = {(48000, 22050, 1024), (48000, 22050, 64), (16000, 22050, 64)}


@functools.lru_cache(maxsize=None)
def _case(case):
    """Rows of one rate pair, their float64 reference and the fp32 conv1d figure, computed once."""
    orig, new, lfw = case
    taps = R.taps_ref(orig, new, lfw)
    _, width, o, n = taps
    long_row = (2 * MFMA_FRAMES + 20) * o + 7             # three frame tiles of the MFMA kernel, ending inside the third
    lens = [1, max(o - 1, 1), o, o + 1, 2 * width + 3, 6000, 6001, long_row]
    rows = [voiced(L, 10 + i, sr=orig) for i, L in enumerate(lens)]
    refs = [R.resample_ref(r, orig, new, taps=taps).numpy() for r in rows]
    f32 = max(float(np.abs(R.resample_ref(r, orig, new, dtype=torch.float32, taps=taps).numpy().astype(np.float64) - ref).max())
              for r, ref in zip(rows, refs))
    return rows, refs, f32, (o, n)


def _engine(case):
    from ttsamd.engine import ResampleEngine
    return ResampleEngine(case[0], case[1], lowpass_filter_width=case[2])


@pytest.mark.parametrize('case', sorted(R.RATE_CASES))
def test_resample_both_routes_against_float64(case):
    from ttsamd.lib import TtsAmdError
    rows, refs, f32, (o, n) = _case(case)
    eng = _engine(case)
    assert (eng.o, eng.n, eng.taps_per_phase) == R.RATE_CASES[case]
    buf, lens = R.pack_rows(rows)
    wave, dl = torch.from_numpy(buf).cuda(), torch.from_numpy(lens).cuda()
    if case in MUST_BE_ELIGIBLE:
        assert eng.mfma_eligible
    if n == 1:
        assert not eng.mfma_eligible
    if not eng.mfma_eligible:
        with pytest.raises(TtsAmdError, match='route 2'):
            eng.forward(wave, dl, route='mfma')
    outs = {}
    routes = ['general'] + (['mfma'] if eng.mfma_eligible else [])
    for route in routes:
        out, nout = eng.forward(wave, dl, route=route)
        out2, _ = eng.forward(wave, dl, route=route)
        out, out2, nout = out.cpu().numpy(), out2.cpu().numpy(), nout.cpu().numpy()
        outs[route] = out
        assert out.shape[1] == eng.out_len(buf.shape[1]) == R.out_len(buf.shape[1], o, n)
        assert nout.tolist() == [R.out_len(int(L), o, n) for L in lens]
        err = max(float(np.abs(out[b, :nout[b]].astype(np.float64) - refs[b]).max()) for b in range(len(rows)))
        print(f'{case} route {route}: max-abs against float64 {err:.2e}; F.conv1d in fp32 on the CPU {f32:.2e}; ratio {err / f32:.2f}')
        assert err < WAVE_TOL
        for b in range(len(rows)):
            assert not out[b, nout[b]:].any(), (route, b)                     # zeros behind the row, poison never read
            alone, na = eng.forward(torch.from_numpy(np.ascontiguousarray(buf[b:b + 1, :lens[b]])).cuda(), None, route=route)
            assert int(na[0]) == nout[b]
            assert np.array_equal(alone[0, :nout[b]].cpu().numpy().view(np.uint32), out[b, :nout[b]].view(np.uint32)), (route, b)
        assert np.array_equal(out.view(np.uint32), out2.view(np.uint32))
    for route in routes[1:]:
        print(f'{case}: routes general and {route} differ in {int((outs["general"] != outs[route]).sum())} of {outs[route].size} samples')
    auto, _ = eng.forward(wave, dl)
    assert any(np.array_equal(auto.cpu().numpy().view(np.uint32), o_.view(np.uint32)) for o_ in outs.values())


def test_resample_surface_shapes_and_equal_rates():
    from utils.audio import Resample, resample
    x = torch.from_numpy(voiced(2 * 3 * 1000, 7, sr=16000).reshape(2, 3, 1000)).cuda()
    y = resample(x, 16000, 22050)
    assert tuple(y.shape) == (2, 3, 1379)
    ref = R.resample_ref(x[1, 2].cpu().numpy(), 16000, 22050).numpy()
    assert np.abs(y[1, 2].cpu().numpy() - ref).max() < WAVE_TOL
    assert resample(x, 22050, 22050) is x
    y2, n2 = Resample(16000, 22050)(x[0], lens=torch.tensor([1000, 10, 500]))
    assert n2.tolist() == [1379, 14, 690] and not y2[1, 14:].any()
    assert np.array_equal(y2[0].cpu().numpy(), y[0, 0].cpu().numpy())


def _trim_batch():
    rows = R.trim_rows()
    buf, lens = R.pack_rows(rows)
    return rows, torch.from_numpy(buf).cuda(), torch.from_numpy(lens).cuda()


def test_trim_bounds_and_peak_exact():
    from utils.audio import trim
    from ttsamd.engine import TrimEngine
    rows, wave, lens = _trim_batch()
    want = []
    for i, x in enumerate(rows):
        bounds, margin = R.trim_ref(x, 23, 1024, 256)
        if i < 4:
            assert margin > 0.5 and bounds == R.TRIM_BOUNDS[i]                # a condition on the inputs: fp32 rounding never decides
        want.append(bounds)
    assert want[4] == (0, 3000) and len(rows[5]) < 256
    bounds, peak = TrimEngine().bounds(wave, lens, top_db=23, frame_length=1024, hop_length=256)
    assert bounds.cpu().tolist() == [list(b) for b in want]
    assert np.array_equal(peak.cpu().numpy(), np.array([np.abs(x).max() for x in rows], dtype=np.float32))
    assert torch.equal(trim(wave, 23, 1024, 256, lens=lens), bounds)
    y, (s, e) = trim(wave[0, :lens[0]], top_db=23, frame_length=1024, hop_length=256)
    assert (s, e) == want[0] and torch.equal(y, wave[0, s:e])


def test_prepare_recording_bit_exact_after_the_resampler_and_against_float64():
    from utils.audio import prepare_recording, resample
    segs = [(3000, 9000, 4000), (0, 12001, 2500), (2600, 7000, 0)]
    rng = np.random.default_rng(1)
    rows = [np.concatenate([1e-3 * rng.standard_normal(a), voiced(b, 50 + i, sr=48000).astype(np.float64),
                            1e-3 * rng.standard_normal(c)]).astype(np.float32) for i, (a, b, c) in enumerate(segs)]
    buf, lens = R.pack_rows(rows)
    wave, dl = torch.from_numpy(buf).cuda(), torch.from_numpy(lens).cuda()
    out, olen = prepare_recording(wave, 48000, lens=dl, lowpass_filter_width=64)
    res, rlen = resample(wave, 48000, 22050, 64, lens=dl)
    assert out.shape[1] == res.shape[1] + 768
    out, olen, res, rlen = out.cpu().numpy(), olen.cpu().numpy(), res.cpu().numpy(), rlen.cpu().numpy()
    taps = R.taps_ref(48000, 22050, 64)
    for b, x in enumerate(rows):
        # (1) the GPU's own resampled row through numpy's float32 arithmetic: pins trim_apply and the bounds
        y = res[b, :rlen[b]]
        y = y / np.abs(y).max() * np.float32(0.999)
        assert y.dtype == np.float32
        (s, e), margin = R.trim_ref(y, 23, 1024, 256)
        assert margin > 0.5
        want = np.concatenate([y[s:e], np.zeros(768, dtype=np.float32)])
        assert olen[b] == want.size
        assert np.array_equal(out[b, :olen[b]].view(np.uint32), want.view(np.uint32)), b
        assert not out[b, olen[b]:].any()
        # (2) the float64 pipeline from the 48 kHz input: same bounds, samples within the resampler's bar scaled by the gain
        r = R.resample_ref(x, 48000, 22050, taps=taps).numpy()
        m = np.abs(r).max()
        r = r / m * 0.999
        (s64, e64), margin64 = R.trim_ref(r, 23, 1024, 256)
        assert margin64 > 0.5 and (s64, e64) == (s, e)
        err = float(np.abs(out[b, :e - s].astype(np.float64) - r[s:e]).max())
        print(f'row {b}: bounds {(s, e)}, max-abs against the float64 pipeline {err:.2e} (bar {WAVE_TOL * 0.999 / m:.2e})')
        assert err < WAVE_TOL * 0.999 / m


def test_drop_silent_frames_equals_boolean_indexing():
    from utils.data import drop_silent_frames
    rng = np.random.default_rng(3)
    T = 300
    loud = np.zeros((5, T), dtype=bool)
    loud[0, 20:120] = loud[0, 160:290] = True           # silence at the start, in the middle and at the end (the end is kept)
    loud[1, :] = False                                  # no frame above the threshold
    loud[2, :] = True                                   # all above
    loud[3, 0:50] = True                                # trailing silence kept
    loud[4, 0] = False                                  # T = 1, silent
    lens = np.array([300, 77, 259, 131, 1], dtype=np.int64)
    mel = rng.normal(0.0, 0.5, size=(5, 80, T)).astype(np.float32) + np.where(loud, -4.0, -11.5)[:, None, :].astype(np.float32)
    pitch = rng.uniform(80, 300, size=(5, 1, T)).astype(np.float32)
    dmel, dpitch, dl = torch.from_numpy(mel).cuda(), torch.from_numpy(pitch).cuda(), torch.from_numpy(lens).cuda()
    om, op, ol = drop_silent_frames(dmel, dl, -10.0, extra=dpitch)
    om2, ol2 = drop_silent_frames(dmel, dl, -10.0)
    assert torch.equal(om, om2) and torch.equal(ol, ol2)
    for b in range(5):
        e = mel[b, :, :lens[b]].astype(np.float64).mean(0)
        assert np.abs(e + 10.0).min() > 0.01                                  # a condition on the inputs
        keep = torch.from_numpy(R.remove_silence_ref(e, -10.0))
        k = int(keep.sum())
        assert int(ol[b]) == k
        assert torch.equal(om[b, :, :k].cpu(), torch.from_numpy(mel[b, :, :lens[b]])[:, keep])
        assert torch.equal(op[b, :, :k].cpu(), torch.from_numpy(pitch[b, :, :lens[b]])[:, keep])
        assert not om[b, :, k:].any() and not op[b, :, k:].any()
    assert ol.cpu().tolist() == [300 - 20 - 40, 76, 259, 131, 0]


def test_error_paths():
    from ttsamd.lib import TtsAmdError
    from utils.audio import prepare_recording, resample, trim
    from utils.data import drop_silent_frames
    x = torch.zeros(2, 1000, device='cuda')
    with pytest.raises(TtsAmdError, match='sinc_interp_hann'):
        resample(x, 48000, 22050, resampling_method='sinc_interp_kaiser')
    for fn in (lambda: resample(x.cpu(), 48000, 22050), lambda: trim(x.cpu()), lambda: prepare_recording(x.cpu(), 48000),
               lambda: drop_silent_frames(torch.zeros(1, 80, 10))):
        with pytest.raises(TtsAmdError):
            fn()
    for bad in [(0, 22050), (48000, -1), (48000.5, 22050)]:
        with pytest.raises(TtsAmdError):
            resample(x, *bad)
    with pytest.raises(TtsAmdError, match='frame_length'):
        trim(x, frame_length=16384, hop_length=512)
    with pytest.raises(TtsAmdError, match='hop_length'):
        trim(x, frame_length=1024, hop_length=2048)


def test_new_symbols_are_bound_and_the_abi_revision_stays():
    from ttsamd import lib
    h = lib.load()
    for name in ('ttsamd_resample_create', 'ttsamd_resample_destroy', 'ttsamd_resample_out_len', 'ttsamd_resample_forward',
                 'ttsamd_trim_bounds', 'ttsamd_trim_apply', 'ttsamd_frames_compact'):
        assert name in lib.SYMBOLS and getattr(h, name) is not None
    assert lib.ABI_VERSION == 8 == h.ttsamd_version()
