"""Multi-resolution STFT distance on the GPU (pytest -m gpu): ttsamd_mr_stft (csrc/mrstft.hip) through the C ABI, ttsamd.engine.mr_stft
and the utils.objective wrappers, against the float64 restatement tests/mrstft_ref.py (pinned on the CPU by tests/test_mrstft_cpu.py
against torch.stft).  Every buffer is NaN behind a row's length.

Bounds.  frames: exact.  Spectral convergence: 1e-11 relative (SDR_RTOL of tests/test_gpu_wavescore.py); log-magnitude distance: 1e-9
absolute (its LSD_TOL).  Derivation: the kernel's transform has at most 11 butterfly levels (2048 = 2 * 4^5), each rounding at 2^-53
of the frame's norm, so a bin is off by about 11 * 1.1e-16 * ||frame|| = 1.2e-15 ||frame||, the restatement's rfft by as much.  sc is
a ratio of two norms over all bins: the denominator moves by 1e-15 relative, the numerator ||S_ref - S_est|| by 1e-15 ||S_ref|| in
absolute terms, and the pairs of these tests differ by no less than a 30 dB noise (||S_ref - S_est|| of the order of 0.03 ||S_ref||;
est = 0 is larger still), so sc moves by less than 1e-13 relative; the sums of up to 4e5 float64 terms in another order add 1e-13.  mag is a
mean of |ln S_ref - ln S_est|: a bin's ln S moves by 1.2e-15 ||frame|| / S, at most 1e-11 for a bin at the floor sqrt(1e-7) of a
frame of norm 3, and the mean over the bins is far below the worst bin.  Both bounds leave two orders of room; an error of the
framing (one sample of offset, a wrong reflection, the symmetric window) moves either number by more than 1e-4.  The identical pair
is exact: both signals go through the same transform.  Rows of a ragged batch, two runs and the wrappers: bit for bit.

Lengths, per resolution (N, H, W), the smallest that take each branch: N / 2 (NaN, 0 frames), N / 2 + 1 (the shortest valid row: both
reflections inside one frame), N - 1, k H - 1 and k H (the frame count steps; k = N / H + 2 so that both are valid), 16 H and 32 H
(one frame more than one block's chunk of 16 frames, and than two), 20 000."""
import ctypes as C

import numpy as np
import pytest
import torch

import mrstft_ref as M
import wavescore_ref as R

pytestmark = pytest.mark.gpu

SC_RTOL, MAG_TOL = 1e-11, 1e-9
CHUNK = 16                                                              # frames per block of mr_stft_kernel
EXTRA = ((512, 128, 512), (1024, 77, 241))
RESOLUTIONS = M.DEFAULT + EXTRA
SNRS = (30.0, 10.0, -5.0)


def lengths(N, H):
    k = N // H + 2
    return (N // 2, N // 2 + 1, N - 1, k * H - 1, k * H, CHUNK * H, 2 * CHUNK * H, 20000)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def x():
    return R.speech_like()


@pytest.fixture(scope='module')
def ests(x):
    """the estimates by name, computed once: noisy copies, zeros, the reference itself"""
    out = {f'{snr:g} dB': R.add_noise(x, snr) for snr in SNRS}
    out['zero'] = np.zeros_like(x)
    out['same'] = x
    return out


_want = {}


def want(x, ests, name, n, res):
    """the restatement's (sc, mag, frames) of one row at one resolution, computed once and shared"""
    key = (name, n, res)
    if key not in _want:
        _want[key] = M.stft_distance(x[:n], ests[name][:n], *res)
    return _want[key]


def _poisoned(xs, dev, stride=None):
    """rows of different lengths in one buffer whose every entry behind a row's length is NaN -> (wave [B, stride], lens int64 [B])"""
    stride = max(len(v) for v in xs) if stride is None else stride
    buf = np.full((len(xs), stride), np.nan, dtype=np.float32)
    for b, v in enumerate(xs):
        buf[b, :len(v)] = v
    return torch.from_numpy(buf).to(dev), torch.tensor([len(v) for v in xs], dtype=torch.int64, device=dev)


def _mr(rs, es, dev, resolutions, stride=None):
    """-> (per [B, R, 2], frames [B, R]) as numpy, from NaN-poisoned buffers"""
    from ttsamd.engine import mr_stft
    wr, lens = _poisoned(rs, dev, stride)
    we, _ = _poisoned(es, dev, stride)
    per, frames = mr_stft(wr, we, lens, resolutions)
    assert per.dtype == torch.float64 and frames.dtype == torch.int32 and per.device == wr.device
    assert tuple(per.shape) == (len(rs), len(resolutions), 2) and tuple(frames.shape) == (len(rs), len(resolutions))
    return per.cpu().numpy(), frames.cpu().numpy()


def _check_row(got, frames, ref, what):
    """one (sc, mag), frame count against the restatement's triple -> the two differences"""
    sc, mag, F = ref
    assert frames == F, (what, frames, F)
    if F == 0:
        assert np.isnan(got).all() and np.isnan(sc) and np.isnan(mag), (what, got)
        return 0.0, 0.0
    dsc = abs(got[0] - sc) / abs(sc) if sc != 0.0 else abs(got[0])
    dmag = abs(got[1] - mag)
    assert dsc <= SC_RTOL and dmag <= MAG_TOL, (what, got.tolist(), sc, mag)
    return dsc, dmag


@pytest.mark.parametrize('res', RESOLUTIONS, ids=lambda r: '-'.join(map(str, r)))
def test_kernel_against_the_restatement(dev, x, ests, res):
    N, H, W = res
    ns = lengths(N, H)
    worst_sc = worst_mag = 0.0
    for name, y in ests.items():
        per, frames = _mr([x[:n] for n in ns], [y[:n] for n in ns], dev, [res])
        for b, n in enumerate(ns):
            ref = want(x, ests, name, n, res)
            assert ref[2] == (1 + n // H if n > N // 2 else 0)
            dsc, dmag = _check_row(per[b, 0], int(frames[b, 0]), ref, (name, n, res))
            worst_sc, worst_mag = max(worst_sc, dsc), max(worst_mag, dmag)
            if name == 'same' and n > N // 2:
                assert per[b, 0].tolist() == [0.0, 0.0]               # exactly
    print(f'resolution {res}: worst relative difference of sc {worst_sc:.3e} (bound {SC_RTOL:.0e}), worst absolute difference of mag '
          f'{worst_mag:.3e} (bound {MAG_TOL:.0e})')


def test_five_resolutions_in_one_call(dev, x, ests):
    """R = 5: the defaults and two more, one of them with N - W odd; every resolution has the bits of its own call"""
    ns = (600, 3000, 20000)                                             # 600: too short at 2048 only
    y = ests['10 dB']
    per, frames = _mr([x[:n] for n in ns], [y[:n] for n in ns], dev, RESOLUTIONS)
    for r, res in enumerate(RESOLUTIONS):
        one, fone = _mr([x[:n] for n in ns], [y[:n] for n in ns], dev, [res])
        assert one[:, 0].tobytes() == per[:, r].tobytes() and np.array_equal(fone[:, 0], frames[:, r])
        for b, n in enumerate(ns):
            _check_row(per[b, r], int(frames[b, r]), want(x, ests, '10 dB', n, res), (n, res))
    assert frames[0].tolist() == [6, 0, 13, 5, 8] and np.isnan(per[0, 1]).all() and np.isfinite(per[0, [0, 2, 3, 4]]).all()


def test_ragged_batch_rows_are_the_rows_alone(dev, x, ests):
    ns = (20000, 1024, 1025, 32 * 240, 2047)                            # at 2048: long, NaN, shortest valid, two chunks + 1 frame, N - 1
    names = ('10 dB', '30 dB', '-5 dB', 'zero', 'same')
    rs, es = [x[:n] for n in ns], [ests[k][:n] for k, n in zip(names, ns)]
    per, frames = _mr(rs, es, dev, M.DEFAULT, stride=20096)
    again = _mr(rs, es, dev, M.DEFAULT, stride=20096)
    assert per.tobytes() == again[0].tobytes() and np.array_equal(frames, again[1])      # two runs: the same bits
    for b, n in enumerate(ns):
        for r, res in enumerate(M.DEFAULT):
            _check_row(per[b, r], int(frames[b, r]), want(x, ests, names[b], n, res), (n, res))
        for stride in (n, 20096):                                       # alone, trimmed and in the batch's stride
            p1, f1 = _mr(rs[b:b + 1], es[b:b + 1], dev, M.DEFAULT, stride=stride)
            assert p1.tobytes() == per[b:b + 1].tobytes() and np.array_equal(f1, frames[b:b + 1]), (n, stride)
    assert np.isnan(per[1, 1]).all() and frames[1, 1] == 0 and per[4].tolist() == [[0.0, 0.0]] * 3


def _raw(dev, res, B=1, n=3000, short=0, null=None):
    """ttsamd_mr_stft through ctypes on poisoned output buffers -> (rc, out, frames): `short` bytes taken off the workspace size"""
    from ttsamd import lib as L
    h = L.load()
    wave = torch.zeros(B, n, device=dev)
    lens = torch.full((B,), n, dtype=torch.int64, device=dev)
    R_ = len(res)
    arr = [(C.c_int32 * max(R_, 1))(*(r[q] for r in res)) for q in range(3)]
    nbytes = int(h.ttsamd_mr_stft_workspace_bytes(B, n, arr[0], arr[1], arr[2], R_))
    ok = [(C.c_int32 * 1)(v) for v in (512, 128, 512)]
    size = nbytes if nbytes >= 0 else int(h.ttsamd_mr_stft_workspace_bytes(B, n, ok[0], ok[1], ok[2], 1))
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    out = torch.full((B, max(R_, 1), 2), -7.0, dtype=torch.float64, device=dev)
    frames = torch.full((B, max(R_, 1)), -7, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    args = [p(wave), p(wave), n, p(lens), B, arr[0], arr[1], arr[2], R_, p(out), p(frames), p(ws), size - short,
            C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    if null is not None:
        args[null] = None
    rc = h.ttsamd_mr_stft(*args)
    torch.cuda.synchronize()
    return rc, nbytes, out.cpu(), frames.cpu()


@pytest.mark.parametrize('res, short', [
    ([(256, 64, 256)], 0), ([(4096, 1024, 4096)], 0), ([(512, 128, 513)], 0), ([(1024, 256, 0)], 0), ([(1024, 0, 1024)], 0),
    ([], 0), ([(512, 128, 512)] * 9, 0), ([(1024, 120, 600), (300, 100, 300)], 0), (list(M.DEFAULT), 1)],
    ids=['n_fft 256', 'n_fft 4096', 'W > N', 'W = 0', 'hop 0', 'R = 0', 'R = 9', 'second resolution bad', 'workspace one byte short'])
def test_refusals_leave_the_outputs_untouched(dev, res, short):
    from ttsamd import lib as L
    rc, nbytes, out, frames = _raw(dev, res, short=short)
    assert rc == -1                                                     # TTSAMD_EINVAL
    assert (nbytes > 0) if short else (nbytes == -1)
    assert bool((out == -7.0).all()) and bool((frames == -7).all())
    with pytest.raises(L.TtsAmdError):
        L.check(rc, 'mr_stft')
    if not short:                                                       # the wrapper refuses the same resolutions
        from ttsamd.engine import mr_stft
        with pytest.raises(L.TtsAmdError):
            mr_stft(torch.zeros(1, 3000, device=dev), torch.zeros(1, 3000, device=dev), None, res)


def test_null_pointers_and_batch_are_refused_and_a_full_workspace_runs(dev):
    from ttsamd import lib as L
    rc, nbytes, out, frames = _raw(dev, list(M.DEFAULT))
    assert rc == 0 and nbytes > 0 and frames[0].tolist() == [26, 13, 61] and out[0].tolist() == [[0.0, 0.0]] * 3
    for null in (0, 1, 3, 5, 6, 7, 9, 10, 11):
        rc, _, out, frames = _raw(dev, list(M.DEFAULT), null=null)
        assert rc == -1 and bool((out == -7.0).all()) and bool((frames == -7).all()), null
    h = L.load()
    arr = [(C.c_int32 * 1)(v) for v in (512, 128, 512)]
    assert h.ttsamd_mr_stft_workspace_bytes(0, 3000, arr[0], arr[1], arr[2], 1) == -1
    assert h.ttsamd_mr_stft_workspace_bytes(65536, 3000, arr[0], arr[1], arr[2], 1) == -1
    assert h.ttsamd_mr_stft_workspace_bytes(1, -1, arr[0], arr[1], arr[2], 1) == -1
    assert h.ttsamd_mr_stft_workspace_bytes(1, 1 << 31, arr[0], arr[1], arr[2], 1) == -1
    assert h.ttsamd_mr_stft_workspace_bytes(1, 3000, None, arr[1], arr[2], 1) == -1


@pytest.fixture(scope='module')
def pair22(dev):
    """one second at 22 050 Hz and a degraded copy, on the device"""
    a = R.speech_like(22050, fs=22050, seed=5)
    return torch.from_numpy(a).to(dev), torch.from_numpy(R.add_noise(a, 10.0, seed=6)).to(dev)


def test_multi_resolution_stft_keys_shapes_and_numpy_conventions(dev, pair22):
    from ttsamd.engine import WaveScoreEngine, mr_stft
    from utils.objective import MR_STFT_KEYS, multi_resolution_stft, stft_distance
    a, b = pair22
    m = multi_resolution_stft(b, a)
    assert tuple(m) == MR_STFT_KEYS == ('mr_stft', 'spectral_convergence', 'log_stft_magnitude', 'per_resolution', 'frames')
    assert all(isinstance(v, torch.Tensor) and v.device.type == 'cuda' for v in m.values())
    assert all(m[k].dtype == torch.float64 and m[k].dim() == 0 for k in MR_STFT_KEYS[:3])
    assert m['per_resolution'].dtype == torch.float64 and tuple(m['per_resolution'].shape) == (3, 2)
    assert m['frames'].dtype == torch.int32 and m['frames'].tolist() == [1 + 22050 // 120, 1 + 22050 // 240, 1 + 22050 // 50]
    assert torch.equal(m['mr_stft'], m['spectral_convergence'] + m['log_stft_magnitude'])          # bit for bit
    per, frames = mr_stft(a[None], b[None])
    assert torch.equal(per[0], m['per_resolution']) and torch.equal(frames[0], m['frames'])
    eng = WaveScoreEngine(22050, device=dev).mr_stft(a[None], b[None])
    assert torch.equal(eng[0], per) and torch.equal(eng[1], frames)
    assert torch.equal(m['spectral_convergence'], per[0, :, 0].mean()) and torch.equal(m['log_stft_magnitude'], per[0, :, 1].mean())
    want = M.mr_stft(a.cpu().numpy(), b.cpu().numpy())
    assert np.abs(per[0, :, 0].cpu().numpy() - want[0][:, 0]).max() <= SC_RTOL * want[0][:, 0].max()
    assert np.abs(per[0, :, 1].cpu().numpy() - want[0][:, 1]).max() <= MAG_TOL and 0.0 < float(m['mr_stft'])
    for r, (N, H, W) in enumerate(M.DEFAULT):                           # one resolution: the bits of its row
        sc, mag = stft_distance(b, a, n_fft=N, hop_length=H, win_length=W)
        assert isinstance(sc, torch.Tensor) and sc.dtype == torch.float64 and sc.dim() == 0
        assert torch.equal(sc, m['per_resolution'][r, 0]) and torch.equal(mag, m['per_resolution'][r, 1])
    sc, mag = stft_distance(b, a)                                       # 1024 / 256, win_length None: n_fft
    two = multi_resolution_stft(b, a, (1024, 512), (256, 128), (1024, 512))
    assert torch.equal(sc, two['per_resolution'][0, 0]) and torch.equal(mag, two['per_resolution'][0, 1])
    an, bn = a.cpu().numpy(), b.cpu().numpy()
    mn = multi_resolution_stft(bn, an)                                  # numpy in: floats and arrays out
    assert all(isinstance(mn[k], float) and mn[k] == m[k].item() for k in MR_STFT_KEYS[:3])
    assert isinstance(mn['per_resolution'], np.ndarray) and mn['per_resolution'].shape == (3, 2) and mn['frames'].dtype == np.int32
    assert np.array_equal(mn['per_resolution'], m['per_resolution'].cpu().numpy()) and mn['frames'].tolist() == m['frames'].tolist()
    assert mn['mr_stft'] == mn['spectral_convergence'] + mn['log_stft_magnitude']
    scn, magn = stft_distance(bn, an, 2048, 240, 1200)
    assert isinstance(scn, float) and (scn, magn) == tuple(mn['per_resolution'][1].tolist())
    mb = multi_resolution_stft(np.stack([bn, bn]), np.stack([an, an[::-1].copy()]), lens=[22050, 1000])    # batched: [B] and [B, R, 2]
    assert all(isinstance(mb[k], np.ndarray) and mb[k].shape == (2,) for k in MR_STFT_KEYS[:3])
    assert mb['per_resolution'].shape == (2, 3, 2) and mb['frames'].shape == (2, 3)
    assert all(mb[k][0] == mn[k] for k in MR_STFT_KEYS[:3]) and np.array_equal(mb['per_resolution'][0], mn['per_resolution'])
    assert mb['frames'][1].tolist() == [9, 0, 21] and all(np.isnan(mb[k][1]) for k in MR_STFT_KEYS[:3])   # NaN where any resolution is
    assert np.isfinite(mb['per_resolution'][1, [0, 2]]).all()
    sb = stft_distance(np.stack([bn, bn]), np.stack([an, an]), 512, 50, 240, lens=[22050, 1000])
    assert sb[0].shape == (2,) and sb[0][0] == mn['per_resolution'][2, 0] and sb[1][0] == mn['per_resolution'][2, 1]
    wide = multi_resolution_stft(torch.nn.functional.pad(b, (0, 50)), a)      # different padded widths: compared over the min of the two
    assert all(torch.equal(wide[k], m[k]) for k in MR_STFT_KEYS)


def test_wave_metrics_and_copy_synthesis_carry_the_keys_on_request(dev, pair22):
    from ttsamd import engine as E
    from ttsamd import synth
    from ttsamd.config import HIFIGAN_CONFIG
    from utils.objective import MR_STFT_KEYS, WAVE_KEYS, copy_synthesis, multi_resolution_stft, wave_metrics
    from vocoder.hifigan.models import Generator
    a, b = pair22
    plain, more, mr = wave_metrics(b, a), wave_metrics(b, a, mr_stft=True), multi_resolution_stft(b, a)
    assert tuple(plain) == WAVE_KEYS == ('stoi', 'estoi', 'si_sdr', 'snr', 'lsd', 'frames', 'frames_kept')
    assert tuple(more) == WAVE_KEYS + MR_STFT_KEYS[:3]
    assert all(torch.equal(more[k], plain[k]) for k in WAVE_KEYS) and all(torch.equal(more[k], mr[k]) for k in MR_STFT_KEYS[:3])
    mn = wave_metrics(b.cpu().numpy(), a.cpu().numpy(), mr_stft=True)
    assert all(isinstance(mn[k], float) and mn[k] == more[k].item() for k in MR_STFT_KEYS[:3]) and isinstance(mn['frames'], int)
    hsd = synth.hifigan_state_dict()
    gen = Generator(dict(HIFIGAN_CONFIG), state_dict={k: torch.from_numpy(np.array(v)) for k, v in hsd.items()}).to(dev)
    score32, out32 = copy_synthesis(gen, a, mr_stft=True)
    assert tuple(copy_synthesis(gen, a)[0]) == WAVE_KEYS and tuple(score32) == WAVE_KEYS + MR_STFT_KEYS[:3]
    vals, own = {}, {}
    for mode in ('bf16', 'bf16x3'):
        E.set_precision(mode)
        try:
            own[mode], out = copy_synthesis(gen, a, mr_stft=True)
        finally:
            E.set_precision('f32')
        assert tuple(own[mode]) == WAVE_KEYS + MR_STFT_KEYS[:3] and all(bool(torch.isfinite(own[mode][k])) for k in MR_STFT_KEYS[:3])
        vals[mode] = multi_resolution_stft(out, out32)                  # the mode's resynthesis against the fp32 one
    print('mr_stft of copy synthesis against its input (synthetic weights): fp32 %r, plain bf16 %r, split bf16 %r'
          % (float(score32['mr_stft']), float(own['bf16']['mr_stft']), float(own['bf16x3']['mr_stft'])))
    print('multi-resolution STFT distance of the resynthesis against the fp32 one (synthetic weights):',
          {k: (float(v['mr_stft']), v['per_resolution'].tolist()) for k, v in vals.items()})
    # plain bf16 lies further from the input than split bf16 does (both next to a generator with random weights: 9.8768 against 9.8757)
    # and, the sharper statement, further from the fp32 resynthesis (2.8e-2 against 5.1e-5)
    assert np.isfinite(float(own['bf16']['mr_stft'])) and float(own['bf16']['mr_stft']) > float(own['bf16x3']['mr_stft'])
    assert np.isfinite(float(vals['bf16']['mr_stft'])) and float(vals['bf16']['mr_stft']) > float(vals['bf16x3']['mr_stft']) >= 0.0
    assert all(bool(torch.isfinite(score32[k])) for k in MR_STFT_KEYS[:3])
