"""CPU: the true-peak arithmetic of include/ttsamd.h, on its numpy restatement tests/true_peak_ref.py: conformance on the EBU Tech 3341
true-peak signals, the properties of the interpolator and of the limiter with the true-peak detector, the level bound, the library's
tap table against the restatement's, and the host-side pieces (reach, stream halo, the `true_peak` switch's validation).  The kernels
are held to this restatement bit for bit in tests/test_gpu_true_peak.py."""
import ctypes as C

import numpy as np
import pytest

import limiter_ref as LR
import true_peak_ref as T
from utils.audio import true_peak, true_peak_db          # noqa: F401  (the public names exist; they run on the GPU only)

Q = LR.Q


def quarter_rate_sine(fs, amp, phase_deg, fade_ms=10.0):
    """one second of a sine at fs / 4 with a raised-cosine fade at both ends, so that the row's edges do not decide the reading"""
    n = np.arange(fs)
    x = amp * np.sin(2 * np.pi * n / 4 + np.deg2rad(phase_deg))
    k = int(round(fade_ms * fs / 1000.0))
    fade = 0.5 - 0.5 * np.cos(np.pi * (np.arange(k) + 0.5) / k)
    x[:k] *= fade
    x[-k:] *= fade[::-1]
    return x.astype(np.float32)


# EBU Tech 3341 (2016), table 3, cases 15 - 19: the reading and the document's tolerance of +0.2 / -0.4 dB
EBU_CASES = [(0.5, 0.0, -6.0), (0.5, 45.0, -6.0), (0.5, 60.0, -6.0), (0.5, 67.5, -6.0), (1.41, 45.0, 3.0)]


@pytest.mark.parametrize('fs', [22050, 48000])
@pytest.mark.parametrize('amp,phase,want', EBU_CASES)
def test_ebu_tech_3341_true_peak_signals(fs, amp, phase, want):
    x = quarter_rate_sine(fs, amp, phase)
    got = T.true_peak_db(x)
    print(f'fs {fs}, amplitude {amp}, phase {phase}: {got:+.4f} dBTP (sample peak {20 * np.log10(np.abs(x).max()):+.4f} dBFS), expected {want:+.1f}')
    assert want - 0.4 <= got <= want + 0.2


def test_table():
    from ttsamd import lib
    from ttsamd.engine import true_peak_taps
    from ttsamd.resample import resample_taps
    assert T.TAPS.shape == (3, 25) and T.TAPS.dtype == np.float32
    assert np.abs(T.TAPS).max() <= 1.0                                   # |h| <= 1: an impulse's true peak is the impulse
    taps, width, o, n = resample_taps(1, 4, 12, 1.0)
    assert (width, o, n) == (12, 1, 4) and np.array_equal(taps[1:], T.TAPS)
    # phase 0 of the table is the sample up to sin(k pi) != 0 in float64: why the true peak takes the sample itself there
    assert taps[0][12] == 1.0 and np.abs(np.delete(taps[0], 12)).max() < 1e-16
    got = true_peak_taps()                                               # the table the kernels get, from the library (no GPU)
    assert got.shape == (3, 25) and got.dtype == np.float64 and np.array_equal(got, T.TAPS.astype(np.float64))
    assert 2.0 < T.H < 2.5
    h = lib.load()
    assert h.ttsamd_true_peak_taps(C.POINTER(C.c_double)()) == -1 and b'true_peak_taps' in h.ttsamd_last_error()


def test_phase_and_position_properties():
    rng = np.random.default_rng(1)
    for n in (0, 1, 12, 13, 300):
        x = rng.uniform(-0.9, 0.9, n).astype(np.float32)
        tp = T.true_peak(x)
        assert tp.dtype == np.float32 and float(tp) >= (float(np.abs(x).max()) if n else 0.0)
        assert float(tp) >= T.true_peak64(x) and float(np.nextafter(tp, np.float32(0))) < T.true_peak64(x) or n == 0
        assert float(T.true_peak(np.zeros(n, np.float32))) == 0.0
    assert float(T.true_peak(np.zeros(0, np.float32))) == 0.0
    for n, at in ((1, 0), (40, 0), (40, 39), (40, 17)):
        x = np.zeros(n, np.float32)
        x[at] = 1.0
        assert float(T.true_peak(x)) == 1.0
    # positions: the tail behind the last sample counts, nothing in front of sample 0 does
    x = np.zeros(30, np.float32)
    x[0], x[1] = 1.0, 1.0
    v = T.interpolate(x)
    assert v.shape == (30, 3) and abs(v[0]).max() > 1.0                  # between the two ones
    y = np.zeros(30, np.float32)
    y[-1] = -0.5
    assert np.array_equal(T.interpolate(y)[-1], -0.5 * T.TAPS[:, 12].astype(np.float64))
    # upward rounding
    assert T.ceil32(1.0 + 2.0 ** -40) == np.nextafter(np.float32(1), np.float32(2)) and T.ceil32(0.75) == np.float32(0.75)


def _noise(n, seed, amp=0.9):
    return np.random.default_rng(seed).uniform(-amp, amp, n).astype(np.float32)


@pytest.mark.parametrize('A,R', [(5, 40), (0, 0), (7, 7)])
def test_limiter_properties_on_the_restatement(A, R):
    c = np.float32(0.99)
    x = _noise(700, 3)
    x[300:420] *= np.float32(0.05)                                       # a quiet stretch longer than the reach
    g = np.float32(1.3)
    r = T.curves(x, g, c, A, R)
    u, d, y = r['u'], r['d'], r['y']
    assert np.abs(y).max() <= c and (d >= np.abs(u)).all() and (d > np.abs(u)).any()
    assert (r['q'] <= LR.q_plane(u, c)).all()                            # the detector only ever asks for more reduction
    over = d > np.float64(c)
    assert over.any()
    free = np.array([not over[max(i - A - R, 0):i + 2 * A + 1].any() for i in range(len(x))])
    assert free.any() and np.array_equal(LR.bits(y[free]), LR.bits(u[free]))
    assert (r['s'][~free] < Q).all()
    # the reach: y[i] depends on x over [i - A - R - 13, i + 2A + 13] only
    rng = np.random.default_rng(4)
    for i in (0, 1, 13, 250, 351, 699):
        lo, hi = max(i - A - R - T.REACH, 0), min(i + 2 * A + T.REACH, len(x) - 1)
        x2 = rng.uniform(-0.9, 0.9, len(x)).astype(np.float32)
        x2[lo:hi + 1] = x[lo:hi + 1]
        assert LR.bits(T.limit(x2, g, c, A, R)[0][i:i + 1]) == LR.bits(y[i:i + 1]), i
    # one sample further out on either side does reach y[i] somewhere: the interval is not wider than it has to be by more than 1
    x3 = np.zeros(200, np.float32)
    x3[100], x3[101] = 0.9, 0.9                                          # an inter-sample peak above the ceiling between 100 and 101
    r3 = T.curves(x3, np.float32(1.0), c, A, R)
    assert np.abs(x3).max() < c and r3['s'].min() < Q and (r3['s'][[100, 101]] < Q).all()


def _level_mode2_capped(x, c):
    """ttsamd_wave_level's mode 2 where the cap decides, with the true peak as its peak: g = fl32(c / TP), one fp32 step down if
    fl32(TP g) > c; y = fl32(x g)"""
    tp = T.true_peak(x)
    g = np.float32(np.float64(c) / np.float64(tp))
    if np.float32(tp * g) > c:
        g = np.nextafter(g, np.float32(0))
    return (x * g).astype(np.float32)


def test_level_bound():
    c = np.float32(0.99)
    for name, x in (('fs / 4 at 45 degrees', quarter_rate_sine(22050, 0.5, 45.0)), ('noise', _noise(5000, 9, 0.3))):
        y = _level_mode2_capped(x, c)
        tp = T.true_peak64(y)
        print(f'{name}: true peak {T.true_peak64(x):.7f} -> {tp:.9f}, sample peak {np.abs(y).max():.7f}; bound {T.level_bound(c):.9f}')
        assert tp <= T.level_bound(c) and tp > 0.98
    assert np.abs(_level_mode2_capped(quarter_rate_sine(22050, 0.5, 45.0), c)).max() < 0.72        # about 3 dB under the ceiling


def test_reach_and_switch_validation():
    from ttsamd.engine import TRUE_PEAK_REACH, check_true_peak, limiter_reach
    from ttsamd.stream import limiter_halo_frames
    assert TRUE_PEAK_REACH == T.REACH == 13
    assert limiter_reach(33, 331) == (364, 66) and limiter_reach(33, 331, true_peak=True) == (377, 79)
    assert limiter_halo_frames(33, 331, 256) == 2 and limiter_halo_frames(33, 331, 256, True) == 2
    assert limiter_halo_frames(0, 0, 256, True) == 1 and limiter_halo_frames(100, 400, 256, True) == 3 and limiter_halo_frames(100, 400, 256) == 2
    assert check_true_peak(False, None, None) is False and check_true_peak(True, 'lufs', None) is True
    assert check_true_peak(True, None, True) is True and check_true_peak(True, [None, -16.0], False) is True
    for bad in (dict(true_peak=True, normalize=None, limiter=None), dict(true_peak=True, normalize=[None, None], limiter=False),
                dict(true_peak=1, normalize='lufs', limiter=None), dict(true_peak='yes', normalize='lufs', limiter=None)):
        with pytest.raises(ValueError):
            check_true_peak(**bad)
