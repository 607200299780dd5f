"""CPU: the numpy restatement of csrc/join.hip (tests/join_ref.py) pinned against plain numpy, so that tests/test_gpu_join.py can trust
it; and the host helpers of ttsamd/join.py that need no device."""
import numpy as np
import pytest

import join_ref as J


def _rows(lengths, seed=0, width=None):
    rng = np.random.default_rng(seed)
    width = max(max(lengths), 1) if width is None else width
    wave = rng.standard_normal((len(lengths), width)).astype(np.float32)
    return wave, np.array(lengths, dtype=np.int64)


def test_no_fade_and_gaps_is_concatenate_with_zero_runs():
    lengths, gaps, lead = [5, 0, 17, 1, 9], [3, 2, 0, 4, 6], 2
    wave, ns = _rows(lengths)
    out, segs, total = J.join(wave, ns, None, gaps, None, 0, lead, 80)
    parts = [np.zeros(lead, np.float32)]
    for b, n in enumerate(lengths):
        parts += [wave[b, :n], np.zeros(gaps[b], np.float32)]
    want = np.concatenate(parts)
    assert total == want.size == lead + sum(lengths) + sum(gaps)
    assert np.array_equal(out[:total], want) and not out[total:].any()
    starts = lead + np.concatenate([[0], np.cumsum(np.array(lengths) + np.array(gaps))[:-1]])
    assert np.array_equal(segs[:, 0], starts) and np.array_equal(segs[:, 1] - segs[:, 0], lengths)
    assert np.array_equal(segs[:, 2], np.zeros(5)) and np.array_equal(segs[:, 3], lengths)


def test_bounds_and_keep_are_clamped_to_the_row():
    wave, ns = _rows([40, 40, 40, 40], width=50)
    bounds = np.array([[10, 30], [0, 40], [3, 38], [0, 0]], dtype=np.int64)
    _, segs, total = J.join(wave, ns, bounds, [0, 0, 0, 0], None, 7, 0, 200)
    assert segs[:, 2:].tolist() == [[3, 37], [0, 40], [0, 40], [0, 0]]           # widened by 7, clamped at 0 and at the row's length
    assert total == 34 + 40 + 40
    # bounds past the row, reversed, negative: clamped to 0 <= s <= e <= n
    bad = np.array([[-5, 99], [30, 10], [45, 48], [41, 41]], dtype=np.int64)
    _, segs, _ = J.join(wave, ns, bad, [0, 0, 0, 0], None, 0, 0, 200)
    assert segs[:, 2:].tolist() == [[0, 40], [30, 30], [40, 40], [40, 40]]
    # nsamples is clamped to the stride
    _, segs, _ = J.join(wave, np.array([60, -3, 50, 1]), None, [0, 0, 0, 0], None, 0, 0, 200)
    assert segs[:, 2:].tolist() == [[0, 50], [0, 0], [0, 50], [0, 1]]


@pytest.mark.parametrize('F', [0, 1, 4, 16])
def test_total_follows_the_formula(F):
    lengths, gaps, lead = [30, 7, 0, 12, 3], [-4, 5, -2, -100, -9], 3
    wave, ns = _rows(lengths)
    _, segs, total = J.join(wave, ns, None, gaps, J.fade_table(F), 0, lead, 10)
    m, p = lengths, lead
    for b in range(5):
        assert segs[b, 0] == p and segs[b, 1] == p + m[b]
        if gaps[b] >= 0:
            g = gaps[b]
        elif b == 4:
            g = 0                                                  # the last row's negative gap
        else:
            g = -min(-gaps[b], F, m[b] // 2, m[b + 1] // 2)
        p += m[b] + g
    assert total == p                                              # unclamped: out_stride was 10


def test_a_negative_gap_is_the_sum_of_exactly_two_faded_rows():
    F, lengths = 8, [40, 50]
    wave, ns = _rows(lengths)
    fade = J.fade_table(F)
    out, segs, total, count = J.join(wave, ns, None, [-8, 0], fade, 0, 0, 100, return_count=True)
    assert total == 40 + 50 - 8 and segs[1, 0] == 32
    y = []
    for b, n in enumerate(lengths):
        r = wave[b, :n].copy()
        r[:F] = r[:F] * fade
        r[n - F:] = r[n - F:] * fade[::-1]
        y.append(r)
    assert np.array_equal(out[:32], y[0][:32]) and np.array_equal(out[40:82], y[1][8:])
    assert np.array_equal(out[32:40], y[0][32:] + y[1][:8])                       # fp32 + fp32, rounded once
    assert count[:82].tolist() == [1] * 32 + [2] * 8 + [1] * 42
    # fades of a row shorter than 2 F overlap inside it: both factors on one sample
    out1, _, _ = J.join(wave[:1], np.array([5]), None, [0], fade, 0, 0, 8)
    want = np.array([np.float32(np.float32(wave[0, i] * fade[i]) * fade[4 - i]) for i in range(5)], dtype=np.float32)
    assert np.array_equal(out1[:5], want)


def test_never_three_contributors():
    """a 3-sample row between two long ones, every gap asking for far more overlap than there is"""
    F = 64
    wave, ns = _rows([500, 3, 500])
    out, segs, total, count = J.join(wave, ns, None, [-64, -64, -64], J.fade_table(F), 0, 0, 1100, return_count=True)
    assert segs[:, 0].tolist() == [0, 499, 501] and total == 1001                 # overlaps of 3 // 2 = 1 on both sides of the short row
    assert count.max() == 2 and count[:total].min() == 1 and not count[total:].any()
    for lengths in ([9, 2, 2, 9], [100, 1, 100], [7, 0, 7], [64, 65, 3, 2, 1, 0, 1, 200]):
        wave, ns = _rows(lengths)
        *_, count = J.join(wave, ns, None, [-4096] * len(lengths), J.fade_table(F), 0, 1, 600, return_count=True)
        assert count.max() <= 2, lengths


def test_truncation_keeps_the_prefix():
    wave, ns = _rows([20, 20, 20])
    full, _, total = J.join(wave, ns, None, [5, -3, 2], J.fade_table(3), 0, 1, 100)
    cut, _, total_cut = J.join(wave, ns, None, [5, -3, 2], J.fade_table(3), 0, 1, 30)
    assert total_cut == total == 1 + 60 + 5 - 3 + 2 and np.array_equal(cut, full[:30])


def test_fade_table_and_the_host_helpers():
    from ttsamd.join import DEFAULT_PAUSES, fade_table, gaps_for, ms_to_samples, pause_table
    for n in (0, 1, 2, 110, 4096):
        t = fade_table(n)
        assert t.dtype == np.float32 and t.shape == (n,) and np.array_equal(t, J.fade_table(n))
        if n:
            assert np.all(np.diff(t.astype(np.float64)) > 0) or n == 1
            assert 0 < t[0] and t[-1] < 1
            assert np.abs(t.astype(np.float64) + t[::-1] - 1.0).max() < 1e-7       # a table and its mirror add up to 1
    with pytest.raises(ValueError):
        fade_table(4097)
    assert ms_to_samples(5.0) == 110 and ms_to_samples(-5.0) == -110 and ms_to_samples(10.0) == 221 and ms_to_samples(0) == 0
    assert ms_to_samples(350, 22050) == 7718 and ms_to_samples(1000, 8000) == 8000
    table = pause_table(None, 5.0)
    assert table == dict(DEFAULT_PAUSES, forced=-5.0)
    assert pause_table({'sentence': 100, 'forced': 0}, 5.0)['forced'] == 0 and pause_table({'sentence': 100}, 2.0)['sentence'] == 100
    for bad in ({'phrase': 1.0}, {'comma': float('nan')}, {'comma': 'long'}):
        with pytest.raises(ValueError):
            pause_table(bad, 5.0)
    assert gaps_for(['sentence', 'forced', 'comma', 'end'], table) == [7718, -110, 3308, 0]
