"""The loudness meter's arithmetic on the CPU (tests/r128_ref.py, the float64 restatement the GPU tests hold the kernels to): the EBU
Tech 3342 loudness-range signals, a steady tone on all three time scales, the chunked meter against the whole-wave one, and the
percentile indices."""
import numpy as np
import pytest

import loudness_ref as R
import r128_ref as X

FS = 22050


def _sine(seconds, dbfs, fs=FS, f=1000.0):
    return (10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * f * np.arange(int(seconds * fs)) / fs)).astype(np.float32)


@pytest.mark.parametrize('levels, want', [((-20.0, -30.0), 10.0), ((-40.0, -20.0), 20.0)])
def test_tech_3342_range_signals(levels, want):
    """Tech 3342 cases 1 and 2: 20 s of a 1 kHz sine at each of two levels -> LRA within 1 LU of their distance; the restatement
    gives it to three decimals"""
    m = X.meter(np.concatenate([_sine(20, levels[0]), _sine(20, levels[1])]), FS)
    print(f'levels {levels}: LRA {m["lra"]:.6f} LU over {m["k"]} of {len(m["S"])} short-term values')
    assert abs(m['lra'] - want) <= 1.0
    assert round(m['lra'], 3) == want


def test_steady_sine_reads_the_same_on_every_scale():
    m = X.meter(_sine(6, -23.0), FS)
    assert len(m['M']) == 57 and len(m['S']) == 31
    for v in (m['M'], m['S']):
        assert np.abs(v - m['L']).max() < 0.1
    assert abs(m['max_momentary'] - m['L']) < 0.1 and abs(m['max_short_term'] - m['L']) < 0.1 and m['lra'] < 0.1


@pytest.mark.parametrize('chunk', [1, 777, 16384])
def test_chunked_meter_equals_the_whole_wave(chunk):
    """sequential filtering with carried state in chunks of any length: every figure within 1e-9 LU of the whole-wave restatement"""
    fs = 8000
    rng = np.random.default_rng(7)
    x = np.concatenate([(rng.standard_normal(int(d * fs)) * sg).astype(np.float32) for d, sg in ((1.5, 0.1), (1.0, 0.0002), (1.35, 0.03))])
    whole = X.meter(x, fs)
    assert len(whole['S']) == 9 and R.gate_margin(whole) > 1e-6 and X.lra_margin(whole) > 1e-6
    cm = X.chunked(x, fs, chunk)
    got = cm.result()
    assert cm.n == len(x) and got['peak'] == whole['peak']
    assert len(got['M']) == len(whole['M']) and len(got['S']) == len(whole['S'])
    assert np.abs(got['M'] - whole['M']).max() < 1e-9 and np.abs(got['S'] - whole['S']).max() < 1e-9
    for k in ('L', 'lra', 'max_momentary', 'max_short_term'):
        assert abs(got[k] - whole[k]) < 1e-9, k
    last = cm.reading()
    assert abs(last['momentary'] - whole['M'][-1]) < 1e-9 and abs(last['short_term'] - whole['S'][-1]) < 1e-9
    assert abs(last['integrated'] - whole['L']) < 1e-9


def test_chunked_meter_short_row_and_empty_pushes():
    x = X.edge_row(3000)
    cm = X.chunked(x, FS, [0, 1000, 0, 2000, 0])
    got, whole = cm.result(), X.meter(x, FS)
    assert len(got['M']) == 1 and abs(got['L'] - whole['L']) < 1e-9 and got['max_short_term'] == -np.inf and got['lra'] == 0.0
    assert cm.reading() == dict(momentary=-np.inf, short_term=-np.inf, integrated=-np.inf)
    assert X.ChunkedMeter(FS).result()['L'] == -np.inf


def test_percentile_indices():
    """round((k - 1) p) for p = 0.10 and 0.95, in integers"""
    assert [X.percentile_indices(k) for k in (1, 2, 11, 109)] == [(0, 0), (0, 1), (1, 10), (11, 103)]
    for k in (1, 2, 11, 109):
        lo, hi = X.percentile_indices(k)
        assert lo == int(np.floor((k - 1) * 0.10 + 0.5)) and hi == int(np.floor((k - 1) * 0.95 + 0.5))


def test_rows_of_the_gpu_tests_keep_off_the_gates():
    """the program row: 161 short-term values, 110 above -70, 109 above the relative gate, LRA 14.80 LU"""
    m = X.meter(X.program_row(), FS)
    assert len(m['S']) == 161 and int((m['S'] > -70.0).sum()) == 110 and m['k'] == 109
    assert abs(m['lra'] - 14.80) < 0.005 and X.lra_margin(m) > 0.4 and R.gate_margin(m) > 0.4
    for n, js in zip(X.EDGE_LENGTHS, (0, 0, 0, 0, 0, 1, 2)):
        e = X.meter(X.edge_row(n), FS)
        assert len(e['S']) == js and R.gate_margin(e) >= 1e-6 and X.lra_margin(e) >= 1e-6, n
