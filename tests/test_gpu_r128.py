"""The loudness meter on the GPU (pytest -m gpu): ttsamd_loudness_meter and the stream meter ttsamd_meter_* (csrc/loudness.hip), the
utils.audio surface and tts_stream(meter=True), against the float64 restatement tests/r128_ref.py.

Tolerances.  L_TOL = 1e-9 LU on every loudness (what tests/test_gpu_loudness.py holds the integrated loudness to: the float64 floor of
the energies is three orders below), 2 L_TOL on the range (a difference of two values); counts, peak: exact.  Integrated loudness and
peak of the whole-wave meter: the bits of ttsamd_loudness_measure.  A value that sits on a gate flips a count, so every row is checked
on the CPU, before any device call, to keep its blocks at least 1e-6 LU from the gates of the integrated loudness (gate_margin) and its
short-term values at least 1e-6 LU from the gates of the range (lra_margin).

The floor.  Behind a passage of signal the filter rings out: a window of digital silence reads -900 LUFS and less (the program row has
4 s of zeros).  Those values are the float64 rounding noise of the filter state at the level of the signal before them, 2^-53 of it,
seen from far below: two float64 filters (scipy's sequential one and the kernels' scan) agree on a window that lies D dB under the
row's loudest one within about 10 * 8.7 * 2^-53 * 10^(D / 20) LU, which passes 1e-9 LU at D = 94 dB.  So a series value is held to L_TOL
where the restatement has it within FLOOR_DB = 90 dB of the row's maximum momentary loudness (every window that holds signal, the
sigma 0.0002 passage at -54 dB included); under that the device value has to be under the floor as well."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import loudness_ref as R
import r128_ref as X
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EINVAL = -1
L_TOL = 1e-9
FLOOR_DB = 90.0
FS = 22050


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


def _ref(x, fs):
    m = X.meter(x, fs)
    assert R.gate_margin(m) >= 1e-6 and X.lra_margin(m) >= 1e-6, (len(x), fs, R.gate_margin(m), X.lra_margin(m))
    return m


@pytest.fixture(scope='module')
def rows():
    """{name: (samples, rate, restatement)}, computed once and left unchanged"""
    out = {'program': (X.program_row(), FS)}
    for n in X.EDGE_LENGTHS:
        out[f'edge{n}'] = (X.edge_row(n), FS)
    out['long8k'] = (X.long_row(), 8000)
    for n in (143999, 144000, 148800):                       # 3 s at 48 000 Hz: one sample short, one S, two S
        out[f'edge48k_{n}'] = ((np.random.default_rng(7).standard_normal(n) * 0.1).astype(np.float32), 48000)
    return {k: (x, fs, _ref(x, fs)) for k, (x, fs) in out.items()}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _poisoned(xs, dev):
    stride = max(1, max(len(x) for x in xs))
    buf = np.full((len(xs), stride), np.nan, dtype=np.float32)
    for b, x in enumerate(xs):
        buf[b, :len(x)] = x
    return torch.from_numpy(buf).to(dev), torch.tensor([len(x) for x in xs], dtype=torch.int64, device=dev)


def _meter(xs, dev, fs):
    """-> (dict of numpy arrays of LoudnessEngine.meter(series=True), (loudness, peak) of LoudnessEngine.measure) on the same buffer"""
    from ttsamd.engine import leveller
    wave, lens = _poisoned(xs, dev)
    eng = leveller(fs, dev)
    m = eng.meter(wave, lens, series=True)
    loud, peak = eng.measure(wave, lens)
    return {k: v.cpu().numpy() for k, v in m.items()}, (loud.cpu().numpy(), peak.cpu().numpy())


def _same(a, r):
    """within L_TOL of a finite reference value; equal to one that is not (-inf)"""
    return a == r if not np.isfinite(r) else abs(a - r) < L_TOL


def _series_diff(a, r, floor):
    """largest difference over the reference values at and above the floor; where the reference is under it, so is the device"""
    a, r = np.atleast_1d(a), np.atleast_1d(r)
    held = r >= floor
    assert (a[~held] < floor + 1e-3).all()
    return float(np.abs(a[held] - r[held]).max()) if held.any() else 0.0


def _check_row(got, b, ref, what):
    J, JS = len(ref['M']), len(ref['S'])
    assert got['counts'][b].tolist() == [J, JS], what
    M, S = got['momentary'][b], got['short_term'][b]
    assert np.isnan(M[J:]).all() and np.isnan(S[JS:]).all(), what          # the sentinel: nothing written past the row's count
    floor = ref['max_momentary'] - FLOOR_DB
    dm, ds = _series_diff(M[:J], ref['M'], floor), _series_diff(S[:JS], ref['S'], floor)
    dl = abs(got['loudness_range'][b] - ref['lra'])
    print(f'{what}: {J} M / {JS} S values, max |dM| {dm:.2e}, max |dS| {ds:.2e}, maxima {got["max_momentary"][b]:.9f} / '
          f'{got["max_short_term"][b]:.9f}, LRA {got["loudness_range"][b]:.9f} (restatement {ref["lra"]:.9f}, difference {dl:.2e})')
    assert dm < L_TOL and ds < L_TOL, what
    assert _same(got['max_momentary'][b], ref['max_momentary']) and _same(got['max_short_term'][b], ref['max_short_term']), what
    assert dl < 2 * L_TOL, what
    assert _same(got['integrated'][b], ref['L']), what


def test_rows_alone(dev, rows):
    for name, (x, fs, ref) in rows.items():
        if fs != FS:
            continue
        got, (loud, peak) = _meter([x], dev, fs)
        _check_row(got, 0, ref, name)
        assert got['integrated'].view(np.int64)[0] == loud.view(np.int64)[0] and got['peak'][0] == peak[0] == ref['peak'], name


def test_ragged_batch_has_the_bits_of_the_rows_alone(dev, rows):
    names = [k for k, (_, fs, _) in rows.items() if fs == FS]
    xs = [rows[k][0] for k in names]
    got, (loud, peak) = _meter(xs, dev, FS)
    again, _ = _meter(xs, dev, FS)
    for k in got:
        assert np.array_equal(got[k], again[k], equal_nan=True), k
    assert np.array_equal(got['integrated'].view(np.int64), loud.view(np.int64)) and np.array_equal(got['peak'], peak)
    for b, name in enumerate(names):
        alone, _ = _meter([xs[b]], dev, FS)
        _check_row(got, b, rows[name][2], f'{name} in the batch')
        for k in ('integrated', 'loudness_range', 'max_momentary', 'max_short_term', 'peak', 'counts'):
            assert got[k][b].tobytes() == alone[k][0].tobytes(), (name, k)
        J, JS = got['counts'][b]
        assert got['momentary'][b, :J].tobytes() == alone['momentary'][0, :J].tobytes(), name
        assert got['short_term'][b, :JS].tobytes() == alone['short_term'][0, :JS].tobytes(), name


def test_other_sample_rates(dev, rows):
    for name, (x, fs, ref) in rows.items():
        if fs == FS:
            continue
        got, (loud, peak) = _meter([x], dev, fs)
        _check_row(got, 0, ref, name)
        assert got['integrated'].view(np.int64)[0] == loud.view(np.int64)[0] and got['peak'][0] == peak[0] == ref['peak'], name
    assert rows['long8k'][2]['k'] > 1024 and len(rows['long8k'][2]['S']) == 1101          # crosses a tile of the rank count
    assert [len(rows[f'edge48k_{n}'][2]['S']) for n in (143999, 144000, 148800)] == [0, 1, 2]


# ---- the stream meter ----
def _sizes(n, chunk):
    return [min(chunk, n - p) for p in range(0, n, chunk)]


CHUNKINGS = {'whole': lambda n: [n], '16384': lambda n: _sizes(n, 16384), '777': lambda n: _sizes(n, 777),
             'mixed': lambda n: [0, 5, 0, 62, 1, 2205, 0, 8820, 30000] + _sizes(max(n - 41093, 0), 50001) + [0]}


def _push_all(meter, xs, sizes, slots, dev):
    """push rows xs together in chunks of `sizes` (a row that has ended goes on with empty chunks) -> readings [pushes][3][rows]"""
    pos, out = 0, []
    for c in sizes:
        buf = np.full((len(xs), max(c, 1)), np.nan, dtype=np.float32)
        lens = []
        for b, x in enumerate(xs):
            part = x[pos:pos + c]
            buf[b, :len(part)] = part
            lens.append(len(part))
        r = meter.push(torch.from_numpy(buf).to(dev), torch.tensor(lens, dtype=torch.int64), slots)
        out.append(torch.stack([r['momentary'], r['short_term'], r['integrated']]))
        pos += c
    return torch.stack(out).cpu().numpy()


@pytest.mark.parametrize('chunking', list(CHUNKINGS))
def test_stream_meter(dev, rows, chunking):
    from utils.audio import LoudnessMeter
    xs = [rows['program'][0], rows['edge66150'][0]]
    refs = [rows['program'][2], rows['edge66150'][2]]
    sizes = CHUNKINGS[chunking](len(xs[0]))
    assert sum(sizes) >= len(xs[0])
    lm = LoudnessMeter(FS, max_streams=4, max_seconds=20.0, device=dev)
    together = _push_all(lm, xs, sizes, [2, 0], dev)
    res = {k: v.cpu().numpy() for k, v in lm.result([2, 0]).items()}
    cms = [X.ChunkedMeter(FS), X.ChunkedMeter(FS)]
    pos = 0
    for i, c in enumerate(sizes):                            # after each push: the reference's values for the samples so far
        for b in range(2):
            want = cms[b].push(xs[b][pos:pos + c])
            for j, k in enumerate(('momentary', 'short_term', 'integrated')):
                assert _series_diff(together[i, j, b], want[k], refs[b]['max_momentary'] - FLOOR_DB) < L_TOL, (chunking, i, b, k, together[i, j, b], want[k])
        pos += c
    for b, ref in enumerate(refs):
        assert res['counts'][b].tolist() == [len(ref['M']), len(ref['S'])] and res['peak'][b] == ref['peak'] and res['status'][b] == 0
        for k, rk in (('integrated', 'L'), ('max_momentary', 'max_momentary'), ('max_short_term', 'max_short_term')):
            assert _same(res[k][b], ref[rk]), (chunking, b, k, res[k][b], ref[rk])
        assert abs(res['loudness_range'][b] - ref['lra']) < 2 * L_TOL
        print(f'{chunking}, row {b}: {len(sizes)} pushes, L {res["integrated"][b]:.9f} (restatement {ref["L"]:.9f}), LRA '
              f'{res["loudness_range"][b]:.9f} ({ref["lra"]:.9f})')
    # each stream alone, with the same chunking, in a slot that was used and reset: the same bits
    lm.reset([2])
    for b in range(2):
        alone = _push_all(lm, [xs[b]], sizes, [2], dev)
        assert alone[:, :, 0].tobytes() == together[:, :, b].tobytes(), (chunking, b)
        ra = {k: v.cpu().numpy() for k, v in lm.result([2]).items()}
        for k in res:
            assert ra[k][0].tobytes() == res[k][b].tobytes(), (chunking, b, k)
        lm.reset([2])


def test_stream_short_row_and_overflow(dev, rows):
    from utils.audio import LoudnessMeter
    x, _, ref = rows['edge3000']
    lm = LoudnessMeter(FS, max_streams=2, max_seconds=1.0, device=dev)
    r = _push_all(lm, [x], [1000, 0, 2000], [1], dev)
    assert np.isneginf(r).all()                              # no whole block yet: the short-row rule is result's
    res = {k: v.cpu().numpy() for k, v in lm.result([1, 0]).items()}
    assert res['counts'].tolist() == [[1, 0], [0, 0]] and res['peak'].tolist() == [float(ref['peak']), 0.0]
    assert abs(res['integrated'][0] - ref['L']) < L_TOL and abs(res['max_momentary'][0] - ref['max_momentary']) < L_TOL
    assert np.isneginf(res['max_short_term']).all() and np.isneginf(res['integrated'][1]) and not res['loudness_range'].any()
    # a push beyond max_seconds (22 050 samples): left out and flagged, the slot as it was
    big = torch.from_numpy(rows['edge66150'][0][:20000]).to(dev)
    lm.push(big, slots=[1])
    after = {k: v.cpu().numpy() for k, v in lm.result([1, 0]).items()}
    assert after['status'].tolist() == [LoudnessMeter_DROPPED(), 0]
    for k in res:
        if k != 'status':
            assert after[k].tobytes() == res[k].tobytes(), k
    with pytest.raises(ValueError):
        lm.push(big[None].repeat(2, 1), slots=[1, 1])
    with pytest.raises(ValueError):
        lm.push(big, slots=[2])


def LoudnessMeter_DROPPED():
    from ttsamd.engine import LoudnessMeter
    return LoudnessMeter.METER_DROPPED


# ---- refusals ----
def test_refusals(dev):
    from ttsamd import lib as L
    lib = L.load()
    n, B = 30000, 2
    wave = torch.zeros(B, n, device=dev)
    lens = torch.full((B,), n, dtype=torch.int64, device=dev)
    f64 = [torch.full((B,), 7.0, dtype=torch.float64, device=dev) for _ in range(4)]
    peak = torch.full((B,), 7.0, device=dev)
    counts = torch.full((B, 2), 7, dtype=torch.int64, device=dev)
    nbytes = int(lib.ttsamd_loudness_meter_workspace_bytes(B, n, FS))
    assert nbytes > 0 and lib.ttsamd_loudness_meter_workspace_bytes(B, n, 7999) == -1 == lib.ttsamd_loudness_meter_workspace_bytes(0, n, FS)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call(wave_=wave, fs=FS, nb=nbytes, loud=f64[0], stride_m=0, M=None):
        return lib.ttsamd_loudness_meter(_ptr(wave_), n, _ptr(lens), B, fs, _ptr(loud), _ptr(peak), _ptr(f64[1]), _ptr(f64[2]), _ptr(f64[3]),
                                         _ptr(counts), _ptr(M), stride_m, None, 0, _ptr(ws), nb, _stream())
    assert call(wave_=None) == EINVAL and call(loud=None) == EINVAL
    assert call(fs=7999) == EINVAL and call(fs=192001) == EINVAL
    assert call(nb=nbytes - 1) == EINVAL
    M = torch.zeros(B, 10, dtype=torch.float64, device=dev)
    assert call(M=M, stride_m=9) == EINVAL                   # a 30 000-sample stride has 10 momentary values
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in f64 + [peak, counts])         # nothing was launched
    assert call() == 0 and call(M=M, stride_m=10) == 0
    # the stream meter
    assert lib.ttsamd_meter_state_bytes(0, 22050, FS) == -1 == lib.ttsamd_meter_state_bytes(2, 0, FS) == lib.ttsamd_meter_state_bytes(2, 22050, 7999)
    sb = int(lib.ttsamd_meter_state_bytes(2, 22050, FS))
    state = torch.zeros(sb, dtype=torch.uint8, device=dev)
    slots = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    pws = int(lib.ttsamd_meter_push_workspace_bytes(B, n, FS))
    pw = torch.empty(pws, dtype=torch.uint8, device=dev)

    def push(st=state, sbytes=sb, fs=FS, sl=slots, nb=pws, out=f64[0]):
        return lib.ttsamd_meter_push(_ptr(st), sbytes, 2, 22050, fs, _ptr(wave), n, _ptr(lens), _ptr(sl), B, _ptr(out), _ptr(f64[1]), _ptr(f64[2]),
                                     _ptr(pw), nb, _stream())
    assert lib.ttsamd_meter_reset(_ptr(state), sb, 2, 22050, FS, _ptr(slots), 2, _stream()) == 0
    for t in f64:
        t.fill_(7.0)
    assert push(st=None) == EINVAL and push(sl=None) == EINVAL and push(out=None) == EINVAL
    assert push(fs=7999) == EINVAL and push(fs=192001) == EINVAL
    assert push(nb=pws - 1) == EINVAL and push(sbytes=sb - 1) == EINVAL
    assert lib.ttsamd_meter_reset(_ptr(state), sb - 1, 2, 22050, FS, _ptr(slots), 2, _stream()) == EINVAL
    assert lib.ttsamd_meter_result(_ptr(state), sb, 2, 22050, FS, _ptr(slots), 2, None, _ptr(f64[1]), _ptr(f64[2]), _ptr(f64[3]), _ptr(peak),
                                   _ptr(counts), _ptr(counts), _stream()) == EINVAL
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in f64[:3])


# ---- utils.audio ----
def test_loudness_stats_takes_a_list_and_a_batch(dev, rows):
    from utils import audio
    names = ['edge66150', 'program', 'edge3000']
    xs = [rows[k][0] for k in names]
    as_list = audio.loudness_stats([torch.from_numpy(x) for x in xs])
    wave, lens = _poisoned(xs, dev)
    as_batch = audio.loudness_stats(wave, lens=lens)
    assert sorted(as_list) == ['integrated', 'loudness_range', 'max_momentary', 'max_short_term', 'peak']
    for k in as_list:
        assert as_list[k].device.type == 'cuda' and torch.equal(as_list[k], as_batch[k]), k
    for b, name in enumerate(names):
        ref = rows[name][2]
        assert abs(float(as_list['integrated'][b]) - ref['L']) < L_TOL and abs(float(as_list['loudness_range'][b]) - ref['lra']) < 2 * L_TOL
    M, cm = audio.momentary_loudness(wave, lens=lens)
    S, cs = audio.short_term_loudness(wave, lens=lens)
    assert cm.tolist() == [len(rows[k][2]['M']) for k in names] and cs.tolist() == [len(rows[k][2]['S']) for k in names]
    ref = rows['program'][2]
    floor = ref['max_momentary'] - FLOOR_DB
    assert _series_diff(M[1, :len(ref['M'])].cpu().numpy(), ref['M'], floor) < L_TOL
    assert _series_diff(S[1, :len(ref['S'])].cpu().numpy(), ref['S'], floor) < L_TOL
    assert torch.equal(audio.loudness_range(wave, lens=lens), as_batch['loudness_range'])


def test_normalize_loudness_with_a_short_term_cap(dev, rows):
    from utils import audio
    prog, _, ref = rows['program']
    assert abs(ref['max_short_term'] + 17.06) < 0.005 and abs(ref['L'] + 20.0) < 0.01       # -3 dB to -23: maxS -20.06, the cap is idle
    bind = X.binding_row()
    rb = _ref(bind, FS)
    assert rb['L'] + (-18.0 - rb['max_short_term']) < -23.0, (rb['L'], rb['max_short_term'])
    wave, lens = _poisoned([prog, bind], dev)
    wave = torch.nan_to_num(wave)
    plain = audio.normalize_loudness(wave, target_lufs=-23.0, lens=lens)
    capped = audio.normalize_loudness(wave, target_lufs=-23.0, lens=lens, max_short_term=-18.0)
    assert torch.equal(plain[0].view(torch.int32), capped[0].view(torch.int32))
    stats = audio.loudness_stats(capped, lens=lens)
    got = float(stats['max_short_term'][1])
    print(f'binding row: L {rb["L"]:.4f}, max S {rb["max_short_term"]:.4f} -> max S {got:.6f} after the call, L {float(stats["integrated"][1]):.4f}')
    assert abs(got + 18.0) < 1e-4
    assert float(audio.loudness_stats(plain, lens=lens)['max_short_term'][1]) > -18.0 + 0.1


# ---- through the model ----
@pytest.fixture(scope='module')
def model(tmp_path_factory, synth_weights, dev):
    import text
    from models.fastpitch import FastPitch2Wave
    from ttsamd.config import HIFIGAN_CONFIG, NET_CONFIG
    d = tmp_path_factory.mktemp('ckpt_r128')
    torch.save({'model': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['fastpitch'].items()}, 'config': dict(NET_CONFIG),
                'symbols': list(text.symbols)}, d / 'fp.pth')
    torch.save({'generator': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['hifigan'].items()}}, d / 'hg.pth')
    with open(d / 'config.json', 'w') as f:
        json.dump(HIFIGAN_CONFIG, f)
    return FastPitch2Wave(str(d / 'fp.pth'), vocoder_sd=str(d / 'hg.pth'), vocoder_config=str(d / 'config.json')).to(dev)


def test_tts_stream_with_a_meter(model):
    with open(os.path.join(GOLDEN, 'infer_text_lines.json'), encoding='utf-8') as f:
        every = json.load(f)
    lines = [every[i] for i in (68, 14)]
    kw = dict(chunk_frames=16, first_chunk_frames=8, denoise=0.0)
    with pytest.raises(ValueError):
        list(model.tts_stream(lines[0], meter=True, pcm16=True, **kw))
    with pytest.raises(ValueError):
        list(model.tts_stream(lines[0], meter=True, encoding='mulaw', sample_rate=8000, **kw))
    plain = list(model.tts_stream(lines[0], **kw))
    metered = list(model.tts_stream(lines[0], meter=True, **kw))
    assert len(plain) == len(metered) and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, (b, _) in zip(plain, metered))
    last = metered[-1][1]
    assert sorted(last) == ['integrated', 'loudness_range', 'max_momentary', 'max_short_term', 'momentary', 'short_term']
    assert sorted(metered[0][1]) == ['integrated', 'momentary', 'short_term'] and all(isinstance(v, float) for v in last.values())
    ref = X.chunked(torch.cat(plain).numpy(), FS, [int(c.numel()) for c in plain]).result()
    print(f'tts_stream(meter=True): {len(plain)} chunks, {sum(int(c.numel()) for c in plain)} samples, integrated {last["integrated"]:.9f} '
          f'(restatement {ref["L"]:.9f})')
    assert R.gate_margin(ref) >= 1e-6
    assert np.isfinite(ref['L']) and abs(last['integrated'] - ref['L']) < L_TOL
    assert abs(last['max_momentary'] - ref['max_momentary']) < L_TOL
    # a list: (i, chunk, last, reading), the lines' own figures
    parts, final = {0: [], 1: []}, {}
    for i, chunk, end, reading in model.tts_stream(lines, meter=True, max_streams=2, **kw):
        parts[i].append(chunk)
        if end:
            final[i] = reading
    for i in range(2):
        want = _ref(torch.cat(parts[i]).numpy(), FS)
        assert abs(final[i]['integrated'] - want['L']) < L_TOL, i
