"""The paragraph join on the device (csrc/join.hip) and `tts_long` next to the route a caller had before it: `tts(list)`, then trim, fade and
concatenate on the host in numpy (profiles/r41/NOTES.md is written from its output).

Three measurements in one process, every case warmed up first and the cases alternating:
  join      ttsamd_wave_join alone on 32 rows x 5 s (110 250 samples each) of speech-like signal with given bounds, pauses of 350 ms and a
            5 ms fade: the median time of --iters back-to-back calls between two device events (two launches a call), and the rate over
            the bytes the arithmetic needs: every source sample inside the bounds read once, every output sample written once.
  tts_long  FastPitch2Wave.tts_long on a 32-sentence paragraph (the synthetic full-size checkpoints, 32 of the committed text lines joined
            with '. '), host clock around the call, which ends in its single copy to the host.
  host      the same 32 sentences through `tts(list, batch_size=32)` (32 copies to the host), then librosa.effects.trim's arithmetic
            (frame 1024, hop 256, 40 dB), the same fades and pauses and np.concatenate in numpy: the route before this feature.
Also reported: the bytes read back per join (segs and total: 8 (4 B + 1)) and the launches per join (trim bounds 2 + join 2, as the two
launchers issue them; this script does not count them with a profiler).  No ratio is required of any of it.

    python profiles/join_bench.py [--reps 7] [--warmup 2] [--iters 20] [--sentences 32] [--only join|tts] [--out FILE.jsonl]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tts-arabic-pytorch_amd'))
sys.path.insert(0, os.path.join(REPO, 'profiles'))

from griffinlim_bench import speech_like  # noqa: E402


def host_trim(y, top_db=40.0, frame=1024, hop=256):
    """librosa.effects.trim(y, top_db, ref=np.max, frame_length, hop_length) in numpy: (start, end)"""
    import numpy as np
    pad = np.pad(y, frame // 2)
    T = 1 + y.size // hop
    idx = np.arange(frame)[None, :] + hop * np.arange(T)[:, None]
    ms = np.maximum((pad[idx] ** 2).mean(axis=1), 1e-10)
    keep = np.flatnonzero(ms > 10.0 ** (-top_db / 10.0) * ms.max())
    if keep.size == 0:
        return 0, 0
    return int(keep[0]) * hop, min(y.size, (int(keep[-1]) + 1) * hop)


def host_join(waves, gaps, keep, fade):
    """the join in numpy on host waves: trim, keep, fade both edges, zeros between (no overlap: the pauses here are positive)"""
    import numpy as np
    parts, F = [], fade.size
    for w, g in zip(waves, gaps):
        w = w.numpy()
        s, e = host_trim(w)
        s, e = max(0, s - keep), min(w.size, e + keep)
        y = w[s:e].copy()
        if y.size >= F:
            y[:F] *= fade
            y[y.size - F:] *= fade[::-1]
        parts += [y, np.zeros(g, dtype=np.float32)]
    return np.concatenate(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--sentences', type=int, default=32)
    ap.add_argument('--only', choices=['join', 'tts'], default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from ttsamd import lib as L
    from ttsamd.join import fade_table, ms_to_samples

    assert torch.cuda.is_available(), 'join_bench needs an MI355X: a CPU run says nothing about time'
    dev = torch.device('cuda:0')
    row = dict(bench='join', reps=args.reps, iters=args.iters)
    cases = {}

    if args.only in (None, 'join'):
        B, n = 32, 110250
        wave = torch.from_numpy(speech_like(B, n)).to(dev)
        lens = torch.full((B,), n, dtype=torch.int64, device=dev)
        bounds = torch.tensor([[256 * (3 + b % 5), n - 256 * (2 + b % 7)] for b in range(B)], dtype=torch.int64).to(dev)
        gaps = torch.tensor([ms_to_samples(350.0)] * (B - 1) + [0], dtype=torch.int64).to(dev)
        fade = torch.from_numpy(fade_table(110)).to(dev)
        width = B * n + int(gaps.sum())
        out = torch.empty(width, dtype=torch.float32, device=dev)
        table = torch.empty(4 * B + 1, dtype=torch.int64, device=dev)
        h = L.load()
        p = lambda t: C.c_void_p(t.data_ptr())                                                   # noqa: E731
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def join():
            L.check(h.ttsamd_wave_join(p(wave), n, p(lens), p(bounds), p(gaps), B, p(fade), 110, 221, 0, p(out), width, p(table),
                                       C.c_void_p(table.data_ptr() + 32 * B), stream), 'wave_join')
        join()
        torch.cuda.synchronize()
        t = table.cpu()
        total = int(t[4 * B])
        src = int((t[:4 * B].reshape(B, 4)[:, 3] - t[:4 * B].reshape(B, 4)[:, 2]).sum())
        row.update(join_rows=B, join_samples_per_row=n, join_total_samples=total, join_out_stride=width,
                   join_bytes=4 * (src + width) + 8 * (4 * B + 1) + 8 * 4 * B, join_launches=2, join_readback_bytes=8 * (4 * B + 1))

        def timed_join():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                join()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / args.iters
        cases['join_ms'] = timed_join

    if args.only in (None, 'tts'):
        import text
        from models.fastpitch import FastPitch2Wave
        from ttsamd import synth
        from ttsamd.config import HIFIGAN_CONFIG, NET_CONFIG
        with open(os.path.join(REPO, 'tests', 'golden', 'infer_text_lines.json'), encoding='utf-8') as f:
            every = json.load(f)
        lines = sorted(every, key=len)[:args.sentences]
        with tempfile.TemporaryDirectory() as d:
            torch.save({'model': {k: torch.from_numpy(np.array(v)) for k, v in synth.fastpitch_state_dict().items()}, 'config': dict(NET_CONFIG),
                        'symbols': list(text.symbols)}, os.path.join(d, 'fp.pth'))
            torch.save({'generator': {k: torch.from_numpy(np.array(v)) for k, v in synth.hifigan_state_dict().items()}}, os.path.join(d, 'hg.pth'))
            with open(os.path.join(d, 'config.json'), 'w') as f:
                json.dump(HIFIGAN_CONFIG, f)
            model = FastPitch2Wave(os.path.join(d, 'fp.pth'), vocoder_sd=os.path.join(d, 'hg.pth'), vocoder_config=os.path.join(d, 'config.json')).to(dev)
        paragraph = '. '.join(lines)
        pause, keep, fade_np = ms_to_samples(350.0), ms_to_samples(10.0), fade_table(110)
        res = {}

        def tts_long():
            t0 = time.perf_counter()
            res['long'] = model.tts_long(paragraph, batch_size=32)
            return (time.perf_counter() - t0) * 1e3

        def host_route():
            t0 = time.perf_counter()
            waves = model.tts(lines, batch_size=32)
            t1 = time.perf_counter()
            res['host'] = host_join(waves, [pause] * (len(lines) - 1) + [0], keep, fade_np)
            res['host_join_ms'] = (time.perf_counter() - t1) * 1e3
            return (time.perf_counter() - t0) * 1e3
        cases['tts_long_ms'] = tts_long
        cases['host_route_ms'] = host_route

    for fn in cases.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    host_join_ms = []
    for _ in range(args.reps):
        for k, fn in cases.items():
            times[k].append(fn())
            if k == 'host_route_ms':
                host_join_ms.append(res['host_join_ms'])
    for k, v in times.items():
        row[k] = round(statistics.median(v), 4)
        row[k.replace('_ms', '_min_ms')] = round(min(v), 4)
        row[k.replace('_ms', '_max_ms')] = round(max(v), 4)
    if 'join_ms' in row:
        row['join_GBps'] = round(row['join_bytes'] / (row['join_ms'] * 1e-3) / 1e9, 1)
    if 'tts_long_ms' in row:
        row.update(sentences=len(lines), paragraph_chars=len(paragraph), tts_long_samples=int(res['long'].numel()),
                   host_route_samples=int(res['host'].size), host_join_ms=round(statistics.median(host_join_ms), 4),
                   tts_long_readback_bytes=8 * (4 * len(lines) + 1), tts_long_join_launches=4)
    line = json.dumps(row)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
