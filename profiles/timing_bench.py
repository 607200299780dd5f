"""What the timestamps cost (csrc/timing.hip, ttsamd/timing.py; profiles/r42/NOTES.md is written from its output): every case against
the SAME call without the flag, in the same process, warmed up first and alternating.

  spans     ttsamd_token_spans alone at B = 32, L = 256 with 40 word ranges a row and a map: the median time of --iters back-to-back
            calls between two device events (one launch a call).
  tts       FastPitch2Wave.tts(32 lines, batch_size=32) with and without return_timestamps=True, host clock around the call (the
            synthetic full-size checkpoints, the 32 shortest committed text lines).
  tts_long  FastPitch2Wave.tts_long on the 32-sentence paragraph of profiles/join_bench.py, with and without the flag.
Device -> host copies are counted per call by wrapping torch.Tensor.cpu / .tolist / .item for the duration of one call of each case (the
only ways the synthesis path reads back); the count with the flag off is the path's own.  No ratio is required of any of it.

--tree DIR runs the flag-off cases alone on ANOTHER checkout's package (DIR/tts-arabic-pytorch_amd with its library built): the parent
commit on the same machine, for the times and copy counts the flag-off path is held against.

    python profiles/timing_bench.py [--reps 9] [--warmup 2] [--iters 50] [--tree DIR] [--out FILE.jsonl]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index('--tree') + 1]) if '--tree' in sys.argv else REPO      # (before the package is imported)
sys.path.insert(0, os.path.join(TREE, 'tts-arabic-pytorch_amd'))


class CopyCounter:
    """counts the device -> host reads of a block: .cpu(), .tolist() and .item() of a tensor that lives on the device"""

    def __enter__(self):
        import torch
        self.n, self.saved = 0, {k: getattr(torch.Tensor, k) for k in ('cpu', 'tolist', 'item')}
        for name, fn in self.saved.items():
            def wrapped(t, *a, _fn=fn, **kw):
                if t.device.type == 'cuda':
                    self.n += 1
                return _fn(t, *a, **kw)
            setattr(torch.Tensor, name, wrapped)
        return self

    def __exit__(self, *exc):
        import torch
        for name, fn in self.saved.items():
            setattr(torch.Tensor, name, fn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--tree', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    other = args.tree is not None

    import numpy as np
    import torch
    import text
    from models.fastpitch import FastPitch2Wave
    from ttsamd import lib as L
    from ttsamd import synth
    from ttsamd.config import HIFIGAN_CONFIG, NET_CONFIG

    assert torch.cuda.is_available(), 'timing_bench needs an MI355X: a CPU run says nothing about time'
    dev = torch.device('cuda:0')
    row = dict(bench='timing', reps=args.reps, iters=args.iters, tree='other' if other else 'this')

    B, Lt, G = 32, 256, 40
    rng = np.random.default_rng(0)
    reps = torch.from_numpy(rng.integers(0, 20, size=(B, Lt)).astype(np.int64)).to(dev)
    groups = torch.from_numpy(np.stack([np.stack([np.arange(G) * 6, np.arange(G) * 6 + 5], 1)] * B).astype(np.int32)).to(dev)
    maps = torch.tensor([(300, 1 << 40, 1000 * b, 160, 441) for b in range(B)], dtype=torch.int64).to(dev)
    tok = torch.empty(B, Lt, 2, dtype=torch.int64, device=dev)
    grp = torch.empty(B, G, 2, dtype=torch.int64, device=dev)
    h = L.load()
    p = lambda t: C.c_void_p(t.data_ptr())                                                       # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def spans():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            L.check(h.ttsamd_token_spans(p(reps), Lt, None, B, Lt, p(groups), None, G, 256, p(maps), p(tok), p(grp), stream), 'token_spans')
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.iters

    with open(os.path.join(REPO, 'tests', 'golden', 'infer_text_lines.json'), encoding='utf-8') as f:
        lines = sorted(json.load(f), key=len)[:32]
    with tempfile.TemporaryDirectory() as d:
        torch.save({'model': {k: torch.from_numpy(np.array(v)) for k, v in synth.fastpitch_state_dict().items()}, 'config': dict(NET_CONFIG),
                    'symbols': list(text.symbols)}, os.path.join(d, 'fp.pth'))
        torch.save({'generator': {k: torch.from_numpy(np.array(v)) for k, v in synth.hifigan_state_dict().items()}}, os.path.join(d, 'hg.pth'))
        with open(os.path.join(d, 'config.json'), 'w') as f:
            json.dump(HIFIGAN_CONFIG, f)
        model = FastPitch2Wave(os.path.join(d, 'fp.pth'), vocoder_sd=os.path.join(d, 'hg.pth'), vocoder_config=os.path.join(d, 'config.json')).to(dev)
    paragraph = '. '.join(lines)

    def clocked(fn):
        def run():
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3
        return run
    calls = {
        'tts_ms': lambda: model.tts(lines, batch_size=32),
        'tts_stamps_ms': lambda: model.tts(lines, batch_size=32, return_timestamps=True),
        'tts_long_ms': lambda: model.tts_long(paragraph, batch_size=32),
        'tts_long_stamps_ms': lambda: model.tts_long(paragraph, batch_size=32, return_timestamps=True),
    }
    if other:
        calls = {k: fn for k, fn in calls.items() if 'stamps' not in k}
    cases = dict({} if other else {'spans_ms': spans}, **{k: clocked(fn) for k, fn in calls.items()})
    for fn in cases.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for k, fn in calls.items():
        with CopyCounter() as cc:
            fn()
        row[k.replace('_ms', '_d2h_copies')] = cc.n
    times = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, fn in cases.items():
            times[k].append(fn())
    for k, v in times.items():
        row[k] = round(statistics.median(v), 4)
        row[k.replace('_ms', '_min_ms')] = round(min(v), 4)
        row[k.replace('_ms', '_max_ms')] = round(max(v), 4)
    row.update(lines=len(lines))
    if not other:
        row.update(spans_rows=B, spans_tokens=Lt, spans_groups=G, spans_launches=1, spans_bytes_out=16 * B * (Lt + G),
                   tts_added_ms=round(row['tts_stamps_ms'] - row['tts_ms'], 4), tts_long_added_ms=round(row['tts_long_stamps_ms'] - row['tts_long_ms'], 4))
    line = json.dumps(row)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
