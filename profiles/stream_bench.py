"""Streaming synthesis against the one-shot vocoder call (profiles/r17/NOTES.md is written from its output).

  (a) one mel of T = 2048 frames: host time from StreamingVocoder.open to the first chunk on the host, against Generator.forward of the
      whole mel + the copy of its wave to the host;
  (b) 32 streams of T = 512 at chunk_frames 64 and 128: host time from the first open to the last chunk on the host, against the
      one-shot ragged batch of the same mels (HifiGanEngine.forward + the copy of the waves), and both without the copies (the audio
      stays in HBM, one synchronise at the end), next to the arithmetic overhead (chunk + 2 halo) / chunk.

Host clock around work that ends in a device-to-host copy (a synchronise); every shape is warmed up first; medians over --reps runs,
the two sides of a comparison alternating inside one process.  Synthetic V1 weights, random mels from a seed.

  (c) the delivery formats (profiles/r18/NOTES.md): 32 open streams of T = 512 at chunk_frames 64, first_chunk_frames 32, leaving at
      --sample-rate as --encoding: the time per step (the whole run without copies / its steps) and the time from the first open to
      the first step's 32 chunks on the host.  Without the two flags the constructor gets no new argument, so the same file measures
      the commit before them.

    python profiles/stream_bench.py [--reps 15] [--warmup 3] [--precision f32] [--out FILE.jsonl]
                                    [--sample-rate 8000] [--encoding mulaw] [--only-c]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tts-arabic-pytorch_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--precision', default='f32')
    ap.add_argument('--out', default=None)
    ap.add_argument('--sample-rate', type=int, default=None)
    ap.add_argument('--encoding', default=None, choices=['float32', 'pcm16', 'mulaw', 'alaw'])
    ap.add_argument('--only-c', action='store_true', help='case (c) alone')
    args = ap.parse_args()
    delivery = {k: v for k, v in (('sample_rate', args.sample_rate), ('encoding', args.encoding)) if v is not None}

    import numpy as np
    import torch
    from ttsamd import synth
    from ttsamd.config import HIFIGAN_CONFIG
    from ttsamd.engine import set_precision
    from ttsamd.stream import StreamingVocoder
    from vocoder.hifigan.models import Generator

    assert torch.cuda.is_available(), 'stream_bench needs an MI355X: a CPU run says nothing about time'
    dev = torch.device('cuda:0')
    set_precision(args.precision)
    gen = Generator(dict(HIFIGAN_CONFIG), state_dict={k: torch.from_numpy(v) for k, v in synth.hifigan_state_dict().items()}).to(dev)
    eng = gen.engine()
    rng = np.random.default_rng(0)
    rows = []

    def emit(**kw):
        kw['precision'] = args.precision
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                for r in rows:
                    f.write(json.dumps(r) + '\n')

    def ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    def med(xs):
        return round(statistics.median(xs), 3), round(min(xs), 3), round(max(xs), 3)

    # ---- (c) 32 open streams at a delivery format: time per step, time to the first chunks ------------------------------------------------
    B, T = 32, 512
    mels_c = torch.from_numpy((np.random.default_rng(1).standard_normal((B, 80, T)) * 1.5 - 4.0).astype(np.float32)).to(dev)
    sv = StreamingVocoder(gen, max_streams=B, max_frames=T, chunk_frames=64, first_chunk_frames=32, **delivery)
    steps, first_c, run_c = [0], [], []

    def first_chunks():
        for b in range(B):
            sv.open(mels_c[b])
        [c.cpu() for _, c, _ in sv.step()]

    def rest_on_device():
        steps[0] = 1
        while sv.open_streams:
            steps[0] += 1
            sv.step()
        torch.cuda.synchronize()

    for i in range(args.warmup + args.reps):
        a, b = ms(first_chunks), ms(rest_on_device)
        if i >= args.warmup:
            first_c.append(a)
            run_c.append(b / (steps[0] - 1))
    emit(case='c', streams=B, frames=T, chunk_frames=64, first_chunk_frames=32, steps=steps[0], halo=sv.halo,
         sample_rate=getattr(sv, 'sample_rate', 22050), encoding=getattr(sv, 'encoding', 'float32'), first_chunks_ms=med(first_c),
         step_ms=med(run_c))
    if args.only_c:
        return save()

    # ---- (a) time to first audio of one long line ------------------------------------------------------------------------------------
    T = 2048
    mel = torch.from_numpy((rng.standard_normal((80, T)) * 1.5 - 4.0).astype(np.float32)).to(dev)
    sv = StreamingVocoder(gen, max_streams=1, max_frames=T)                # the shipped defaults: first 32, then 64
    first, total, oneshot = [], [], []

    def streamed():
        t0 = time.perf_counter()
        sv.open(mel)
        sv.step()[0][1].cpu()
        first.append(1e3 * (time.perf_counter() - t0))
        while sv.open_streams:
            for _, chunk, _ in sv.step():
                chunk.cpu()

    for i in range(args.warmup + args.reps):
        a, b = ms(streamed), ms(lambda: gen(mel).cpu())
        if i >= args.warmup:
            total.append(a)
            oneshot.append(b)
    first = first[args.warmup:]
    emit(case='a', frames=T, chunk_frames=sv.chunk_frames, first_chunk_frames=sv.first_chunk_frames, halo=sv.halo,
         first_chunk_ms=med(first), streamed_total_ms=med(total), oneshot_ms=med(oneshot), audio_s=round(256 * T / 22050, 2))

    # ---- (b) 32 streams against the one-shot ragged batch ----------------------------------------------------------------------------
    B, T = 32, 512
    mels = torch.from_numpy((rng.standard_normal((B, 80, T)) * 1.5 - 4.0).astype(np.float32)).to(dev)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    for chunk in (64, 128):
        sv = StreamingVocoder(gen, max_streams=B, max_frames=T, chunk_frames=chunk)
        steps = [0]

        def streamed_b():
            steps[0] = 0
            for b in range(B):
                sv.open(mels[b])
            while sv.open_streams:
                steps[0] += 1
                for _, c, _ in sv.step():
                    c.cpu()

        def streamed_b_device():                                          # the same without the copies: the chunks stay in HBM
            for b in range(B):
                sv.open(mels[b])
            while sv.open_streams:
                sv.step()
            torch.cuda.synchronize()

        def oneshot_b():
            w = eng.forward(mels, lens)
            [w[b].cpu() for b in range(B)]

        def oneshot_b_device():
            eng.forward(mels, lens)
            torch.cuda.synchronize()

        t = {k: [] for k in ('streamed', 'oneshot', 'streamed_device', 'oneshot_device')}
        for i in range(args.warmup + args.reps):
            run = dict(streamed=ms(streamed_b), oneshot=ms(oneshot_b), streamed_device=ms(streamed_b_device), oneshot_device=ms(oneshot_b_device))
            if i >= args.warmup:
                for k, v in run.items():
                    t[k].append(v)
        halo = sv.halo[0]
        m = {k: statistics.median(v) for k, v in t.items()}
        emit(case='b', streams=B, frames=T, chunk_frames=chunk, first_chunk_frames=sv.first_chunk_frames, steps=steps[0],
             streamed_ms=med(t['streamed']), oneshot_ms=med(t['oneshot']), streamed_device_ms=med(t['streamed_device']),
             oneshot_device_ms=med(t['oneshot_device']), ratio=round(m['streamed'] / m['oneshot'], 3),
             ratio_device=round(m['streamed_device'] / m['oneshot_device'], 3), arithmetic_ratio=round((chunk + 2 * halo) / chunk, 3))
    save()


if __name__ == '__main__':
    main()
