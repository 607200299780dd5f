"""Vocos in the chunked vocoder (profiles/r24/NOTES.md is written from its output).

  (a) 32 open '22k' streams of T = 512 frames at the default chunking (first 32, then 64): the time of a warm step (the whole run
      without copies over its steps, one synchronise at the end) and per second of audio the step delivers; the same at chunk_frames
      128 and 256; the one-shot ragged batch of the same mels (VocosEngine.forward) beside it;
  (b) one utterance of 400 frames: host time from StreamingVocoder.open to the first chunk on the host, against one-shot
      MelVocos.forward of the same mel + the copy of its wave;
  (c) the window batch of a steady step (32 windows of 64 + 2 * 29 = 122 frames, the core in the middle) through
      ttsamd_vocos_forward_windows against the same batch through ttsamd_vocos_forward_rows, which computes the head on every window
      frame: device events around `--inner` calls of each, the two alternating inside the process;
  (d) the share of a step's frames that are halo, from the plans.

Every shape is warmed up first; medians (min, max) over --reps runs.  Synthetic weights, random mels from a seed, fp32.

    python profiles/vocos_stream_bench.py [--reps 15] [--warmup 3] [--inner 20] [--out FILE.jsonl]"""
import argparse
import ctypes as C
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
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from ttsamd import synth
    from ttsamd.config import VOCOS_22K_CONFIG
    from ttsamd.stream import StreamingVocoder, plan_chunks, vocos_halo_frames
    from vocoder.vocos import MelVocos

    assert torch.cuda.is_available(), 'vocos_stream_bench needs an MI355X: a CPU run says nothing about time'
    dev = torch.device('cuda:0')
    voc = MelVocos('22k')
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.vocos_state_dict(VOCOS_22K_CONFIG).items()})
    voc = voc.to(dev)
    eng = voc.engine()
    lib = eng.lib
    rng = np.random.default_rng(0)
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    def ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    def med(xs):
        return round(statistics.median(xs), 3), round(min(xs), 3), round(max(xs), 3)

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def cur():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    hl, hr = vocos_halo_frames(VOCOS_22K_CONFIG)

    # ---- (a) 32 open streams: a warm step -------------------------------------------------------------------------------------------------
    B, T = 32, 512
    mels = torch.from_numpy((rng.standard_normal((B, 80, T)) * 1.5 - 4.0).astype(np.float32)).to(dev)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    oneshot = []
    for i in range(args.warmup + args.reps):
        t = ms(lambda: (eng.forward(mels, lens), torch.cuda.synchronize()))
        if i >= args.warmup:
            oneshot.append(t)
    for chunk in (64, 128, 256):
        sv = StreamingVocoder(voc, max_streams=B, max_frames=T, chunk_frames=chunk, first_chunk_frames=32)
        steps, run = [0], []

        def on_device():
            steps[0] = 0
            for b in range(B):
                sv.open(mels[b])
            while sv.open_streams:
                steps[0] += 1
                sv.step()
            torch.cuda.synchronize()

        for i in range(args.warmup + args.reps):
            t = ms(on_device)
            if i >= args.warmup:
                run.append(t)
        plan = plan_chunks(T, 32, chunk, hl, hr)
        win, core = sum(c[3] for c in plan), sum(c[1] for c in plan)
        m = statistics.median(run)
        emit(case='a', streams=B, frames=T, chunk_frames=chunk, first_chunk_frames=32, steps=steps[0], halo=sv.halo, run_ms=med(run),
             step_ms=round(m / steps[0], 3), ms_per_audio_s=round(m / (B * 256 * T / 22050), 4), oneshot_ms=med(oneshot),
             ratio=round(m / statistics.median(oneshot), 3), window_frames=win, core_frames=core, halo_share=round(1 - core / win, 3),
             arithmetic_ratio=round(win / core, 3))

    # ---- (b) time to the first chunk of one utterance -------------------------------------------------------------------------------------
    T1 = 400
    mel = torch.from_numpy((rng.standard_normal((80, T1)) * 1.5 - 4.0).astype(np.float32)).to(dev)
    sv = StreamingVocoder(voc, max_streams=1, max_frames=T1)                # the defaults: first 32, then 64
    first, total, one = [], [], []

    def streamed():
        t0 = time.perf_counter()
        sv.open(mel)
        sv.step()[0][1].cpu()
        first.append(1e3 * (time.perf_counter() - t0))
        while sv.open_streams:
            for _, chunk, _ in sv.step():
                chunk.cpu()

    for i in range(args.warmup + args.reps):
        a, b = ms(streamed), ms(lambda: voc(mel[None]).cpu())
        if i >= args.warmup:
            total.append(a)
            one.append(b)
    emit(case='b', frames=T1, chunk_frames=sv.chunk_frames, first_chunk_frames=sv.first_chunk_frames, first_chunk_ms=med(first[args.warmup:]),
         streamed_total_ms=med(total), oneshot_ms=med(one), audio_s=round(256 * T1 / 22050, 2))

    # ---- (c) the window batch: the windows entry against the rows entry -------------------------------------------------------------------
    W, core = 32, 64
    w_max = (core + hl + hr + 3) & ~3
    batch = torch.from_numpy((rng.standard_normal((W, 80, w_max)) * 1.5 - 4.0).astype(np.float32)).to(dev)
    wl = torch.full((W,), core + hl + hr, dtype=torch.int64, device=dev)
    dn = torch.zeros(W, dtype=torch.float32, device=dev)
    bias = eng.bias_vec().reshape(-1)
    wave = torch.zeros(W, 256 * w_max, device=dev)
    nb = lib.ttsamd_vocos_workspace_bytes(eng.handle, W, w_max)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    i32 = C.c_int32 * W
    ns, nl = i32(*[hl] * W), i32(*[core] * W)

    def windows():
        rc = lib.ttsamd_vocos_forward_windows(eng.handle, ptr(batch), ptr(wl), W, w_max, ns, nl, ptr(dn), ptr(bias), ptr(wave), ptr(ws), nb, cur())
        assert rc == 0, lib.ttsamd_last_error()

    def whole():
        rc = lib.ttsamd_vocos_forward_rows(eng.handle, ptr(batch), ptr(wl), W, w_max, ptr(dn), ptr(bias), ptr(wave), ptr(ws), nb, cur())
        assert rc == 0, lib.ttsamd_last_error()

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.inner

    tw, tr = [], []
    for i in range(args.warmup + args.reps):
        x, y = events(windows), events(whole)
        if i >= args.warmup:
            tw.append(x)
            tr.append(y)
    emit(case='c', windows=W, window_frames=core + hl + hr, core_frames=core, forward_windows_ms=med(tw), forward_rows_ms=med(tr),
         ratio=round(statistics.median(tw) / statistics.median(tr), 4))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
