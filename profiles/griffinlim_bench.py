"""Griffin-Lim on the device (csrc/griffinlim.hip) next to the same loop written with torch.stft / torch.istft on the same GPU
(profiles/r39/NOTES.md is written from its output).

Workload: B = 1 and B = 32 rows of 450 frames (`center` framing: 449 * 256 = 114 944 samples, 5.2 s at 22 050 Hz) of a speech-like
row's STFT magnitude, 32 iterations, momentum 0.99 and 0, from the hashed initial phase.  Reported per case: the median time of
GriffinLimEngine.forward (n_iter + 3 launches) over --reps measurements of --iters back-to-back calls between two device events on one
stream, every case warmed up first and the cases alternating inside one process; the time per iteration (the difference to the same
call at n_iter = 0, over n_iter); the algorithmic HBM bytes of one iteration -- what gl_iter_kernel reads and writes: per frame the
previous frame matrix (4 KiB unique; 16 KiB issued, each sample gathering up to four frames' entries, the overlap served by L2), the
new frame (4 KiB written), its column of `mag` (2052 B) and, with momentum, tprev read and written (2 x 4104 B) -- and the rate that
gives; and the torch loop (torchaudio.functional.griffinlim's statements on torch.stft / torch.istft with the same window, from the
same initial angles: the reference route, and the only baseline there is).  No ratio is required of either.

    python profiles/griffinlim_bench.py [--reps 9] [--warmup 2] [--iters 5] [--frames 450] [--n-iter 32] [--out FILE.jsonl]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tts-arabic-pytorch_amd'))


def speech_like(rows, n, fs=22050):
    import numpy as np
    rng = np.random.default_rng(0)
    t = np.arange(n) / fs
    out = np.empty((rows, n), dtype=np.float32)
    for b in range(rows):
        phase = 2 * np.pi * (100.0 + 5.0 * b) * t + 3.0 * np.sin(2 * np.pi * 5.0 * t)
        s = sum(np.sin(h * phase + 0.7 * h) / h for h in range(1, 9))
        env = np.maximum(np.sin(2 * np.pi * 2.3 * t + 0.2 * b), 0.0) ** 2
        out[b] = 0.3 * env * s + 3e-3 * rng.standard_normal(n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--frames', type=int, default=450)
    ap.add_argument('--n-iter', type=int, default=32)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import torch
    from ttsamd.engine import GriffinLimEngine

    assert torch.cuda.is_available(), 'griffinlim_bench needs an MI355X: a CPU run says nothing about time'
    dev = torch.device('cuda:0')
    eng = GriffinLimEngine(device=dev)
    T, n_iter = args.frames, args.n_iter
    n = 256 * (T - 1)
    win = torch.hann_window(1024, device=dev)

    def stft(x):
        return torch.stft(x, 1024, 256, 1024, win, center=True, pad_mode='reflect', normalized=False, onesided=True, return_complex=True)

    def torch_loop(mag, angles, momentum, iters):
        """torchaudio.functional.griffinlim's loop; mag, angles [B, 513, T]"""
        c = momentum / (1 + momentum)
        tprev = torch.zeros_like(angles)
        for _ in range(iters):
            inv = torch.istft(mag * angles, 1024, 256, 1024, win, center=True, length=n)
            rebuilt = stft(inv)
            angles = rebuilt - c * tprev if momentum else rebuilt
            angles = angles / (angles.abs() + 1e-16)
            tprev = rebuilt
        return torch.istft(mag * angles, 1024, 256, 1024, win, center=True, length=n)

    def timed(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters

    wave_all = torch.from_numpy(speech_like(32, n)).to(dev)
    cases, meta = {}, {}
    for B in (1, 32):
        mag = stft(wave_all[:B]).abs().contiguous()                     # [B, 513, T]
        for momentum in (0.99, 0.0):
            # the engine's own initial angles, so that both routes start from the same state
            _, ang = eng.forward(mag, None, n_iter=0, momentum=momentum, framing='center', init='hash', seed=1, return_phase=True)
            ang_cf = ang.transpose(1, 2).contiguous()                   # [B, 513, T] for the torch loop
            key = f'b{B}_m{momentum:g}'
            cases[f'{key}_hip_ms'] = lambda m=mag, mo=momentum: eng.forward(m, None, n_iter=n_iter, momentum=mo, framing='center', init='hash', seed=1)
            cases[f'{key}_hip0_ms'] = lambda m=mag, mo=momentum: eng.forward(m, None, n_iter=0, momentum=mo, framing='center', init='hash', seed=1)
            cases[f'{key}_torch_ms'] = lambda m=mag, a=ang_cf, mo=momentum: torch_loop(m, a, mo, n_iter)
            unique = 4096 + 4096 + 2052 + (2 * 4104 if momentum else 0)
            meta[key] = dict(B=B, momentum=momentum, bytes_unique_per_iter=B * T * unique, bytes_issued_per_iter=B * T * (unique + 3 * 4096))
            # one correctness line per case: both routes from the same angles, one iteration (fp32 on both sides)
            w_hip = eng.forward(mag, None, n_iter=1, momentum=momentum, framing='center', init='phase', phase=ang)
            w_ref = torch_loop(mag, ang_cf, momentum, 1)
            meta[key]['one_iter_max_abs_vs_torch'] = float((w_hip - w_ref).abs().max())
            meta[key]['peak'] = float(w_ref.abs().max())
    for fn in cases.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, fn in cases.items():
            times[k].append(timed(fn, args.iters))
    row = dict(bench='griffinlim', frames=T, samples_per_row=n, n_iter=n_iter, framing='center', reps=args.reps, iters=args.iters,
               kernel_launches=n_iter + 3)
    for k, v in times.items():
        row[k] = round(statistics.median(v), 4)
        row[k.replace('_ms', '_min_ms')] = round(min(v), 4)
        row[k.replace('_ms', '_max_ms')] = round(max(v), 4)
    for key, m in meta.items():
        per_iter = (row[f'{key}_hip_ms'] - row[f'{key}_hip0_ms']) / n_iter
        row[f'{key}_hip_per_iter_ms'] = round(per_iter, 5)
        row[f'{key}_torch_per_iter_ms'] = round(row[f'{key}_torch_ms'] / (n_iter + 0.5), 5)
        row[f'{key}_bytes_unique_per_iter'] = m['bytes_unique_per_iter']
        row[f'{key}_bytes_issued_per_iter'] = m['bytes_issued_per_iter']
        row[f'{key}_unique_GBps'] = round(m['bytes_unique_per_iter'] / (per_iter * 1e-3) / 1e9, 1)
        row[f'{key}_issued_GBps'] = round(m['bytes_issued_per_iter'] / (per_iter * 1e-3) / 1e9, 1)
        row[f'{key}_frame_pairs_per_us'] = round(m['B'] * T / 2 / (per_iter * 1e3), 3)
        row[f'{key}_torch_over_hip'] = round(row[f'{key}_torch_ms'] / row[f'{key}_hip_ms'], 2)
        row[f'{key}_one_iter_max_abs_vs_torch'] = m['one_iter_max_abs_vs_torch']
        row[f'{key}_peak'] = m['peak']
    line = json.dumps(row)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
