"""Objective evaluation (csrc/objective.hip): milliseconds per ttsamd.engine.objective_score call -- two cepstra, the DTW of their
coefficients 1 .. 12, the evaluation along the path -- at B = 1 and B = 32 pairs of about 450 x 430 frames (80 bands, 13 coefficients,
ragged), its pieces alone, and ObjectiveEngine.score_waves on 32 pairs of 5 s (mel analysis and pYIN of both sides included).  Beside
them the float64 numpy restatement (tests/objective_ref.py, with the fp32 DTW of tests/oversmoothing_ref.py) on the same pairs: a
restatement, NOT a reference -- no package computes these numbers the same way; it is the only other thing that runs.
Per measurement: warm-up, then >= 15 calls timed with device events around work that ends in a synchronise, median; three rounds, the
per-round medians kept.  One JSON line per measurement, written to stdout.
    python tools/objective_bench.py [--calls 20] [--rounds 3] > profiles/r13/objective_bench.jsonl
    python tools/objective_bench.py --kernel-only      (the library's calls alone, for `rocprofv3 --kernel-trace --stats -- python ...`)"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tts-arabic-pytorch_amd'))
sys.path.insert(0, os.path.join(REPO, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--numpy-pairs', type=int, default=2, help='pairs the numpy restatement is timed on (its time is per pair)')
    a = ap.parse_args()
    import torch
    import melspec_ref as MR
    import objective_ref as R
    import oversmoothing_ref as OR
    from ttsamd import engine as E
    dev = torch.device('cuda:0')

    def timed(fn, calls):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def rounds(fn):
        return [timed(fn, max(a.calls, 15)) for _ in range(a.rounds)]

    med = lambda r: float(np.median(r))  # noqa: E731
    us = lambda r: round(med(r) * 1e3, 1)  # noqa: E731
    rng = np.random.default_rng(0)
    for B in (1, 32):
        tp, tr = 450, 430
        lp = np.full(B, tp) if B == 1 else np.concatenate([[tp], rng.integers(300, tp + 1, B - 1)])
        lr = np.full(B, tr) if B == 1 else np.concatenate([[tr], rng.integers(300, tr + 1, B - 1)])
        pred, ref = np.zeros((B, 80, tp), np.float32), np.zeros((B, 80, tr), np.float32)
        for b in range(B):
            pa, pb = OR.warped_pair(100 + b, 80, int(lp[b]), int(lr[b]))
            pred[b, :, :lp[b]], ref[b, :, :lr[b]] = pa, pb
        fp = np.where(rng.random((B, tp)) < 0.3, 0.0, rng.uniform(80, 400, (B, tp))).astype(np.float32)
        fr = np.where(rng.random((B, tr)) < 0.3, 0.0, rng.uniform(80, 400, (B, tr))).astype(np.float32)
        d = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
        pred_d, ref_d, fp_d, fr_d, lp_d, lr_d = d(pred), d(ref), d(fp), d(fr), d(lp), d(lr)
        score = lambda: E.objective_score(pred_d, lp_d, ref_d, lr_d, fp_d, fr_d)  # noqa: E731
        if a.kernel_only:
            for _ in range(5):
                score()
            torch.cuda.synchronize()
            continue
        out = score()
        cp, cr = E.mel_cepstrum(pred_d, lp_d, 13), E.mel_cepstrum(ref_d, lr_d, 13)
        path, plen = out['path'], out['path_len']
        r_score = rounds(score)
        r_frames = rounds(lambda: E.objective_score(pred_d, lp_d, ref_d, lr_d, fp_d, fr_d, align='frames'))
        r_cep = rounds(lambda: E.mel_cepstrum(pred_d, lp_d, 13))
        r_dtw = rounds(lambda: E.dtw(cp[:, 1:], cr[:, 1:], lp_d, lr_d))
        r_eval = rounds(lambda: E.dtw_aligned_eval(cp, cr, path, plen, pred_d, ref_d, fp_d, fr_d))
        # the numpy restatement of the same chain, per pair
        t_np, worst = [], 0.0
        for b in range(min(B, a.numpy_pairs)):
            t0 = time.perf_counter()
            ca = R.cepstrum(pred[b, :, :lp[b]], 13).astype(np.float32)
            cb = R.cepstrum(ref[b, :, :lr[b]], 13).astype(np.float32)
            _, wpath = OR.dtw_fp32(ca[1:].T, cb[1:].T, 0, -1)
            want = R.aligned_eval(ca, cb, wpath, pred[b], ref[b], fp[b], fr[b])
            t_np.append(time.perf_counter() - t0)
            got = np.array([float(out[k][b]) for k in E.OBJECTIVE_KEYS])
            worst = max(worst, float(np.nanmax(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))))
        print(json.dumps({
            'what': f'objective_score b{B}', 'batch': B, 'frames_pred': tp, 'frames_ref': tr, 'frames_min': int(min(lp.min(), lr.min())),
            'path_steps_mean': round(float(plen.float().mean()), 1),
            'score_dtw_us': us(r_score), 'score_dtw_us_per_round': [round(v * 1e3, 1) for v in r_score],
            'score_frames_us': us(r_frames), 'mel_cepstrum_us': us(r_cep), 'dtw_us': us(r_dtw), 'dtw_aligned_eval_us': us(r_eval),
            'numpy_restatement_ms_per_pair': round(float(np.median(t_np)) * 1e3, 1), 'numpy_pairs_timed': len(t_np),
            'max_rel_diff_to_restatement': worst}), flush=True)

    # wave against wave: 32 pairs of about 5 s
    B = 32
    n_p, n_r = rng.integers(4 * 22050, 5 * 22050 + 1, B), rng.integers(4 * 22050, 5 * 22050 + 1, B)
    n_p[0] = n_r[0] = 5 * 22050
    wp, wr = np.zeros((B, n_p.max()), np.float32), np.zeros((B, n_r.max()), np.float32)
    for b in range(B):
        wp[b, :n_p[b]], wr[b, :n_r[b]] = MR.voiced(int(n_p[b]), 200 + b), MR.voiced(int(n_r[b]), 300 + b)
    wp_d, wr_d, np_d, nr_d = (torch.from_numpy(x).to(dev) for x in (wp, wr, n_p, n_r))
    obj = E.ObjectiveEngine()
    waves = lambda: obj.score_waves(wp_d, np_d, wr_d, nr_d)  # noqa: E731
    if a.kernel_only:
        for _ in range(3):
            waves()
        torch.cuda.synchronize()
        return
    out = waves()
    r_waves = rounds(waves)
    r_feat = rounds(lambda: obj.features(wp_d, np_d))
    print(json.dumps({
        'what': 'score_waves b32 5s', 'batch': B, 'seconds_max': 5.0, 'frames_max': int(out['lens_pred'].max()),
        'score_waves_us': us(r_waves), 'score_waves_us_per_round': [round(v * 1e3, 1) for v in r_waves],
        'features_one_side_us': us(r_feat), 'n_vv_share_mean': round(float((out['n_vv'] / out['n']).mean()), 3),
        'mcd_mean_db': round(float(out['mcd'].mean()), 3)}), flush=True)


if __name__ == '__main__':
    main()
