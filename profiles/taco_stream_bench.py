"""Tacotron2 as a stream next to the one-shot calls (profiles/r36/NOTES.md is written from its output).

Workload: config 4's shape -- B = 8 lines of about 64 tokens, 448 decoder steps (a synthetic checkpoint whose gate never fires, so
decoder_max_step decides) -- and B = 1.  One process, every case warmed up first, the cases alternating; host clock around calls that
end in a device-to-host copy.
  * wrapper: Tacotron2Wave.tts_stream -- time from the call to the first chunk on the host, and to the last -- against tts (tts_batch /
    tts_single) of the same lines in the same run;
  * decoder: a session driven in advances of --chunk steps against the same session driven in one advance of 448, both through
    Tacotron2Engine.stream: the difference per extra advance is what a segment costs beyond its steps (region copy, sentinel fill,
    cooperative launch that loads the resident weights again, the report's copy and the host's wait).

    timeout 600 python profiles/taco_stream_bench.py [--reps 7] [--warmup 2] [--steps 448] [--chunk 64] [--out FILE.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tts-arabic-pytorch_amd'))

PHRASE = 'اَلسَّلامُ عَلَيكُم يَا صَدِيقِي'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--steps', type=int, default=448)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import text
    from models.tacotron2 import Tacotron2Wave
    from ttsamd.config import HIFIGAN_CONFIG, TACOTRON2_CONFIG
    from ttsamd.synth import hifigan_state_dict, tacotron2_state_dict

    assert torch.cuda.is_available(), 'taco_stream_bench needs an MI355X: a CPU run says nothing about time'
    dev = torch.device('cuda:0')
    with tempfile.TemporaryDirectory() as d:
        sd = tacotron2_state_dict(dict(TACOTRON2_CONFIG, num_speakers=40), seed=0, gate_bias=-20.0)
        torch.save({'model': {k: torch.from_numpy(np.asarray(v).copy()) for k, v in sd.items()}, 'symbols': list(text.symbols)},
                   os.path.join(d, 'taco.pth'))
        torch.save({'generator': {k: torch.from_numpy(v.copy()) for k, v in hifigan_state_dict().items()}}, os.path.join(d, 'hg.pth'))
        with open(os.path.join(d, 'config.json'), 'w') as f:
            json.dump(HIFIGAN_CONFIG, f)
        model = Tacotron2Wave(os.path.join(d, 'taco.pth'), os.path.join(d, 'hg.pth'), os.path.join(d, 'config.json'),
                              n_symbol=len(text.symbols)).to(dev)
    model.model.decoder_max_step = args.steps
    model.model.dropout_seed = 3
    line = PHRASE
    while len(text.arabic_to_tokens(line + ' ' + PHRASE)) <= 64:
        line = line + ' ' + PHRASE
    n_tokens = len(text.arabic_to_tokens(line))
    lines8 = [line] * 8

    def sync_clock():
        torch.cuda.synchronize()
        return time.perf_counter()

    def stream_case(inp, batch_size):
        t0 = sync_clock()
        first, n_chunks = None, 0
        for item in model.tts_stream(inp, batch_size=batch_size, postprocess_mel=False, chunk_frames=args.chunk, first_chunk_frames=32,
                                     max_frames=max(args.steps, 64)):
            if first is None:
                first = time.perf_counter() - t0
            n_chunks += 1
        return {'first_ms': 1e3 * first, 'total_ms': 1e3 * (sync_clock() - t0), 'chunks': n_chunks}

    def one_shot_case(inp, batch_size):
        t0 = sync_clock()
        model.tts(inp, batch_size=batch_size, postprocess_mel=False)
        return {'total_ms': 1e3 * (sync_clock() - t0)}

    eng = model.model.engine()
    tok = torch.randint(1, 40, (8, 64), generator=torch.Generator().manual_seed(0))

    def decoder_case(B, chunk):
        t0 = sync_clock()
        sess = eng.stream(tok[:B], torch.zeros(B, dtype=torch.long), None, max_step=args.steps, dropout_seed=3, max_chunk_steps=chunk)
        while not sess.ended:
            sess.advance(chunk)
        ms = 1e3 * (sync_clock() - t0)
        n = sess.n_advances
        sess.close()
        return {'total_ms': ms, 'advances': n}

    whole = -(-args.steps // 8) * 8
    cases = {
        'b8_stream': lambda: stream_case(lines8, 8), 'b8_one_shot': lambda: one_shot_case(lines8, 8),
        'b1_stream': lambda: stream_case(line, 8), 'b1_one_shot': lambda: one_shot_case(line, 8),
        'b8_decoder_chunked': lambda: decoder_case(8, args.chunk), 'b8_decoder_whole': lambda: decoder_case(8, whole),
        'b1_decoder_chunked': lambda: decoder_case(1, args.chunk), 'b1_decoder_whole': lambda: decoder_case(1, whole),
    }
    for fn in cases.values():
        for _ in range(args.warmup):
            fn()
    runs = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, fn in cases.items():
            runs[k].append(fn())
    row = dict(bench='taco_stream', steps=args.steps, chunk=args.chunk, first_chunk_frames=32, tokens_per_line=n_tokens, reps=args.reps)
    for k, v in runs.items():
        for field in v[0]:
            vals = [r[field] for r in v]
            row[f'{k}_{field}'] = round(statistics.median(vals), 4) if field.endswith('_ms') else vals[0]
            if field.endswith('_ms'):
                row[f'{k}_{field[:-3]}_min_ms'], row[f'{k}_{field[:-3]}_max_ms'] = round(min(vals), 4), round(max(vals), 4)
    for b in ('b8', 'b1'):
        extra = row[f'{b}_decoder_chunked_advances'] - row[f'{b}_decoder_whole_advances']
        row[f'{b}_segment_overhead_us'] = round(1e3 * (row[f'{b}_decoder_chunked_total_ms'] - row[f'{b}_decoder_whole_total_ms']) / max(extra, 1), 2)
        row[f'{b}_first_chunk_before_one_shot'] = row[f'{b}_stream_first_ms'] < row[f'{b}_one_shot_total_ms']
    out = json.dumps(row)
    print(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
