"""Command line twin of the reference's inference.py (same flags and defaults, :96-111): synthesise every
line of --list with FastPitch2Wave / Tacotron2Wave on the MI355X and write <out_dir>/wavs/static<i>.wav.
The html sample page of the reference (utils/make_html.py) is out of scope; a plain index.tsv is written."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from utils import read_lines_from_file  # noqa: E402
from utils.audio import resample, save_wav  # noqa: E402

WAV_ENCODINGS = {'pcm16': ('PCM_S', 16), 'float32': ('PCM_F', 32), 'mulaw': ('ULAW', 8), 'alaw': ('ALAW', 8)}


def normalize_option(text):
    """--normalize: 'peak', 'lufs' or a number (a target in LUFS)"""
    if text in ('peak', 'lufs'):
        return text
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r}: 'peak', 'lufs' or a target in LUFS such as -16")


def infer(args):
    if args.cpu or not torch.cuda.is_available():
        raise SystemExit('inference.py: this build runs on an MI355X only (no CPU path); drop --cpu')
    if args.model == 'fastpitch':
        from models.fastpitch import FastPitch2Wave as Model
    elif args.model == 'tacotron2':
        from models.tacotron2 import Tacotron2Wave as Model
    else:
        raise TypeError('model type not supported')
    model = Model(args.checkpoint, vocoder_sd=args.vocoder_sd, vocoder_config=args.vocoder_config).to('cuda').eval()
    os.makedirs(os.path.join(args.out_dir, 'wavs'), exist_ok=True)
    lines = [ln for ln in read_lines_from_file(args.list) if ln]
    idx = 0
    rate = args.sample_rate or 22_050
    enc, bits = WAV_ENCODINGS[args.encoding]
    with open(os.path.join(args.out_dir, 'index.tsv'), 'w', encoding='utf-8') as index:
        for k in range(0, len(lines), args.batch_size):
            batch = lines[k:k + args.batch_size]
            level = dict(normalize=args.normalize, **({'limiter': True} if args.limiter else {}), **({'true_peak': True} if args.true_peak else {}))
            stamps = {'return_timestamps': True} if args.timestamps else {}
            if args.long:                           # every line is a paragraph: split, synthesised and joined on the device (tts_long)
                wavs = [model.tts_long(line, denoise=args.denoise, speed=args.speed, **level, **stamps) for line in batch]
                wavs, timings = (zip(*wavs) if stamps else (wavs, [None] * len(batch)))
            else:
                wavs = model.tts(batch, batch_size=args.batch_size, denoise=args.denoise, speed=args.speed, **level, **stamps)
                wavs, timings = wavs if stamps else (wavs, [None] * len(batch))
            for line, wav, timing in zip(batch, wavs, timings):
                if rate != 22_050:                      # the finished wave through the device resampler, then the matching file format
                    wav = resample(wav.reshape(1, -1).to('cuda'), 22_050, rate)[0]
                if timing is not None:                  # static<i>.json | srt | vtt next to the wave, the marks at the rate of the file
                    from ttsamd.timing import delivered_timing
                    from utils import timing as T
                    write = {'json': T.to_json, 'srt': T.to_srt, 'vtt': T.to_vtt}[args.timestamps]
                    with open(os.path.join(args.out_dir, 'wavs', f'static{idx}.{args.timestamps}'), 'w', encoding='utf-8') as f:
                        f.write(write(delivered_timing(timing, rate)))
                save_wav(os.path.join(args.out_dir, 'wavs', f'static{idx}.wav'), wav, rate, encoding=enc, bits_per_sample=bits)
                index.write(f'wavs/static{idx}.wav\t{wav.numel()}\t{line}\n')
                idx += 1
    print(f'Saved files to: {args.out_dir}')


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--list', type=str, default='./data/infer_text.txt')
    p.add_argument('--model', type=str, default='fastpitch')
    p.add_argument('--checkpoint', type=str, default='pretrained/fastpitch_ar_adv.pth')
    p.add_argument('--vocoder_sd', type=str, default=None)
    p.add_argument('--vocoder_config', type=str, default=None)
    p.add_argument('--out_dir', type=str, default='samples/results')
    p.add_argument('--speed', type=float, default=1.0)
    p.add_argument('--denoise', type=float, default=0)
    p.add_argument('--batch_size', type=int, default=2)
    p.add_argument('--cpu', action='store_true')
    # not in the reference: the rate and the encoding of the files (8000 + mulaw / alaw: G.711 telephony files, WAVE format 7 / 6)
    p.add_argument('--sample_rate', type=int, default=None)
    p.add_argument('--encoding', type=str, default='pcm16', choices=sorted(WAV_ENCODINGS))
    # ... and the level of every wave, set on the device: peak (x / max|x| * 0.99), lufs (-23 LUFS, ITU-R BS.1770-4) or a target in LUFS
    p.add_argument('--normalize', type=normalize_option, default=None, metavar='peak|lufs|<LUFS>')
    # ... with the look-ahead limiter in place of the cap on the gain, so that a LUFS target is reached (needs --normalize lufs or a target)
    p.add_argument('--limiter', action='store_true')
    # ... and with 0.99 as a true-peak ceiling (4x oversampled) instead of a sample peak, so that the resampled files do not clip
    p.add_argument('--true_peak', action='store_true')
    # ... every line of --list as a paragraph: cut into sentences, synthesised in batches and joined on the device with pauses (tts_long)
    p.add_argument('--long', action='store_true')
    # ... where every word lies in the wave: static<i>.json (words and tokens, in samples and seconds), .srt or .vtt cues next to static<i>.wav
    p.add_argument('--timestamps', type=str, default=None, choices=['json', 'srt', 'vtt'])
    args = p.parse_args(argv)
    if args.limiter and args.normalize in (None, 'peak'):
        p.error("--limiter needs --normalize lufs or a target in LUFS")
    if args.true_peak and args.normalize is None:
        p.error("--true_peak needs --normalize")
    infer(args)


if __name__ == '__main__':
    main()
