"""Polyphase sinc-resampling table from its published formula, own code: computed in float64 and rounded once to float32.

With g = gcd(orig_freq, new_freq), o = orig_freq // g input samples and n = new_freq // g output samples per frame:
  base  = min(o, n) * rolloff                       (the low-pass cutoff, in units of the input rate / o)
  width = ceil(lowpass_filter_width * o / base)     (input samples the filter reaches to either side)
  J     = 2 * width + o                             (taps per phase)
  t     = clamp(((j - width) / o - p / n) * base, -lowpass_filter_width, +lowpass_filter_width)
  taps[p][j] = sinc(t) * cos(t * pi / lowpass_filter_width / 2) ** 2 * base / o          (Hann-windowed sinc)
Output sample f * n + p of a row is sum_j taps[p][j] * x[f * o + j - width] with zeros outside the row; a row of L samples gives
ceil(n * L / o) outputs.  This is the arithmetic of torchaudio's 'sinc_interp_hann' resampler; torchaudio is not a dependency of this
package, and the values are pinned to the formula, not to a release's own rounding."""
import functools
import math

import numpy as np


def rates(orig_freq, new_freq):
    """-> (o, n): the two rates divided by their gcd.  Non-integer or non-positive rates raise ValueError."""
    if int(orig_freq) != orig_freq or int(new_freq) != new_freq:
        raise ValueError(f'resample: integer sample rates are built (got {orig_freq}, {new_freq})')
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError(f'resample: sample rates must be positive (got {orig_freq}, {new_freq})')
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g


@functools.lru_cache(maxsize=16)
def _taps(o, n, lowpass_filter_width, rolloff):
    base = min(o, n) * rolloff
    width = int(math.ceil(lowpass_filter_width * o / base))
    j = np.arange(-width, width + o, dtype=np.float64)[None, :] / o
    p = np.arange(n, dtype=np.float64)[:, None] / n
    t = np.clip((j - p) * base, -lowpass_filter_width, lowpass_filter_width)
    win = np.cos(t * np.pi / lowpass_filter_width / 2.0) ** 2
    tpi = t * np.pi
    sinc = np.where(tpi == 0.0, 1.0, np.sin(tpi) / np.where(tpi == 0.0, 1.0, tpi))
    taps = (sinc * win * (base / o)).astype(np.float32)
    taps.setflags(write=False)
    return taps, width


def resample_taps(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """-> (taps float32 [n, J] (read-only, cached per argument tuple), width, o, n)."""
    if lowpass_filter_width <= 0:
        raise ValueError('resample: lowpass_filter_width must be positive')
    o, n = rates(orig_freq, new_freq)
    taps, width = _taps(o, n, int(lowpass_filter_width), float(rolloff))
    return taps, width, o, n


MAX_RATIO, MAX_TAPS = 4096, 65536       # the limits of ttsamd_resample_create (csrc/resample.hip) on o, n and on J = 2 * width + o


def geometry(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """-> (o, n, width) without building the table.  ValueError, with ttsamd_resample_create's words, for a pair of rates whose reduced
    ratio or filter the device resampler refuses (22 050 -> 8 003 Hz: no common factor, o = 22 050)."""
    if lowpass_filter_width <= 0:
        raise ValueError('resample: lowpass_filter_width must be positive')
    o, n = rates(orig_freq, new_freq)
    if o > MAX_RATIO or n > MAX_RATIO:
        raise ValueError(f'resample_create: o = {o} / n = {n} outside [1, {MAX_RATIO}] ({int(orig_freq)} -> {int(new_freq)} Hz)')
    width = int(math.ceil(int(lowpass_filter_width) * o / (min(o, n) * float(rolloff))))
    if 2 * width + o > MAX_TAPS:
        raise ValueError(f'resample_create: width {width}: J = 2 * width + o is at most {MAX_TAPS}')
    return o, n, width


def out_len(n_samples, o, n):
    """ceil(n * n_samples / o) in exact integers."""
    return (n * int(n_samples) + o - 1) // o if n_samples > 0 else 0
