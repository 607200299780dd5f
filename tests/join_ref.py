"""Shared by tests/test_join_cpu.py and tests/test_gpu_join.py (not a test module): the numpy restatement of csrc/join.hip
(include/ttsamd.h: ttsamd_wave_join) as plain loops in fp32, pinned on the CPU by tests/test_join_cpu.py."""
import numpy as np

MAX_GAP = 1 << 40


def fade_table(n):
    """rising raised cosine, 0.5 - 0.5 cos(pi (i + 0.5) / n) in float64, rounded once to fp32"""
    i = np.arange(int(n), dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (i + 0.5) / max(int(n), 1))).astype(np.float32)


def ranges(nsamples, wave_stride, bounds, keep):
    """step 1: [(s, e)] per row"""
    out = []
    for b, n in enumerate(nsamples):
        n = min(max(int(n), 0), wave_stride)
        s, e = 0, n
        if bounds is not None:
            s = min(max(int(bounds[b][0]), 0), n)
            e = min(max(int(bounds[b][1]), s), n)
        if e > s:
            s, e = max(0, s - keep), min(n, e + keep)
        out.append((s, e))
    return out


def layout(nsamples, wave_stride, bounds, gap, n_fade, keep, lead):
    """steps 1 - 3: (segs [B][4] = (out_start, out_end, src_start, src_end), total)"""
    rng = ranges(nsamples, wave_stride, bounds, keep)
    m = [e - s for s, e in rng]
    B = len(m)
    segs, p = [], int(lead)
    for b in range(B):
        g = int(gap[b])
        if g >= 0:
            g = min(g, MAX_GAP)
        elif b == B - 1:
            g = 0
        else:
            g = -min(-g, n_fade, m[b] // 2, m[b + 1] // 2)
        segs.append((p, p + m[b], rng[b][0], rng[b][1]))
        p += m[b] + g
    return np.array(segs, dtype=np.int64).reshape(B, 4), p


def join(wave, nsamples, bounds, gap, fade, keep, lead, out_stride, return_count=False):
    """wave [B][wave_stride] fp32 -> (out [out_stride] fp32, segs int64 [B][4], total); with return_count also how many rows covered
    each output sample"""
    wave = np.asarray(wave, dtype=np.float32)
    fade = np.zeros(0, np.float32) if fade is None else np.asarray(fade, dtype=np.float32)
    F = int(fade.size)
    segs, total = layout(nsamples, wave.shape[1], bounds, gap, F, int(keep), int(lead))
    out = np.zeros(out_stride, dtype=np.float32)
    count = np.zeros(out_stride, dtype=np.int32)
    for b in range(wave.shape[0]):
        p, _, s, e = (int(v) for v in segs[b])
        m = e - s
        for i in range(m):
            j = p + i
            if j >= out_stride:
                break
            fin = fade[i] if i < F else np.float32(1.0)
            fout = fade[m - 1 - i] if m - 1 - i < F else np.float32(1.0)
            y = np.float32(np.float32(wave[b, s + i] * fin) * fout)
            out[j] = y if count[j] == 0 else np.float32(out[j] + y)
            count[j] += 1
    return (out, segs, total, count) if return_count else (out, segs, total)
