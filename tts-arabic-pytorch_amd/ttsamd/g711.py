"""G.711 on the host, numpy: the two 8-bit telephone encodings of 16-bit PCM and their decoders, restated from the standard's tables as
integer arithmetic (include/ttsamd.h gives the same two encoders; csrc/stream.hip runs them on the device).  tests/golden/g711.npz pins
every value of all four functions."""
import numpy as np


def _log2(m):
    """floor(log2(m)) of positive int32 values below 2 ** 15"""
    e = np.zeros(m.shape, dtype=np.int32)
    for b in range(1, 15):
        e += (m >> b) > 0
    return e


def lin2ulaw(pcm):
    """int16 -> uint8 mu-law: the 14-bit magnitude plus the bias 33, clipped to 8191, as sign | exponent | 4 mantissa bits, complemented"""
    a = np.asarray(pcm).astype(np.int32) >> 2
    neg = a < 0
    m = np.minimum(np.where(neg, -a, a) + 33, 8191)
    e = _log2(m) - 5
    return (~(neg.astype(np.int32) << 7 | e << 4 | ((m >> (e + 1)) & 15)) & 0xff).astype(np.uint8)


def lin2alaw(pcm):
    """int16 -> uint8 A-law: the 13-bit value in one's complement magnitude as sign | segment | 4 mantissa bits, even bits inverted"""
    a = np.asarray(pcm).astype(np.int32) >> 3
    pos = a >= 0
    a = np.where(pos, a, ~a)
    seg = np.where(a < 32, 0, _log2(np.maximum(a, 1)) - 4)
    mant = np.where(seg < 2, (a >> 1) & 15, (a >> seg) & 15)
    return ((pos.astype(np.int32) << 7 | seg << 4 | mant) ^ 0x55).astype(np.uint8)


def ulaw2lin(data):
    """uint8 mu-law -> int16"""
    u = ~np.asarray(data).astype(np.int32) & 0xff
    t = (((u & 0x0f) << 3) + 0x84) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int16)


def alaw2lin(data):
    """uint8 A-law -> int16"""
    a = (np.asarray(data).astype(np.int32) ^ 0x55) & 0xff
    seg = (a & 0x70) >> 4
    t = (a & 0x0f) << 4
    t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
    return np.where(a & 0x80, t, -t).astype(np.int16)


ENCODERS = {'mulaw': lin2ulaw, 'alaw': lin2alaw}
DECODERS = {'mulaw': ulaw2lin, 'alaw': alaw2lin}
