"""Writes tests/golden/g711.npz: G.711 as the Python standard library's audioop computes it (width 2), the arbiter of ttsamd/g711.py and
of the device encoders of csrc/stream.hip.

  lin2ulaw, lin2alaw  uint8 [65536]: the byte of every int16 value, index = value + 32768
  ulaw2lin, alaw2lin  int16 [256]:   the value of every byte

audioop left the standard library with Python 3.13; run this on an interpreter that still has it.  The tests read only the file."""
import os
import sys

import numpy as np

try:
    import audioop
except ImportError:
    sys.exit('gen_golden_g711: this Python has no audioop module (removed in 3.13): run the tool on Python <= 3.12')

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'g711.npz')


def main():
    pcm = np.arange(-32768, 32768, dtype=np.int32).astype('<i2')
    codes = np.arange(256, dtype=np.uint8)
    np.savez_compressed(
        OUT,
        lin2ulaw=np.frombuffer(audioop.lin2ulaw(pcm.tobytes(), 2), dtype=np.uint8),
        lin2alaw=np.frombuffer(audioop.lin2alaw(pcm.tobytes(), 2), dtype=np.uint8),
        ulaw2lin=np.frombuffer(audioop.ulaw2lin(codes.tobytes(), 2), dtype='<i2'),
        alaw2lin=np.frombuffer(audioop.alaw2lin(codes.tobytes(), 2), dtype='<i2'))
    print(f'{os.path.normpath(OUT)}: {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    main()
