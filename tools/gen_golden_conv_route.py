"""Writes tests/golden/conv_route.json: what the fp32 conv launchers of ONE build route every case of a grid to, per option set.

    python tools/gen_golden_conv_route.py <libttsamd.so of a dry-run build>

A dry-run build is the library with its own launch lines (hipLaunchKernelGGL + hipGetLastError) and lds_opt_in turned into no-ops that
succeed: ttsamd_conv1d_splitk then runs to its end on dummy aligned pointers without a GPU, and ttsamd_conv_last_launch reports what
the launchers decided.  The golden in the repository was made this way from the commit before csrc/conv_route.hip existed, so that
tests/test_conv_route_cpu.py holds the routing function to the launchers it replaced; regenerate it only from a build whose routing is
the intended one, never from the query under test."""
import base64
import ctypes as C
import json
import os
import sys
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
from test_conv_route_cpu import cases  # noqa: E402  (the one enumeration of the grid)

GRID = {
    'k': [1, 2, 3, 5, 7, 11],
    'dilation_k3_7_11': [3, 5],
    'channels': [[80, 512], [512, 512], [256, 256], [128, 128], [64, 64], [32, 32], [128, 64], [384, 1536], [1536, 384], [384, 192],
                 [64, 384], [24, 128], [16, 128]],
    # 23040 = 360 mel frames x 64: batch 1 of HiFi-GAN's C = 128, k = 3, dilation 3 conv lands on conv1d_wino2_f32 there
    'lin': [64, 96, 255, 256, 257, 496, 504, 1031, 1032, 2052, 4100, 23040, 28672],
    'batch': [1, 2, 8, 32],
    'in_slope': [0.1, 1.5],
    'splitk_floats': [0, 4 << 20],
}
OPTION_SETS = [{}, {'WINO': 0}] + [{'WINO4': v} for v in (0, 15, 31, 111, 127)] + [{'WINO4': 0, 'WINO2': v} for v in (0, 6, 15)] + \
              [{'DEEP_SPLITK': 0}]


def main(path):
    h = C.CDLL(path)
    i32, f32, i64, ptr = C.c_int32, C.c_float, C.c_int64, C.c_void_p
    h.ttsamd_conv1d_splitk.argtypes = [ptr] * 5 + [i32] * 6 + [f32, i32, i32, f32, ptr, ptr, ptr, i64, ptr]
    h.ttsamd_set_option.argtypes = [C.c_char_p, C.c_char_p]
    any_buf = 256                                    # stands for every buffer: aligned, never followed by a dry-run build
    route, ksplit = i32(), i32()
    all_cases = list(cases(GRID))
    sets = []
    for options in OPTION_SETS:
        for name, value in options.items():
            assert h.ttsamd_set_option(name.encode(), str(value).encode()) == 0
        out = bytearray(2 * len(all_cases))
        for i, (batch, cin, cout, k, dil, lin, slope, relu_out, has_res, mode, skf) in enumerate(all_cases):
            rc = h.ttsamd_conv1d_splitk(any_buf, any_buf, None, any_buf if has_res else None, None, batch, cin, cout, k, dil, lin, slope,
                                        relu_out, mode, 3.0, any_buf, any_buf, any_buf if skf else None, skf, None)
            if rc == 0:
                assert h.ttsamd_conv_last_launch(C.byref(route), C.byref(ksplit)) == 0
                out[2 * i], out[2 * i + 1] = route.value, ksplit.value
            else:
                out[2 * i], out[2 * i + 1] = 255, 0   # rejected (C-in no multiple of the tile's chunk)
        for name in options:
            assert h.ttsamd_set_option(name.encode(), None) == 0
        sets.append({'options': options, 'routes': base64.b64encode(zlib.compress(bytes(out), 9)).decode()})
        print(options, len(all_cases), 'cases, routes', sorted(set(out[0::2])), 'max ksplit', max(out[1::2]))
    with open(os.path.join(REPO, 'tests', 'golden', 'conv_route.json'), 'w') as f:
        json.dump({'grid': GRID, 'sets': sets}, f, indent=0)
        f.write('\n')


if __name__ == '__main__':
    main(sys.argv[1])
