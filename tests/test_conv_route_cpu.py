"""CPU: the routing of the exact-fp32 conv launches (csrc/conv_route.hip: conv_route, asked through ttsamd_conv1d_route) is the routing
the launchers had when each of them decided for itself.  tests/golden/conv_route.json holds, for every case of a grid and every option
set, the (route, ksplit) that ttsamd_conv_last_launch reported after ttsamd_conv1d_splitk in a build of the commit BEFORE conv_route.hip
whose launch lines did nothing (tools/gen_golden_conv_route.py made it from that build, never from the code under test): one zlib +
base64 string per option set, one byte pair per case in the order of cases(); route 255 = that build rejected the call, and the query
must reject it too."""
import base64
import itertools
import json
import os
import zlib

from conftest import GOLDEN


def cases(grid):
    """the grid's cases in golden order: (batch, cin, cout, k, dilation, lin, in_slope, relu_out, has_res, mode, splitk_floats)"""
    for k, (cin, cout), lin, batch in itertools.product(grid['k'], grid['channels'], grid['lin'], grid['batch']):
        for dil in ([1] + grid['dilation_k3_7_11'] if k in (3, 7, 11) else [1]):
            # none / residual mode 0 / residual mode 2 / relu_out 2 (k = 1 only); the entry rejects relu_out with an accumulate mode
            for relu_out, has_res, mode in [(0, 0, 0), (0, 1, 0), (0, 1, 2)] + ([(2, 0, 0)] if k == 1 else []):
                for slope, skf in itertools.product(grid['in_slope'], grid['splitk_floats']):
                    yield batch, cin, cout, k, dil, lin, slope, relu_out, has_res, mode, skf


def load_golden():
    with open(os.path.join(GOLDEN, 'conv_route.json')) as f:
        g = json.load(f)
    return g['grid'], [(s['options'], zlib.decompress(base64.b64decode(s['routes']))) for s in g['sets']]


def test_golden_covers_every_route():
    """a golden made with a broken stub (nothing recorded, everything on one route) fails here"""
    grid, sets = load_golden()
    n = sum(1 for _ in cases(grid))
    seen = set()
    for _, blob in sets:
        assert len(blob) == 2 * n
        seen |= set(zip(blob[0::2], blob[1::2]))
    assert {r for r, _ in seen} >= {0, 1, 2, 3, 4, 7, 8}, sorted({r for r, _ in seen})
    assert any(r == 0 and ks > 1 for r, ks in seen) and any(r == 3 and ks > 1 for r, ks in seen)


def test_route_query_matches_the_launchers_it_replaced():
    import ctypes as C
    from ttsamd import lib
    h = lib.load()
    grid, sets = load_golden()
    all_cases = list(cases(grid))
    route, ksplit = C.c_int32(), C.c_int32()
    pr, pk = C.byref(route), C.byref(ksplit)
    query = h.ttsamd_conv1d_route
    for options, blob in sets:
        try:
            for name, value in options.items():
                lib.set_option(name, value)
            got = bytearray(len(blob))
            for i, (batch, cin, cout, k, dil, lin, slope, relu_out, has_res, mode, skf) in enumerate(all_cases):
                if query(batch, cin, cout, k, dil, lin, slope, relu_out, has_res, mode, skf, pr, pk) == 0:
                    got[2 * i], got[2 * i + 1] = route.value, ksplit.value
                else:
                    got[2 * i], got[2 * i + 1] = 255, 0
        finally:
            for name in options:
                lib.set_option(name, None)
        if bytes(got) != blob:
            bad = [i for i in range(len(all_cases)) if got[2 * i:2 * i + 2] != blob[2 * i:2 * i + 2]]
            for i in bad[:10]:
                print(f'{options} (batch, cin, cout, k, dil, lin, slope, relu_out, has_res, mode, splitk_floats) = {all_cases[i]}: '
                      f'(route, ksplit) = {tuple(got[2 * i:2 * i + 2])}, golden {tuple(blob[2 * i:2 * i + 2])}')
            raise AssertionError(f'{options}: {len(bad)} of {len(all_cases)} cases route differently')
