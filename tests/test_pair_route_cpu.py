"""CPU: the routing of the fp32 ResBlock1 pairs (csrc/conv_route.hip: pair_route, asked through ttsamd_resblock_pair_route) is the
routing of the code it replaced.  tests/golden/hifigan_launches.json holds the launches of hifigan_forward as the commit before
pair_route logged them (tools/gen_golden_hifigan_launches.py); here every fp32 ResBlock1 forward of it is walked in the forward's order
-- stage, branch, dilation -- and the query must name, for each pair, exactly the launch that was logged."""
from test_gpu_hifigan_launches import SHAPES, load_golden

from ttsamd.config import HIFIGAN_CONFIG

# log name -> (kernel, ntw, wino_phases, points)
ROUTE_OF_NAME = {'': (0, 0, 0, 0), 'fused_pair': (1, 0, 0, 0), 'fused_pair2': (2, 2, 0, 0), 'fused_pair2n': (2, 1, 0, 0),
                 'fused_pair2w': (2, 2, 1, 0), 'fused_pair2ww': (2, 2, 2, 0), 'fused_pair4': (3, 0, 0, 6), 'fused_pair44': (3, 0, 0, 7)}


def logged_pairs(lines, batch, frames):
    """(channels, k, dilation, L, log name or '' for two conv launches) per pair, in the forward's order"""
    cfg = HIFIGAN_CONFIG
    it = iter(lines)
    next(it)                                               # conv_pre
    ch, L = cfg['upsample_initial_channel'], frames
    for u in cfg['upsample_rates']:
        next(it)                                           # the upsampler
        ch, L = ch // 2, L * u
        for k, dils in zip(cfg['resblock_kernel_sizes'], cfg['resblock_dilation_sizes']):
            for d in dils:
                f = next(it).split(',')
                name = f[0] if f[0].startswith('fused_pair') else ''
                if not name:
                    f2 = next(it).split(',')               # c2 of an un-fused pair: the launch with the residual
                    assert (f[6], f2[6]) == ('0', '1') and f2[1:6] == f[1:6]
                assert [int(v) for v in f[1:6]] == [k, ch, ch, L, batch], (f, k, ch, L, batch)
                yield ch, k, d, L, name
    assert next(it, None) is None                          # (conv_post is not logged)


def test_pair_route_answers_what_the_parent_launched(ttsopt):
    from ttsamd.engine import pair_route
    n_pairs, seen = 0, set()
    for gen, prec, options, si, lines in load_golden():
        if (gen, prec) != ('v1', 'f32'):
            continue
        for name, value in options.items():
            ttsopt.set('TTSAMD_' + name, value)
        batch, frames, _ = SHAPES[si]
        for ch, k, d, L, name in logged_pairs(lines, batch, frames):
            want = dict(zip(('kernel', 'ntw', 'wino_phases', 'points'), ROUTE_OF_NAME[name]), name=name)
            got = pair_route(batch, ch, k, L, dilation=d)
            assert got == want, f'{options} batch {batch} x {frames} frames, C = {ch}, k = {k}, dilation {d}: {got}, the parent launched {want}'
            n_pairs += 1
            seen.add(name)
        for name in options:
            ttsopt.set('TTSAMD_' + name, None)
    assert n_pairs == 13 * 3 * 36 and seen == set(ROUTE_OF_NAME)


def test_pair_route_is_an_fp32_answer(ttsopt):
    """under the bf16 precisions no fp32 pair kernel runs: the query says 'two conv launches' for a pair the fp32 engine fuses"""
    from ttsamd import lib
    from ttsamd.engine import pair_route
    ttsopt.set('TTSAMD_FUSED2_MASK', '1ff')
    assert pair_route(8, 32, 7, 40960, dilation=3)['name'] == 'fused_pair44'
    h = lib.load()
    assert h.ttsamd_set_precision(1) == 0
    try:
        assert pair_route(8, 32, 7, 40960, dilation=3) == {'kernel': 0, 'ntw': 0, 'wino_phases': 0, 'points': 0, 'name': ''}
    finally:
        assert h.ttsamd_set_precision(0) == 0
