"""The two recurrent model families against float64 through the C ABI (pytest -m gpu): Tacotron2 (csrc/tacotron2.hip: taco_embed_kernel,
the encoder convs, taco_bilstm_kernel, taco_spk_kernel, taco_pm_kernel, the graph path's taco_prenet / lstm / query / energy / context /
proj kernels, taco_decoder_persistent in both modes and in segments, the postnet) and the diacritizer taggers (csrc/tagger.hip:
tagger_embed_kernel, the 1x1 convs, tagger_bilstm_kernel<hard | soft>, tagger_softmax_kernel, the zero-padded channel rows).

References, cases, checker and bounds: tests/recurrent_ref.py -- every run is compared with the float64 oracle (never with another run),
over the valid positions, and must stay within R times the error of the same oracle in float32 on the same data; every output must be
finite, padding included.  tests/test_recurrent_ref_cpu.py shows what that bound rejects.  R per family (Tacotron2 fp32 / fp32 with
TTSAMD_WINO=0 / split bf16, taggers): recurrent_ref.R_*, derived in profiles/r32/NOTES.md."""
import pytest
import torch

import recurrent_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from ttsamd import lib
    assert lib.load().ttsamd_device_ok() == 1
    return torch.device('cuda:0')


_ENGINES = {}


def _taco_engine(name, dev):
    """One engine per set of weights for the whole module: the two memory dims, and the stop-token case's fitted gate."""
    from ttsamd.engine import Tacotron2Engine
    cfg, sd = R.taco_case(name)[:2]
    key = ('taco', cfg['num_speakers'], name if R.TACO_CASES[name].get('stops') is not None else None)
    if key not in _ENGINES:
        _ENGINES[key] = Tacotron2Engine(sd, cfg, device=dev)
    return _ENGINES[key]


def _tagger_engine(kind, dev):
    from ttsamd.engine import TaggerEngine
    if ('tagger', kind) not in _ENGINES:
        _ENGINES['tagger', kind] = TaggerEngine(R.tagger_weights(kind), R.TAGGER_CONFIGS[kind], device=dev)
    return _ENGINES['tagger', kind]


def _route_id(route):
    return 'unset' if route is None else f'persistent{route}'


def _run_taco(dev, ttsopt, name, route, bound, tag, wino=None):
    cfg, sd, tok, sids, lens, steps, seed, stops = R.taco_case(name)
    _, _, want_lens = R.taco_refs(name)
    ttsopt.set('TTSAMD_TACO_PERSISTENT', route)
    for k, v in R.TACO_CASES[name].get('opts', {}).items():
        ttsopt.set(k, v)
    if wino is not None:
        ttsopt.set('TTSAMD_WINO', wino)
    post, mel_lens, align, raw = _taco_engine(name, dev).infer(tok, sids, lens, max_step=steps, dropout_seed=seed, return_raw=True)
    torch.cuda.synchronize()
    assert mel_lens.cpu().tolist() == want_lens.tolist()
    return R.check_taco({'mel_raw': raw, 'mel_post': post, 'alignments': align}, name, bound, f'{tag} {_route_id(route)}')


TACO_RUNS = [(name, route) for name in R.TACO_CASES for route in R.taco_routes(name)]
_taco_ids = [f'{n}-{_route_id(r)}' for n, r in TACO_RUNS]


@pytest.mark.parametrize('name,route', TACO_RUNS, ids=_taco_ids)
def test_tacotron2(dev, ttsopt, name, route):
    """Every case on every decoder route that serves it: the graph path (TTSAMD_TACO_PERSISTENT=0), the persistent decoder with barriers
    (1) and as a dataflow (2) where the geometry fits (B <= 8, L <= 256), else the graph path and the default route, which has to fall
    back to it; T6 once more in segments of 8 steps; the stop-token case with its lengths exact."""
    _run_taco(dev, ttsopt, name, route, R.R_TACO_F32, 'fp32')


@pytest.mark.parametrize('route', R.taco_routes('TP'), ids=_route_id)
def test_tacotron2_direct_convs(dev, ttsopt, route):
    """TP (the postnet at 256 frames x 8 rows) with TTSAMD_WINO=0: every conv on the direct MFMA kernel."""
    _run_taco(dev, ttsopt, 'TP', route, R.R_TACO_DIRECT, 'fp32 WINO=0', wino='0')


X3_RUNS = [(name, route) for name in ('T4', 'T6', 'TP') for route in R.taco_routes(name)]


@pytest.mark.parametrize('name,route', X3_RUNS, ids=[f'{n}-{_route_id(r)}' for n, r in X3_RUNS])
def test_tacotron2_split_bf16(dev, ttsopt, name, route):
    """set_precision('bf16x3'): the encoder and postnet convs take default_precision() at every batch size (csrc/conv_mfma.hip:
    launch_conv hands every launch whose precision is not 0 to the bf16 engine; only FastPitch keeps small batches in fp32)."""
    from ttsamd.engine import set_precision
    set_precision('bf16x3')
    try:
        _run_taco(dev, ttsopt, name, route, R.R_TACO_X3, 'bf16x3')
    finally:
        set_precision('f32')


# ---- taggers ---------------------------------------------------------------------------------------------------------------------

def _run_tagger(dev, ttsopt, kind, B, T, tag, wino=None):
    if wino is not None:
        ttsopt.set('TTSAMD_WINO', wino)
    probs = _tagger_engine(kind, dev).forward(R.tagger_ids(kind, B, T))
    torch.cuda.synchronize()
    return R.check_tagger(probs, kind, B, T, R.R_TAGGER, tag)


TAGGER_RUNS = [(kind, B, T) for kind in ('shakkelha', 'shakkala') for B, T in R.TAGGER_CASES[kind]]


@pytest.mark.parametrize('kind,B,T', TAGGER_RUNS)
def test_tagger(dev, ttsopt, kind, B, T):
    """Both taggers at the smallest shape, at a second embed block, at a second softmax block and at B = 9, T = 300; the probabilities
    within the bound and no arg-max other than float64's outside its margin."""
    _run_tagger(dev, ttsopt, kind, B, T, 'fp32')


@pytest.mark.parametrize('kind', ['shakkelha', 'shakkala'])
def test_tagger_direct_convs(dev, ttsopt, kind):
    _run_tagger(dev, ttsopt, kind, 9, 300, 'fp32 WINO=0', wino='0')


@pytest.mark.parametrize('B,T', R.TAGGER_CASES['padded'])
def test_tagger_padded_geometry(dev, ttsopt, B, T):
    """lstm_hidden (100, 52): Cy = align_up(2H, 32) = 224 / 128 != 2H, the channel rows tagger_forward zero-fills; the packed input
    projections and dense weights carry zero columns for them (tagger_create) and max_c covers the widest padded activation."""
    _run_tagger(dev, ttsopt, 'padded', B, T, 'fp32')
