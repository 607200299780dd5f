"""CPU: the float64 restatement of the alignment prior and the alignment losses (tests/attn_loss_ref.py) against the golden file that
tools/gen_golden_attn_loss.py wrote with scipy and the reference's loss module; the host-side table of the prior kernel; the drop-ins'
host-side parts.  No compute on a device."""
import inspect
import math

import numpy as np
import pytest

import attn_loss_ref as R

EXACT = ((18, 48), (13, 37), (9, 22), (1, 1), (1, 7), (65, 70))
INTERP = ((48, 18), (37, 13), (22, 9), (149, 29), (150, 30), (249, 49), (250, 50), (49, 9), (51, 11), (2, 1), (1, 3), (1, 1))


@pytest.fixture(scope='module')
def g(golden):
    return golden('attn_loss')


def test_exact_prior_equals_scipy(g):
    for P, M in EXACT:
        want = g[f'exact_{P}_{M}']
        got = R.exact_prior(P, M)
        assert got.shape == want.shape == (M, P)
        assert np.abs(got - want).max() <= 1e-12, (P, M)
    # n = P, not P - 1: a row leaves the mass of k = P out
    assert abs(R.exact_prior(9, 22).sum(axis=1) - 1).max() > 1e-3


def test_interpolated_prior_equals_scipy_zoom(g):
    for w, h in INTERP:
        want = g[f'interp_{w}_{h}']
        got = R.interpolated_prior(w, h)
        assert got.shape == want.shape == (w, h)
        assert np.abs(got - want).max() <= 1e-12, (w, h)


def test_forward_sum_equals_the_reference(g):
    lp, in_lens = g['attn_logprob'], g['in_lens']
    for tag in ('', '_infeasible'):
        rows = g['ctc_rows64' + tag]
        got = R.batch_forward_sum(lp, in_lens, g['out_lens' + tag])
        for a, b in zip(got, rows):
            assert (np.isinf(a) and np.isinf(b) and a > 0) or abs(a - b) <= 1e-10 * abs(b), (tag, a, b)
        assert abs(R.ctc_mean(got, in_lens) - float(g['ctc64' + tag])) <= 1e-10 * float(g['ctc64' + tag])
    # the infeasible row is inf, and the reference's mean counts it as 0
    bad = R.batch_forward_sum(lp, in_lens, g['out_lens_infeasible'])
    assert np.isposinf(bad[0]) and np.isfinite(bad[1:]).all()
    assert R.ctc_mean(bad, in_lens) == pytest.approx(float((bad[1:] / in_lens[1:]).sum() / 4), rel=1e-15)
    assert float(g['ctc64_infeasible']) < float(g['ctc64'])
    # no token: the all-blank path; no frame: no path
    assert R.forward_sum(lp[0, 0], 0, 5) == 0.0 and np.isposinf(R.forward_sum(lp[0, 0], 3, 0))


def test_binarization_equals_the_reference(g, golden):
    a = golden('aligner')
    for tag in ('', '_prior'):
        sum_log, count = R.binarization(a['attn_hard' + tag], a['attn_soft' + tag])
        assert np.array_equal(count, a['mel_lens'].astype(np.float64))
        got, want = -sum_log.sum() / count.sum(), float(g['bin64' + tag])
        assert abs(got - want) <= 1e-12 * want
    soft = np.zeros((1, 2, 2), np.float32)
    sum_log, count = R.binarization(np.eye(2, dtype=np.float32)[None], soft)       # a soft value of 0 on the path: log(eps)
    assert count[0] == 2 and sum_log[0] == pytest.approx(2 * math.log(1e-12), rel=1e-15)


def test_swapped_texts_cost_more_in_the_fixture(g):
    assert float(g['swap_margin']) > 0.5 and g['swap_perm'].tolist() == [0, 2, 1]
    assert ((g['swap_swapped'] - g['swap_matched'])[1:] >= float(g['swap_margin'])).all()
    assert g['swap_swapped'][0] == g['swap_matched'][0]


def test_log_factorial_table():
    from ttsamd.engine import attn_prior_tables
    n = 5200                                                                        # 1024 tokens + 4096 frames + margin
    lf = attn_prior_tables(n)
    want = np.array([math.lgamma(k + 1.0) for k in range(n)])
    assert lf.dtype == np.float64 and lf.shape == (n,) and lf[0] == 0.0 and lf[1] == 0.0
    assert (np.abs(lf - want) <= 4 * np.spacing(np.abs(want))).all()
    from ttsamd.lib import TtsAmdError
    with pytest.raises(TtsAmdError):
        attn_prior_tables(0)


def test_interpolator_rounds_halves_to_even():
    from models.fastpitch.fastpitch.data_function import BetaBinomialInterpolator, beta_binomial_prior_distribution
    it = BetaBinomialInterpolator()
    assert [it.round(w, 100) for w in (49, 149, 249)] == [100, 200, 200]              # (w + 1) / 100 = 0.5, 1.5, 2.5
    assert [it.round(h, 20) for h in (9, 29, 49)] == [20, 40, 40]
    assert [it.round(w, 100) for w in (1, 150, 250, 430)] == [100, 200, 300, 400]
    assert [R.round_to(w, 100) for w in (49, 149, 249)] == [100, 200, 200]
    assert list(inspect.signature(beta_binomial_prior_distribution).parameters) == ['phoneme_count', 'mel_count', 'scaling']
    assert list(inspect.signature(BetaBinomialInterpolator.__init__).parameters) == ['self', 'round_mel_len_to', 'round_text_len_to']


def test_dropins_and_methods_are_there():
    from models.fastpitch.fastpitch import attn_loss_function as A
    from models.fastpitch.networks import AlignmentScore, FastPitch
    from ttsamd import engine as E
    assert inspect.signature(A.AttentionCTCLoss.__init__).parameters['blank_logprob'].default == -1
    assert list(inspect.signature(A.AttentionCTCLoss.forward).parameters) == ['self', 'attn_logprob', 'in_lens', 'out_lens']
    assert list(inspect.signature(A.AttentionBinarizationLoss.forward).parameters) == ['self', 'hard_attention', 'soft_attention', 'eps']
    assert inspect.signature(A.AttentionBinarizationLoss.forward).parameters['eps'].default == 1e-12
    for cls in (A.AttentionCTCLoss, A.AttentionBinarizationLoss):
        assert 'grad' in cls.__doc__
    p = inspect.signature(FastPitch.alignment_score).parameters
    assert list(p) == ['self', 'ids_or_text', 'mel', 'mel_lens', 'attn_prior'] and p['attn_prior'].default == 'interpolated'
    assert AlignmentScore._fields == ('forward_sum', 'binarization', 'dur_tgt', 'ctc_loss', 'bin_loss')
    for name in ('attention_prior', 'forward_sum_loss', 'binarization_loss', 'attn_prior_tables'):
        assert callable(getattr(E, name))
    assert inspect.signature(E.forward_sum_loss).parameters['blank_logprob'].default == -1
    assert inspect.signature(E.attention_prior).parameters['mode'].default == 'interpolated'


def test_no_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        return
    from ttsamd import engine as E
    from ttsamd.lib import TtsAmdError
    with pytest.raises(TtsAmdError):
        E.attention_prior([3], [5])
    with pytest.raises(TtsAmdError):
        E.forward_sum_loss(torch.zeros(1, 2, 2), [2], [2])
