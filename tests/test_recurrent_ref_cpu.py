"""What the bound of tests/test_gpu_recurrent.py rejects, shown without a GPU: every mutant of tests/recurrent_ref.py, run in float32 on
every case it can show in, misses the largest fp32 bound of its model; the unmutated float32 copy passes at R = 1; and the copy the
mutants are switches of is the oracle bit for bit in float64."""
import pytest
import torch

import diac_oracle as DO
import recurrent_ref as R

R_TACO = max(R.R_TACO_F32, R.R_TACO_DIRECT)


def _taco_e_ref(name, key):
    r64, r32, mel_lens = R.taco_refs(name)
    lens = R.TACO_CASES[name]['lens'] if key == 'alignments' else mel_lens.tolist()
    if key == 'alignments' and R.TACO_CASES[name].get('stops') is not None:      # frames before each row's stop
        return max(R._max_err(r32[key][b:b + 1, :n], r64[key][b:b + 1, :n], lens[b:b + 1]) for b, n in enumerate(mel_lens.tolist()))
    return R._max_err(r32[key], r64[key], lens)


@pytest.mark.parametrize('name', list(R.TACO_CASES))
def test_taco_reference_error_is_positive(name):
    """e_ref > 0 for every compared tensor, except where float32 is exact by construction: a batch of one-token rows, whose attention
    is 1.0 (T1's alignments)."""
    for key in ('mel_raw', 'mel_post', 'alignments'):
        e = _taco_e_ref(name, key)
        print(f'{name} {key} e_ref {e:.3e}')
        if key == 'alignments' and max(R.TACO_CASES[name]['lens']) == 1:
            assert e == 0.0
        else:
            assert e > 0.0, (name, key)


@pytest.mark.parametrize('kind,B,T', [(k, B, T) for k, shapes in R.TAGGER_CASES.items() for B, T in shapes])
def test_tagger_reference_error_is_positive(kind, B, T):
    r64, r32 = R.tagger_refs(kind, B, T)
    e = float((r32.double() - r64).abs().max())
    print(f'{kind} ({B}, {T}) probs e_ref {e:.3e}')
    assert e > 0.0
    # float32 takes float64's decision wherever float64's margin exceeds its own rounding error
    top = r64.topk(2, dim=-1).values
    sure = (top[..., 0] - top[..., 1]) > e
    assert not bool(((r32.argmax(-1) != r64.argmax(-1)) & sure).any())


def _got(out):
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize('mut', list(R.TACO_MUTANTS))
def test_taco_mutant_is_rejected(mut):
    cases = R.taco_mutant_cases(mut)
    assert cases, f'mutant {mut} applies to no case'
    print(f'{mut}: cases {cases}')
    for name in cases:
        out, mel_lens = R.taco_mutant(name, mut)
        if mel_lens.tolist() != R.taco_refs(name)[2].tolist():        # the GPU test asserts the lengths exactly: a rejection already
            assert R.TACO_CASES[name].get('stops') is not None
            print(f'mutant {mut} {name} mel_lens {mel_lens.tolist()}, reference {R.taco_refs(name)[2].tolist()}')
            continue
        with pytest.raises(AssertionError, match='max-abs'):
            R.check_taco(_got(out), name, R_TACO, f'mutant {mut}')


@pytest.mark.parametrize('mut', list(R.TAGGER_MUTANTS))
def test_tagger_mutant_is_rejected(mut):
    cases = R.tagger_mutant_cases(mut)
    assert cases, f'mutant {mut} applies to no case'
    print(f'{mut}: cases {cases}')
    for kind, B, T in cases:
        probs = R.tagger_run(kind, B, T, torch.float32, mut=mut)
        with pytest.raises(AssertionError, match='max-abs'):
            R.check_tagger(probs, kind, B, T, R.R_TAGGER, f'mutant {mut}')


@pytest.mark.parametrize('name', list(R.TACO_CASES))
def test_taco_unmutated_copy_passes_at_1(name):
    out, mel_lens = R.taco_mutant(name, None)
    assert mel_lens.tolist() == R.taco_refs(name)[2].tolist()
    R.check_taco(_got(out), name, 1, 'float32 copy')


@pytest.mark.parametrize('kind,B,T', [(k, B, T) for k, shapes in R.TAGGER_CASES.items() for B, T in shapes])
def test_tagger_unmutated_copy_passes_at_1(kind, B, T):
    R.check_tagger(R.tagger_run(kind, B, T, torch.float32, oracle=False), kind, B, T, 1, 'float32 copy')


def test_taco_copy_is_the_oracle():
    """float64, T3: the copy and taco_oracle.tacotron2_infer agree to the last bit (mel_raw: with the oracle's traced projection)."""
    out, mel_lens = R.taco_mutant('T3', None, torch.float64)
    r64, _, want_lens = R.taco_refs('T3')
    assert mel_lens.tolist() == want_lens.tolist()
    for key in ('mel_raw', 'mel_post', 'alignments'):
        assert out[key].dtype == torch.float64 and torch.equal(out[key], r64[key]), key


@pytest.mark.parametrize('kind', ['shakkelha', 'shakkala'])
def test_tagger_copy_is_the_oracle(kind):
    """float64, (2, 65): tagger_forward and diac_oracle's two functions agree to the last bit."""
    fn = DO.shakkelha_forward if kind == 'shakkelha' else DO.shakkala_forward
    W = R._cast(R.tagger_weights(kind), torch.float64)
    want = fn(W, R.tagger_ids(kind, 2, 65))
    got = R.tagger_run(kind, 2, 65, torch.float64, oracle=False)
    assert got.dtype == torch.float64 and torch.equal(got, want)
    assert torch.equal(R.tagger_refs(kind, 2, 65)[0], want)
