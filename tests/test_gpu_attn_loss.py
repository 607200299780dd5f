"""GPU: the alignment prior and the alignment scores (csrc/attn_loss.hip) through the C ABI, the engine functions and the drop-ins, against
the golden file of the reference (tests/golden/attn_loss.npz, tools/gen_golden_attn_loss.py) and, for shapes too big to commit, against the
float64 restatement tests/attn_loss_ref.py, which tests/test_attn_loss_cpu.py pins to that file."""
import numpy as np
import pytest
import torch

import attn_loss_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXACT = ((18, 48), (13, 37), (9, 22), (1, 1), (1, 7), (65, 70))                     # (P, M) of the fixture
INTERP = ((48, 18), (37, 13), (22, 9), (149, 29), (150, 30), (249, 49), (250, 50), (49, 9), (51, 11), (2, 1), (1, 3), (1, 1))   # (w, h)


@pytest.fixture(scope='module')
def g(golden):
    return golden('attn_loss')


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _one_rounding(got, want, what):
    """one fp32 rounding of a float64 value whose own relative error (1.2e-11 for the table route, a device exp of a few ulp) is far below
    half an fp32 ulp"""
    err = np.abs(got.astype(np.float64) - want)
    bound = 2.0 ** -23 * np.abs(want) + 1e-37
    print(f'{what}: largest |out - golden| / (2^-23 |golden| + 1e-37) = {float((err / bound).max()):.3f}')
    assert (err <= bound).all(), what


# ------------------------------------------------------------------------------------------------------------------------------ prior ----
@pytest.mark.parametrize('mode', ['exact', 'interpolated'])
def test_prior_against_the_fixture(g, mode):
    from ttsamd import engine as E
    if mode == 'exact':
        in_lens, mel_lens = [p for p, _ in EXACT], [m for _, m in EXACT]
        want = [g[f'exact_{p}_{m}'] for p, m in EXACT]
    else:
        in_lens, mel_lens = [h for _, h in INTERP], [w for w, _ in INTERP]
        want = [g[f'interp_{w}_{h}'] for w, h in INTERP]
    out = E.attention_prior(in_lens, mel_lens, mode=mode)
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(in_lens), max(mel_lens), max(in_lens))
    out = out.cpu().numpy()
    out64 = E.attention_prior(in_lens, mel_lens, mode=mode, dtype=torch.float64).cpu().numpy()
    for b, (p, m) in enumerate(zip(in_lens, mel_lens)):
        _one_rounding(out[b, :m, :p], want[b], (mode, p, m))
        assert np.abs(out64[b, :m, :p] - want[b]).max() <= 1e-12                   # the value before the rounding
        outside = out[b].copy()
        outside[:m, :p] = 0
        assert not outside.any() and not np.signbit(out[b]).any()                  # exactly 0 outside the corner
        alone = E.attention_prior([p], [m], mode=mode).cpu().numpy()                # a ragged batch equals its rows alone, bit for bit
        assert alone.shape == (1, m, p) and np.array_equal(_bits(alone[0]), _bits(out[b, :m, :p]))
    # lengths past the padded size are clamped to it
    wide = E.attention_prior([max(in_lens) + 5], [max(mel_lens) + 9], n_tokens=max(in_lens), n_frames=max(mel_lens), mode=mode)
    full = E.attention_prior([max(in_lens)], [max(mel_lens)], mode=mode)
    assert torch.equal(wide, full)


# (40, 8200): past the 8192 entries the log-factorial table starts with, so it is rebuilt larger
@pytest.mark.parametrize('P,M', [(1024, 1030), (257, 300), (40, 8200)])
def test_exact_prior_against_the_restatement(P, M):
    from ttsamd import engine as E
    out = E.attention_prior([P], [M], mode='exact').cpu().numpy()
    _one_rounding(out[0], R.exact_prior(P, M), ('exact', P, M))


def test_interpolated_prior_against_the_restatement():
    from ttsamd import engine as E
    out = E.attention_prior([97, 200], [430, 860], mode='interpolated').cpu().numpy()
    _one_rounding(out[0, :430, :97], R.interpolated_prior(430, 97), ('interpolated', 430, 97))
    _one_rounding(out[1], R.interpolated_prior(860, 200), ('interpolated', 860, 200))
    assert not out[0, 430:].any() and not out[0, :, 97:].any()


def test_prior_limits_and_dropins(g):
    from models.fastpitch.fastpitch.data_function import BetaBinomialInterpolator, beta_binomial_prior_distribution
    from ttsamd import engine as E
    from ttsamd.lib import TtsAmdError
    with pytest.raises(TtsAmdError, match='scaling = 1'):
        E.attention_prior([5], [9], mode='exact', scaling=2.0)
    with pytest.raises(TtsAmdError, match='interpolated'):
        E.attention_prior([5], [9], mode='nearest')
    got = beta_binomial_prior_distribution(13, 37)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.device.type == 'cpu' and tuple(got.shape) == (37, 13)
    assert np.abs(got.numpy() - g['exact_13_37']).max() <= 1e-12
    ret = BetaBinomialInterpolator()(149, 29)
    assert isinstance(ret, np.ndarray) and ret.dtype == np.float64 and ret.shape == (149, 29)
    assert np.abs(ret - g['interp_149_29']).max() <= 1e-12
    with pytest.raises(TtsAmdError, match='scaling = 1'):
        beta_binomial_prior_distribution(13, 37, scaling=0.5)


# ------------------------------------------------------------------------------------------------------------------------ forward-sum ----
def _nll(lp, in_lens, out_lens, **kw):
    from ttsamd import engine as E
    return E.forward_sum_loss(torch.from_numpy(np.ascontiguousarray(lp)).to(DEV), torch.as_tensor(in_lens), torch.as_tensor(out_lens),
                              **kw).cpu().numpy()


def _close(got, want, rel=1e-9):
    """relative `rel` where finite; the same infinities elsewhere.  The chain is at most T x (a few float64 operations) deep: about 1e-12
    at T = 1030."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.isfinite(got[fin]).all(), (got, want)
    err = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)
    print(f'forward-sum: largest relative error {float(err.max()) if err.size else 0.0:.2e} over {int(fin.sum())} finite rows')
    assert (np.abs(got[fin] - want[fin]) <= rel * np.abs(want[fin])).all(), (got, want)


def test_forward_sum_against_the_fixture(g):
    from models.fastpitch.fastpitch.attn_loss_function import AttentionCTCLoss
    lp, in_lens = g['attn_logprob'], g['in_lens']
    for tag in ('', '_infeasible'):
        out_lens = g['out_lens' + tag]
        nll = _nll(lp, in_lens, out_lens)
        assert nll.dtype == np.float64
        _close(nll, g['ctc_rows64' + tag])
        loss = AttentionCTCLoss()(torch.from_numpy(lp).to(DEV), torch.from_numpy(in_lens), torch.from_numpy(out_lens))
        assert loss.dtype == torch.float64 and loss.dim() == 0 and not loss.requires_grad
        want64, ref32 = float(g['ctc64' + tag]), float(g['ctc32' + tag])
        print(f'AttentionCTCLoss{tag}: {float(loss):.15f}, reference float64 {want64:.15f}, reference float32 {ref32:.8f}: '
              f'|kernel - f64| {abs(float(loss) - want64):.2e}, |f32 - f64| {abs(ref32 - want64):.2e}')
        assert abs(float(loss) - want64) <= 1e-9 * want64
        assert abs(ref32 - want64) >= abs(float(loss) - want64)                     # not merely as good as fp32
    bad = _nll(lp, in_lens, g['out_lens_infeasible'])
    assert np.isposinf(bad[0])                                                      # ... and the scalar above counted it as 0
    assert float(g['ctc64_infeasible']) == pytest.approx(float((bad[1:] / in_lens[1:]).sum() / 4), rel=1e-9)


def _rows(pairs, T, Lt, seed):
    """a ragged batch [B, T, L] of standard normal x 3 with the given (n_in, n_out) rows"""
    rng = np.random.default_rng(seed)
    lp = (rng.standard_normal((len(pairs), T, Lt)) * 3.0).astype(np.float32)
    return lp, [p[0] for p in pairs], [p[1] for p in pairs]


def _want(lp, in_lens, out_lens):
    return R.batch_forward_sum(lp, in_lens, out_lens)


def _pairs(n_ins):
    return [(n, n + d) for n in n_ins for d in (-1, 0, 1, 7)]


# the lane, wave and block edges of the token ownership: one token per lane and up to four waves (L <= 256), two tokens per lane (257),
# three (700), four (1024); per n_in: no path, the single blank-free path, the first frames with freedom
@pytest.fixture(scope='module')
def batches():
    out = {}
    out['L65'] = _rows(_pairs((1, 2, 63, 64, 65)) + [(1, 1), (5, 13), (0, 4), (0, 0), (3, 0)], 72, 65, 1)
    out['L257'] = _rows(_pairs((255, 256, 257)) + [(130, 141)], 264, 257, 2)
    out['L700'] = _rows([(700, 707), (513, 700), (699, 699), (64, 77)], 707, 700, 3)
    out['L1024'] = _rows(_pairs((1024,)) + [(1, 1), (0, 9), (1000, 1035)], 1040, 1024, 4)
    return out


@pytest.mark.parametrize('name', ['L65', 'L257', 'L700', 'L1024'])
def test_forward_sum_against_the_restatement(batches, name):
    lp, in_lens, out_lens = batches[name]
    got = _nll(lp, in_lens, out_lens)
    _close(got, _want(lp, in_lens, out_lens))
    for b, (n, t) in enumerate(zip(in_lens, out_lens)):
        if n == 0:
            assert got[b] == 0.0                                                    # the all-blank path
        elif t < n:
            assert np.isposinf(got[b])                                              # no path (also: no frame)


def test_forward_sum_row_does_not_depend_on_its_batch(batches):
    """the same corner inside another padded size (other tokens per lane, other wave count, other neighbours) gives the same bits"""
    big, _, _ = batches['L1024']
    T, Lt = big.shape[1:]
    for name, picks in (('L65', (2 * 4 + 3, 4 * 4 + 2, 21)), ('L257', (3, 2 * 4 + 3, 12)), ('L700', (0, 1, 3))):
        lp, in_lens, out_lens = batches[name]
        got = _nll(lp, in_lens, out_lens)
        moved = np.random.default_rng(9).standard_normal((len(picks), T, Lt)).astype(np.float32)
        for i, b in enumerate(picks):
            moved[i, :lp.shape[1], :in_lens[b]] = lp[b, :, :in_lens[b]]
        there = _nll(moved, [in_lens[b] for b in picks], [out_lens[b] for b in picks])
        for i, b in enumerate(picks):
            alone = _nll(lp[b:b + 1, :max(out_lens[b], 1), :in_lens[b]], [in_lens[b]], [out_lens[b]])
            assert np.isfinite(got[b]) and _bits(got[b:b + 1])[0] == _bits(there[i:i + 1])[0] == _bits(alone)[0], (name, b)


def test_forward_sum_limits():
    from ttsamd import engine as E
    from ttsamd.lib import TtsAmdError
    with pytest.raises(TtsAmdError, match='1025 tokens'):
        E.forward_sum_loss(torch.zeros(1, 2, 1025, device=DEV), torch.tensor([2]), torch.tensor([2]))
    lib = E.L.load()
    assert lib.ttsamd_attn_ctc_loss_workspace_bytes(1, 2, 1025) == -1
    x = torch.zeros(1, 2, 1025, device=DEV)
    ws = torch.zeros(1024, dtype=torch.uint8, device=DEV)
    lens = torch.tensor([2], device=DEV)
    nll = torch.zeros(1, dtype=torch.float64, device=DEV)
    rc = lib.ttsamd_attn_ctc_loss(E._ptr(x), E._ptr(lens), E._ptr(lens), 1, 2, 1025, -1.0, E._ptr(nll), E._ptr(ws), 1024, E._stream())
    assert rc == -1 and b'1025 tokens' in lib.ttsamd_last_error()                   # TTSAMD_EINVAL
    with pytest.raises(TtsAmdError, match='backward'):
        E.forward_sum_loss(torch.zeros(1, 2, 3, device=DEV, requires_grad=True), torch.tensor([2]), torch.tensor([2]))
    # another blank: against the restatement
    lp, in_lens, out_lens = _rows([(7, 12), (3, 3)], 12, 7, 5)
    _close(_nll(lp, in_lens, out_lens, blank_logprob=-4.5), R.batch_forward_sum(lp, in_lens, out_lens, -4.5))


# ----------------------------------------------------------------------------------------------------------------------- binarization ----
def test_binarization(g, golden):
    from models.fastpitch.fastpitch.attn_loss_function import AttentionBinarizationLoss
    from ttsamd import engine as E
    from ttsamd.lib import TtsAmdError
    a = golden('aligner')
    for tag in ('', '_prior'):
        hard, soft = torch.from_numpy(a['attn_hard' + tag].astype(np.float32)).to(DEV), torch.from_numpy(a['attn_soft' + tag]).to(DEV)
        sum_log, count = E.binarization_loss(hard, soft)
        ws, wc = R.binarization(a['attn_hard' + tag], a['attn_soft' + tag])
        assert sum_log.dtype == count.dtype == torch.float64 and np.array_equal(count.cpu().numpy(), wc)
        assert (np.abs(sum_log.cpu().numpy() - ws) <= 1e-12 * np.abs(ws)).all()
        loss = AttentionBinarizationLoss()(hard, soft)
        want64, ref32 = float(g['bin64' + tag]), float(g['bin32' + tag])
        print(f'AttentionBinarizationLoss{tag}: {float(loss):.15f}, reference float64 {want64:.15f}, reference float32 {ref32:.8f}')
        assert loss.dtype == torch.float64 and not loss.requires_grad and abs(float(loss) - want64) <= 1e-12 * want64
        again, _ = E.binarization_loss(hard, soft)
        assert torch.equal(sum_log, again)                                          # a fixed order: the same bits
    # more than one pass of the block over a row, a ragged batch, a soft value of 0 on the path
    rng = np.random.default_rng(6)
    B, T, Lt = 3, 300, 257
    soft = rng.random((B, T, Lt)).astype(np.float32) ** 4
    hard = np.zeros((B, T, Lt), np.float32)
    for b, t in enumerate((300, 123, 0)):
        hard[b, np.arange(t), np.sort(rng.integers(0, Lt, t))] = 1
    soft[0, 7, hard[0, 7].argmax()] = 0.0
    sum_log, count = E.binarization_loss(torch.from_numpy(hard).to(DEV), torch.from_numpy(soft).to(DEV))
    ws, wc = R.binarization(hard, soft)
    assert np.array_equal(count.cpu().numpy(), wc) and wc.tolist() == [300, 123, 0]
    assert (np.abs(sum_log.cpu().numpy() - ws) <= 1e-12 * np.abs(ws)).all() and float(sum_log[2]) == 0.0
    one = np.zeros((1, 2, 2), np.float32)
    s1, c1 = E.binarization_loss(torch.eye(2, device=DEV)[None], torch.from_numpy(one).to(DEV), eps=1e-12)
    assert float(c1[0]) == 2 and float(s1[0]) == pytest.approx(2 * np.log(1e-12), rel=1e-15)
    with pytest.raises(TtsAmdError, match='backward'):
        E.binarization_loss(torch.eye(2, device=DEV)[None], torch.zeros(1, 2, 2, device=DEV, requires_grad=True))


# ------------------------------------------------------------------------------------------------------------------------- end to end ----
@pytest.fixture(scope='module')
def model(golden, tmp_path_factory):
    import text
    from models.fastpitch.networks import FastPitch
    from ttsamd import synth
    from ttsamd.config import NET_CONFIG
    a = golden('aligner')
    sd = synth.fastpitch_state_dict()
    sd.update(synth.fastpitch_aligner_state_dict(gain=8.0))
    path = tmp_path_factory.mktemp('attn_loss') / 'fp.pth'
    torch.save({'model': {k: torch.from_numpy(v.copy()) for k, v in sd.items()}, 'config': dict(NET_CONFIG), 'symbols': list(text.symbols)}, path)
    return FastPitch(str(path)).to(DEV), a


def test_align_builds_the_prior_itself(model):
    from ttsamd import engine as E
    m, a = model
    T, Lt = a['mel'].shape[2], a['ids'].shape[1]
    for mode in ('exact', 'interpolated'):
        prior = E.attention_prior(a['in_lens'], a['mel_lens'], n_tokens=Lt, n_frames=T, mode=mode)
        by_name = m.align(a['ids'], a['mel'], a['mel_lens'], attn_prior=mode, return_attn=True)
        by_tensor = m.align(a['ids'], a['mel'], a['mel_lens'], attn_prior=prior, return_attn=True)
        for k in ('dur_tgt', 'attn_soft', 'attn_hard', 'attn_logprob'):
            assert torch.equal(getattr(by_name, k), getattr(by_tensor, k)), (mode, k)
        assert np.array_equal(by_name.dur_tgt.sum(1).cpu().numpy(), a['mel_lens'].astype(np.float32))
    none = m.align(a['ids'], a['mel'], a['mel_lens'])
    assert np.array_equal(none.dur_tgt.cpu().numpy(), a['dur'])                     # None behaves as before


def test_alignment_score(model, g):
    from models.fastpitch.fastpitch.attn_loss_function import AttentionBinarizationLoss, AttentionCTCLoss
    m, a = model
    in_lens, mel_lens = torch.from_numpy(a['in_lens']), torch.from_numpy(a['mel_lens'])
    sc = m.alignment_score(a['ids'], a['mel'], a['mel_lens'])
    res = m.align(a['ids'], a['mel'], a['mel_lens'], attn_prior='interpolated', return_attn=True)
    assert sc.forward_sum.dtype == sc.binarization.dtype == torch.float64 and tuple(sc.forward_sum.shape) == tuple(sc.binarization.shape) == (3,)
    assert torch.equal(sc.dur_tgt, res.dur_tgt) and bool(torch.isfinite(sc.forward_sum).all()) and bool(torch.isfinite(sc.binarization).all())
    ctc, binl = AttentionCTCLoss(), AttentionBinarizationLoss()
    assert torch.equal(sc.ctc_loss, ctc(res.attn_logprob, in_lens, mel_lens)) and torch.equal(sc.bin_loss, binl(res.attn_hard, res.attn_soft))
    for b in range(3):
        assert torch.equal(sc.forward_sum[b], ctc(res.attn_logprob[b:b + 1], in_lens[b:b + 1], mel_lens[b:b + 1]))
        assert torch.equal(sc.binarization[b], binl(res.attn_hard[b:b + 1], res.attn_soft[b:b + 1]))
    # texts that do not belong to their recordings cost more: rows 1 and 2 exchange their ids.  The float64 restatement of the aligner
    # shows the ordering with the recorded margin (tools/gen_golden_attn_loss.py); the fp32 attention sits within a few 1e-5 of it per
    # cell, orders of magnitude below that margin
    perm = g['swap_perm']
    sw = m.alignment_score(a['ids'][perm], a['mel'], a['mel_lens'])
    matched, swapped = sc.forward_sum.cpu().numpy(), sw.forward_sum.cpu().numpy()
    print(f'forward-sum per token: matched {matched.tolist()} (float64 restatement {g["swap_matched"].tolist()}), texts of rows 1 and 2 swapped '
          f'{swapped.tolist()} ({g["swap_swapped"].tolist()}); recorded margin {float(g["swap_margin"]):.3f}')
    assert ((swapped - matched)[1:] >= 0.5 * float(g['swap_margin'])).all()
    # a cell of attn_logprob is within 4 recorded floors of float64 (tests/test_gpu_aligner.py); d per cell moves a frame's log-softmax by
    # at most 2 d, and a path has mel_len frames
    bound = 8 * float(a['floor_attn_logprob_prior']) * a['mel_lens'] / a['in_lens']
    assert (np.abs(matched - g['swap_matched']) <= bound).all() and (np.abs(swapped - g['swap_swapped']) <= bound[perm]).all()
    no_prior = m.alignment_score(a['ids'], a['mel'], a['mel_lens'], attn_prior=None)
    assert np.array_equal(no_prior.dur_tgt.cpu().numpy(), a['dur'])
