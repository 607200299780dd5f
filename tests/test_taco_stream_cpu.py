"""CPU: the host rules of Tacotron2 streaming -- the planner of a vocoder stream that grows (ttsamd.stream.next_growing_chunk), the
causal form of the wrapper's end-of-utterance cut (models.tacotron2.networks.cut_bound) and the postnet's halo, on the oracle's postnet
in float64.  No GPU, no library call."""
import numpy as np
import pytest
import torch


# ---- growing planner ----------------------------------------------------------------------------------------------------------------

def _schedules(T):
    yield 'one at a time', [1] * T
    yield 'blocks of 8', [8] * (T // 8) + ([T % 8] if T % 8 else [])
    yield 'all at once', [T]
    yield 'uneven', [n for n in ([3, 11, 1, 29] * (T // 4 + 1)) if n][:T]            # clipped to T below


def _run_growing(T, arrivals, first, chunk, hl, hr):
    """feed an utterance of T frames in `arrivals`, release whatever the planner allows after each arrival (as step() after step() would),
    finish, drain -> [(chunk, frames known at its release, end known at its release)]"""
    from ttsamd.stream import next_growing_chunk
    released, pos, known = [], 0, 0

    def drain(ended):
        nonlocal pos
        while True:
            c = next_growing_chunk(pos, known, ended, first, chunk, hl, hr)
            if c is None:
                return
            released.append((c, known, ended))
            pos = c[0] + c[1]
    for n in arrivals:
        n = min(n, T - known)
        known += n
        drain(False)
        if known == T:
            break
    assert known == T
    drain(True)
    return released


@pytest.mark.parametrize('first,chunk', [(1, 1), (4, 8), (32, 64), (5, 3)])
@pytest.mark.parametrize('hl,hr', [(0, 0), (13, 13), (29, 41)])
def test_growing_planner_releases_exactly_plan_chunks(first, chunk, hl, hr):
    """every T in 1 ... 200, four arrival schedules: the released chunks are plan_chunks(T, ...) in order -- none twice, none missing --,
    no window reaches past the frames that have arrived, and without the end known no window touches it"""
    from ttsamd.stream import plan_chunks
    for T in range(1, 201):
        want = plan_chunks(T, first, chunk, hl, hr)
        for name, arrivals in _schedules(T):
            got = _run_growing(T, arrivals, first, chunk, hl, hr)
            assert [c for c, _, _ in got] == want, (T, name)
            for (s, n, ws, wl), known, ended in got:
                assert ws + wl <= known, (T, name, (s, n, ws, wl), known)
                assert ended or ws + wl == s + n + hr            # a complete right halo: the window does not end at the utterance's end
            starts = [c[0] for c, _, _ in got]
            assert len(set(starts)) == len(starts)


def test_growing_planner_holds_the_last_core_until_the_end_is_known():
    """with the end unknown something is always kept back (the chunk that will carry `last`), and nothing comes after the last core"""
    from ttsamd.stream import growing_lookahead, next_growing_chunk, plan_chunks
    assert growing_lookahead(64, 16) == 32 and growing_lookahead(8, 16) == 16 and growing_lookahead(1, 0) == 1
    for first, chunk, hr in ((1, 1, 0), (4, 8, 13), (5, 3, 0)):
        for T in range(1, 60):
            got = _run_growing(T, [1] * T, first, chunk, 0, hr)
            assert got[-1][2] is True and got[-1][0] == plan_chunks(T, first, chunk, 0, hr)[-1]
            assert next_growing_chunk(T, T, True, first, chunk, 0, hr) is None
    with pytest.raises(ValueError):
        next_growing_chunk(5, 3, False, 4, 8, 0, 0)            # more released than known


# ---- cut bound ----------------------------------------------------------------------------------------------------------------------

def _sequences(n, seed):
    g = np.random.default_rng(seed)
    for i in range(n):
        T = int(g.integers(1, 301))
        kind = i % 5
        ps = g.random(T).astype(np.float32) + np.float32(1e-6)
        if kind == 1:
            ps = np.sort(ps)                                     # monotone rising: the cut is late
        elif kind == 2:
            ps = np.sort(ps)[::-1].copy()                        # monotone falling: the cut is frame 0
        elif kind == 3:
            ps[int(g.integers(0, max(T // 4, 1)))] += np.float32(5.0)      # an early spike
        elif kind == 4:
            ps[:] = ps[0]                                        # constant
        yield torch.from_numpy(ps)


def _n_end(ps):
    return int((ps >= 0.8 * ps.max()).nonzero()[0])              # truncate_mel's own expression


def test_cut_bound_is_a_monotone_lower_bound_that_ends_at_the_cut():
    from models.tacotron2.networks import cut_bound
    for ps in _sequences(1000, 7):
        n_end, state, prev = _n_end(ps), None, 0
        for s in range(1, ps.numel() + 1):
            c, state = cut_bound(ps[s - 1:s], state)
            assert prev <= c <= n_end, (s, prev, c, n_end)
            assert c < s
            prev = c
        assert prev == n_end


def test_cut_bound_in_blocks_equals_frame_by_frame():
    from models.tacotron2.networks import cut_bound
    for ps in _sequences(50, 11):
        one, state = [], None
        for s in range(ps.numel()):
            c, state = cut_bound(ps[s:s + 1], state)
            one.append(c)
        state = None
        for s0 in range(0, ps.numel(), 8):
            c, state = cut_bound(ps[s0:s0 + 8], state)
            assert c == one[min(s0 + 8, ps.numel()) - 1]


def test_streamed_cut_reproduces_truncate_mel():
    """the host model of what tts_stream feeds the vocoder -- frames below min(c_s, s - halo) as they come, the rest and the three repeated
    frames at the end -- is truncate_mel's mel, frame for frame, and frames do leave before the end where the bound allows"""
    from models.tacotron2.networks import stream_truncate_mel, truncate_mel
    g = torch.Generator().manual_seed(3)
    early = 0
    for ps in _sequences(200, 19):
        T = ps.numel()
        mel = torch.randn(80, T, generator=g)
        if _n_end(ps) == 0:
            continue                                             # an empty cut raises in both (checked below)
        for halo, block in ((0, 8), (10, 8), (10, 1), (10, 64)):
            got, trace = stream_truncate_mel(mel, ps, halo=halo, block=block)
            assert torch.equal(got, truncate_mel(mel, ps)), (T, halo, block)
            assert trace == sorted(trace) and trace[-1] == _n_end(ps)
            early += len(trace) > 1 and trace[-2] > 0
    assert early > 50
    ps = torch.tensor([1.0, 0.5, 0.2])
    for fn in (lambda m: truncate_mel(m, ps), lambda m: stream_truncate_mel(m, ps)[0]):
        with pytest.raises(Exception):
            fn(torch.randn(80, 3))


# ---- postnet halo -------------------------------------------------------------------------------------------------------------------

def _postnet64(W, cfg, mel):
    """the postnet of oracle/taco_oracle.py (tacotron2_infer's last block: conv k5 + folded BatchNorm, tanh on all but the last, plus the
    input), on float64 tensors"""
    import torch.nn.functional as F
    import taco_oracle as T
    y, n = mel, cfg['postnet_n_convolution']
    for i in range(n):
        p = f'postnet.convolutions.{i}.'
        y = F.conv1d(y, W[p + '0.weight'], W[p + '0.bias'], padding=(cfg['postnet_kernel_size'] - 1) // 2)
        s, t = T._bn_fold(W, p + '1')
        y = y * s[None, :, None] + t[None, :, None]
        if i < n - 1:
            y = torch.tanh(y)
    return mel + y


def test_postnet_window_halo_is_sufficient_and_tight():
    """T = 37: a window computed from the raw frames [t0 - halo, t1 + halo) clipped to the mel, with halo = n_conv * (k - 1) / 2 = 10,
    equals the whole-mel postnet to 1e-12 at interior windows and at windows touching either edge; with 9 some frame is off by more
    than 1e-6 of the output's scale"""
    from ttsamd.config import TACOTRON2_CONFIG
    from ttsamd.synth import tacotron2_state_dict
    cfg = dict(TACOTRON2_CONFIG)
    sd = tacotron2_state_dict(cfg, seed=0, gate_bias=-2.0)
    W = {k: torch.as_tensor(np.asarray(v)).double() for k, v in sd.items() if k.startswith('postnet.')}
    halo = cfg['postnet_n_convolution'] * (cfg['postnet_kernel_size'] - 1) // 2
    assert halo == 10
    T = 37
    mel = torch.randn(2, cfg['n_mels'], T, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    whole = _postnet64(W, cfg, mel)
    scale = float(whole.abs().max())

    def window(t0, t1, h):
        a0, a1 = max(t0 - h, 0), min(t1 + h, T)
        return _postnet64(W, cfg, mel[:, :, a0:a1])[:, :, t0 - a0:t1 - a0]
    worst_tight = 0.0
    for t0, t1 in ((0, 5), (0, 12), (11, 17), (12, 13), (10, 27), (20, 37), (36, 37), (0, 37)):
        assert float((window(t0, t1, halo) - whole[:, :, t0:t1]).abs().max()) <= 1e-12 * max(scale, 1.0), (t0, t1)
        if t0 - (halo - 1) > 0 or t1 + (halo - 1) < T:
            worst_tight = max(worst_tight, float((window(t0, t1, halo - 1) - whole[:, :, t0:t1]).abs().max()))
    assert worst_tight > 1e-6 * scale, worst_tight
