"""Drop-in for the reference's models/fastpitch/fastpitch/attn_loss_function.py: `AttentionCTCLoss` and `AttentionBinarizationLoss` with
the reference's names and signatures, FORWARD ONLY, computed in float64 on the device (ttsamd_attn_ctc_loss / ttsamd_attn_bin_loss,
csrc/attn_loss.hip).  They are the evaluation side: scores that say whether a forced alignment can be trusted.  The returned tensors carry
no grad history, and an input that requires grad is refused: the backward is not built.  No CPU fallback."""
import torch

from ttsamd import engine as _engine


class AttentionCTCLoss(torch.nn.Module):
    """forward(attn_logprob [B, 1, T, L], in_lens [B], out_lens [B]) -> scalar float64 on the device: the mean over rows of (forward-sum
    negative log-likelihood, or 0 where it is infinite) / max(in_len, 1) -- nn.CTCLoss(zero_infinity=True) with its default mean reduction
    over the blank-padded, key-masked, log-softmaxed attention, as the reference builds it.  No grad history: forward only."""

    def __init__(self, blank_logprob=-1):
        super().__init__()
        self.blank_logprob = blank_logprob

    @torch.no_grad()
    def forward(self, attn_logprob, in_lens, out_lens):
        nll = _engine.forward_sum_loss(attn_logprob, in_lens, out_lens, self.blank_logprob)
        n = torch.as_tensor(in_lens).to(device=nll.device, dtype=torch.float64).clamp(min=1.0, max=float(attn_logprob.shape[-1]))
        return (torch.where(torch.isinf(nll), torch.zeros_like(nll), nll) / n).mean()


class AttentionBinarizationLoss(torch.nn.Module):
    """forward(hard_attention, soft_attention [B, 1, T, L], eps=1e-12) -> scalar float64 on the device: -sum of log(max(soft, eps)) over
    the cells with hard == 1, divided by their number.  No grad history: forward only."""

    def __init__(self):
        super().__init__()

    @torch.no_grad()
    def forward(self, hard_attention, soft_attention, eps=1e-12):
        sum_log, count = _engine.binarization_loss(hard_attention, soft_attention, eps)
        return -sum_log.sum() / count.sum()
