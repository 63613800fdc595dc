"""TEST INFRASTRUCTURE ONLY: CPU restatement of the reference's causal normalisations
(brever/modules/normalization.py:5-46 CausalGroupNorm; :54-72 the LayerNorm / InstanceNorm
shorthands, groups = 1 / groups = channels). Pinned by tests/golden/norms.npz (generated from
the imported reference by tests/golden/make_golden.py). Nothing on the product path imports
this file. `cumulative_norm` is the FFNN's CumulativeNormalizer
(brever/models/ffnn/ffnn.py:190-203) for float64 use, pinned by `cumnorm_out` of tests/golden/ffnn.npz.

Restated as running moments: with the input viewed as (batch, group, rest, frame), frame t is
normalised by the mean and the biased variance of everything its group holds in frames 0..t
(normalization.py:34-41), then scaled per channel (normalization.py:45-46)."""
import torch


def causal_group_norm(x, gain, bias, groups, time_dim=-1, eps=1e-10):
    """x (B, C, ...) -> same shape; differentiable (torch autograd) so the test can pin the
    gradients as well. `time_dim` may not be 0 or 1 (normalization.py:48-52)."""
    t_ax = range(x.ndim)[time_dim]
    if t_ax in (0, 1):
        raise ValueError('time_dim cannot be the batch or the channel dimension')
    B, C = x.shape[:2]
    if C % groups:
        raise ValueError('num_channels must be divisible by num_groups')
    z = x.movedim(t_ax, -1)                                   # frames last
    moved = z.shape
    T = moved[-1]
    z = z.reshape(B, groups, -1, T)                           # (B, G, rest, T)
    seen = z.shape[2]*torch.arange(1, T + 1, dtype=x.dtype)   # elements seen up to each frame
    m1 = z.sum(2).cumsum(-1)/seen                             # running mean (B, G, T)
    m2 = (z*z).sum(2).cumsum(-1)/seen                         # running mean of squares
    spread = (m2 - m1*m1 + eps).sqrt()
    z = (z - m1[:, :, None])/spread[:, :, None]
    z = z.reshape(moved).movedim(-1, t_ax)
    per_channel = [1, C] + [1]*(x.ndim - 2)
    return z*gain.view(per_channel) + bias.view(per_channel)


def cumulative_norm(x, eps=1e-4, parts=False):
    """The FFNN's CumulativeNormalizer (brever/models/ffnn/ffnn.py:190-203) in the dtype of `x`:
    every row of (..., T) is normalised at frame t by its own mean and biased variance over
    frames 0..t. Meant to be called on `.double()` inputs as the yardstick of the fp32 kernel.
    The variance is clamped at 0, which it cannot go below in exact arithmetic; the reference
    does not clamp, and in fp32 returns NaN on constant rows. parts=True also returns the
    running mean and 1/sqrt(var + eps), from which the tests form their rounding bound."""
    count = torch.arange(1, x.shape[-1] + 1, dtype=x.dtype)
    mean = x.cumsum(-1)/count
    var = ((x*x).cumsum(-1)/count - mean*mean).clamp_min(0)
    spread = (var + eps).sqrt()
    y = (x - mean)/spread
    return (y, mean, 1/spread) if parts else y
