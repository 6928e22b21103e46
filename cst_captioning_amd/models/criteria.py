"""Loss criteria.

  * CrossEntropyCriterion -- ``/root/reference/model.py:26-43``: masked NLL,
    target/mask truncated to the prediction length.
  * RewardCriterion       -- ``model.py:7-23``: REINFORCE
    ``-sum(logp * reward * mask) / sum(mask)`` with mask = ``seq > 0``
    shifted right by one and a leading 1 (the first EOS is rewarded).

  * GroupCriterion        -- ``--rl_objective``: the sequence-level structured
    losses over each video's rollout rows (expected risk, Shen et al. 2016;
    softmax-margin and multi-margin, Edunov et al. 2018).  Not in the
    reference.

All also accept *gathered* log-probs (what the fused HIP engine returns:
``logp[r, t]`` of the token of interest), so no ``(R, T, V)`` tensor is
needed.
"""
import math

import torch
import torch.nn as nn

GROUP_OBJECTIVES = ('risk', 'softmax_margin', 'multi_margin')


def reward_mask(seq):
    m = (seq > 0).float()
    return torch.cat([m.new_ones(m.size(0), 1), m[:, :-1]], 1)


def check_label_smoothing(eps):
    """Validated ``--label_smoothing``: a finite float in [0, 1)."""
    eps = float(eps)
    if not 0.0 <= eps < 1.0:  # (NaN fails the comparison too)
        raise ValueError('label_smoothing must be in [0, 1), got %r' % eps)
    return eps


class CrossEntropyCriterion(nn.Module):
    """``label_smoothing`` eps (``--label_smoothing``, the definition of
    ``F.cross_entropy(..., label_smoothing=eps)``): the per-token log-prob
    becomes ``(1 - eps) lp[y] + eps mean_v lp[v]``.  Applied to dense
    ``(N, T, V)`` log-probs only: gathered ``(N, T)`` input is what the fused
    engine returns, already smoothed (``DecoderEngine.teacher_forced``)."""

    def __init__(self, label_smoothing=0.0):
        super().__init__()
        self.label_smoothing = check_label_smoothing(label_smoothing)

    def forward(self, pred, target, mask):
        """pred: (N, T, V) log-probs, or (N, T) log-probs already gathered at
        ``target``."""
        T = pred.size(1)
        target = target[:, :T]
        mask = mask[:, :T].float()
        lp = pred if pred.dim() == 2 else pred.gather(2, target.unsqueeze(2)).squeeze(2)
        eps = self.label_smoothing
        if eps > 0.0 and pred.dim() == 3:
            lp = (1.0 - eps) * lp + eps * pred.mean(2)
        return -(lp * mask).sum() / mask.sum()


class RewardCriterion(nn.Module):
    def forward(self, seq, logprobs, reward):
        """seq, logprobs: (N, T).  reward: (N, T) as in the reference or (N,)
        (constant over time)."""
        mask = reward_mask(seq)
        if reward.dim() == 1:
            reward = reward[:, None]
        return -(logprobs * reward * mask).sum() / mask.sum()


def check_group_objective(objective, alpha, cost_scale):
    """Validated (objective, alpha, cost_scale) of a group objective
    (``--rl_objective`` / ``--rl_alpha`` / ``--rl_cost_scale``)."""
    if objective not in GROUP_OBJECTIVES:
        raise ValueError('--rl_objective must be one of %s (or reinforce), got %r'
                         % (', '.join(GROUP_OBJECTIVES), objective))
    alpha, cost_scale = float(alpha), float(cost_scale)
    if not (math.isfinite(alpha) and alpha > 0):
        raise ValueError('--rl_alpha must be finite and > 0, got %r' % alpha)
    if not (math.isfinite(cost_scale) and cost_scale >= 0):
        raise ValueError('--rl_cost_scale must be finite and >= 0, got %r' % cost_scale)
    return objective, alpha, cost_scale


class GroupCriterion(nn.Module):
    """Structured loss over each video's S rollout rows (rows v*S .. v*S+S-1
    of ``seq`` / ``logprobs`` belong to video v).  With the reward mask m,
    n_i = sum_t m[i,t], the length-normalised sequence score
    s_i = alpha * sum_t(m lp)[i] / n_i, the row scores r_i, r* = max_j r_j
    attained first at i*, and the costs c_i = cost_scale * (r* - r_i), the
    per-video loss L_v is

      * risk:            sum_i softmax(s)_i c_i
      * softmax_margin:  -s_{i*} + logsumexp_j(s_j + c_j)
      * multi_margin:    (1/S) sum_j max(0, c_j - s_{i*} + s_j)

    and the loss their mean over the videos.  Returns (loss, reward, m, b) in
    the shape of the fused ``cst_loss``: m the mean score, b the mean over the
    videos of the logged baseline b_v (risk: the expected score
    sum_i softmax(s)_i r_i; margins: r*), reward (R,) = r_i - b_v, logged
    only.  Differentiable in ``logprobs`` by autograd; computes in the dtype
    of ``logprobs``."""

    def __init__(self, objective, alpha=1.0, cost_scale=1.0):
        super().__init__()
        self.objective, self.alpha, self.cost_scale = check_group_objective(objective, alpha,
                                                                            cost_scale)

    def forward(self, seq, logprobs, scores):
        if scores.dim() != 2 or scores.size(1) < 2 or scores.numel() != seq.size(0):
            raise ValueError('GroupCriterion: scores (B, S) with S >= 2 and B * S rows')
        S = scores.size(1)
        mask = reward_mask(seq).to(logprobs.dtype)
        s = (self.alpha * (logprobs * mask).sum(1) / mask.sum(1)).view(-1, S)
        r = scores.detach().to(logprobs.dtype)
        rmax = r.max(1, keepdim=True)[0]
        istar = r.argmax(1, keepdim=True)  # (the first index attaining the maximum)
        c = self.cost_scale * (rmax - r)
        if self.objective == 'risk':
            q = torch.softmax(s, 1)
            lv = (q * c).sum(1)
            bv = (q.detach() * r).sum(1, keepdim=True)
        elif self.objective == 'softmax_margin':
            lv = torch.logsumexp(s + c, 1) - s.gather(1, istar).squeeze(1)
            bv = rmax
        else:
            lv = torch.relu(c - s.gather(1, istar) + s).sum(1) / S
            bv = rmax
        return lv.mean(), (r - bv).reshape(-1), r.mean(), bv.mean()
