"""Shared builders of the truncated (top-k / nucleus) sampling tests
(``test_topk_sampling.py`` on the CPU, ``test_gpu_topk_sampling.py`` on the
GPU): an fp64 numpy oracle of the definition that shares no code with
``caption_model.truncated_probs``, logit vectors whose top-k set and
distribution are known exactly, and the membership check of sampled sequences
against teacher-forced log-probs.

Definition (one step, log-softmax ``lp`` at temperature 1): the ``k`` largest
entries, ties to the smaller index, ordered by value descending then index
ascending; ``w_i = exp((lp_i - lp_0) / tau)``, ``q = w / sum w``; ``m`` the
smallest prefix with ``q_0 + .. + q_{m-1} >= p`` (``m = k`` at ``p = 1``); the
draw is ``i < m`` with probability ``q_i / (q_0 + .. + q_{m-1})``."""
import collections

import numpy as np
import torch

VT = 128  # columns per vocabulary tile of the decode launch

Exact = collections.namedtuple('Exact', 'order q m probs margin')


def exact_truncated(x, k, p, tau):
    """fp64 oracle for one row of logits or log-probs ``x`` (the softmax
    normaliser cancels).  ``order``: the k candidates; ``q``: their
    probabilities before the nucleus cut; ``m``; ``probs`` (V) zero outside
    the kept set; ``margin``: distance of the cumulative mass from ``p`` on
    either side of the cut (inf at ``p = 1``, where ``m = k`` by definition)."""
    x = np.asarray(x, dtype=np.float64)
    order = np.lexsort((np.arange(len(x)), -x))[:k]
    v = x[order]
    w = np.exp((v - v[0]) / tau)
    q = w / w.sum()
    cum = np.cumsum(q)
    if p >= 1.0:
        m, margin = k, np.inf
    else:
        m = int(np.argmax(cum >= p)) + 1
        margin = cum[m - 1] - p
        if m > 1:
            margin = min(margin, p - cum[m - 2])
    probs = np.zeros(len(x))
    probs[order[:m]] = q[:m] / q[:m].sum()
    return Exact(order, q, m, probs, margin)


def bf16_exact(a):
    """Round to bf16 and back: values the bf16 weights hold exactly."""
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).bfloat16().float().numpy()


# the 10 best logits of a kernel case, best first (exact in bf16); the
# background stays at or below -3.  Their nucleus cuts at p = 0.9 / 0.5 lie at
# least 1e-3 from the cumulative mass for k in {2, 5, 8} and tau in {1, 0.7}
# (asserted by the tests that use them)
WINNERS = np.array([3.0, 2.5, 2.25, 1.75, 1.5, 1.0, 0.75, 0.5, 0.0, -0.5])
TIE_WINNERS = np.array([3.0, 2.5, 2.5, 1.75, 1.5, 1.5, 1.0, 0.75, 0.5, 0.0])
LAYOUTS = ('one_tile', 'per_tile', 'last_col', 'ties')


def kernel_logits(V, layout, seed=0):
    """(V) fp32 logits, exact in bf16, for the vocab_select construction
    (h = e_0, W[:, 0] = x, b = 0).  Layouts, by where the best values sit:
    one_tile  the 10 best in one 128-column tile (the second, or the first
              when V has fewer than two full tiles);
    per_tile  the best min(n_tiles, 10) in distinct tiles, the last tile
              (possibly narrower than k) among them;
    last_col  the best value in the last valid column V - 1;
    ties      two pairs of equal values (ranks 1, 2 and ranks 4, 5), one of each
              pair in the first tile and one in the last: the smaller index must
              win where a pair straddles rank k (k = 2 and k = 5)."""
    rs = np.random.RandomState(seed)
    x = bf16_exact(-3.0 - 3.0 * rs.rand(V))
    n_vt = (V + VT - 1) // VT
    win = WINNERS.copy()
    if layout == 'one_tile':
        t = 1 if V >= 2 * VT else 0
        cols = t * VT + rs.permutation(VT)[:10]
    elif layout == 'per_tile':
        tiles = [n_vt - 1] + list(range(n_vt - 1))  # the last tile first
        cols = []
        for j in range(10):
            t = tiles[j % n_vt]
            lo, hi = t * VT, min(V, (t + 1) * VT)
            free = [c for c in range(lo, hi) if c not in cols]
            if not free:  # (a 2-column last tile is full after two rounds)
                free = [c for c in range(0, VT) if c not in cols]
            cols.append(free[rs.randint(len(free))])
        cols = np.array(cols)
    elif layout == 'last_col':
        cols = np.concatenate([[V - 1], rs.permutation(V - 1)[:9]])
    elif layout == 'ties':
        # ranks 1, 2 and ranks 4, 5 hold equal values: of each pair one column in
        # the first tile and one in the last tile (V = 130: its two columns)
        lo = (n_vt - 1) * VT
        first = np.sort(rs.permutation(VT // 2)[:2])
        last = lo + np.sort(rs.permutation(V - lo)[:2])
        rest = [c for c in rs.permutation(V) if c not in first and c not in last][:6]
        # (the larger index of a pair is written first: the order must not matter)
        cols = np.array([rest[0], last[0], first[0], rest[1], last[1], first[1]] + rest[2:])
        win = TIE_WINNERS.copy()
    else:
        raise ValueError(layout)
    assert len(set(cols.tolist())) == 10 and cols.max() < V
    x[cols] = win
    assert np.array_equal(bf16_exact(x), x)
    return x.astype(np.float32)


def select_operands(x, R, H=64, device='cpu'):
    """(hd (R, H) bf16, W (V, H) bf16, b (V) fp32) whose logits are exactly x in
    every row."""
    V = len(x)
    W = torch.zeros(V, H)
    W[:, 0] = torch.from_numpy(np.asarray(x, dtype=np.float32))
    hd = torch.zeros(R, H)
    hd[:, 0] = 1.0
    return hd.bfloat16().to(device), W.bfloat16().to(device), torch.zeros(V, device=device)


def teacher_force(model, feats, seq, rows_per_video):
    """Dense log-probs (R, n, V) of the PyTorch path with the sampled tokens
    as inputs: column j is the distribution token seq[:, j] was drawn from."""
    prev, training = model.seq_per_img, model.training
    model.eval()
    model.set_seq_per_img(rows_per_video)
    try:
        lab = torch.cat([torch.full_like(seq[:, :1], model.bos_index), seq,
                         torch.zeros_like(seq[:, :1])], 1)
        with torch.no_grad():
            pred = model(feats, lab)[0]
    finally:
        model.set_seq_per_img(prev)
        model.train(training)
    return pred[:, :seq.size(1)]


def membership(pred, seq, top_k, top_p, tau, near=0.0):
    """Per (row, step) of the sampled tokens up to and including a row's first
    0: ``inside`` -- the token has mass under the truncated distribution of
    ``pred``; ``sure`` -- that verdict does not hinge on a boundary closer
    than ``near`` in ``pred``'s own terms: the gap between the last candidate
    and the first one left out, or between the cumulative mass on either side
    of the nucleus cut and ``top_p``; ``alive`` -- the pairs that count; ``lp``
    -- pred's log-prob of the token.  fp64 on the host."""
    pred = pred.detach().double().cpu()
    seq = seq.detach().cpu()
    n = pred.size(1)
    seq = seq[:, :n]
    R, V = pred.size(0), pred.size(2)
    alive = torch.ones(R, n, dtype=torch.bool)
    alive[:, 1:] = torch.cumprod((seq[:, :-1] > 0).long(), 1) > 0
    vals, idx = torch.sort(pred, dim=-1, descending=True, stable=True)
    kv = vals[..., :top_k]
    w = ((kv - kv[..., :1]) / tau).exp()
    q = w / w.sum(-1, keepdim=True)
    cum = q.cumsum(-1)
    before = cum - q
    keep = before < top_p if top_p < 1.0 else torch.ones_like(q, dtype=torch.bool)
    probs = torch.zeros_like(pred).scatter_(-1, idx[..., :top_k], q * keep)
    inside = probs.gather(2, seq.unsqueeze(2)).squeeze(2) > 0
    sure = torch.ones(R, n, dtype=torch.bool)
    if near > 0.0:
        if top_k < V:
            sure &= (vals[..., top_k - 1] - vals[..., top_k]) >= near
        if top_p < 1.0:
            sure &= ((cum - top_p).abs() >= near).all(-1)
    lp = pred.gather(2, seq.unsqueeze(2)).squeeze(2)
    return inside, sure, alive, lp
