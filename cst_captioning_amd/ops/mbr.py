"""Peer CIDEr-D: every caption of a pool scored against the other captions of
the same pool -- the scorer of consensus (minimum-Bayes-risk) decoding,
``--decode mbr``.

Training measures how well a caption agrees with a set of captions of the same
video (the CST reward, the GT consensus baseline).  At test time the set is the
model's own: the standard decode plus multinomial samples
(:meth:`..models.caption_model.CaptionModel.sample_mbr`).  The caption returned
is the one that agrees most with the others under CIDEr-D.

The references of a row are the other rows of its pool, so there is no reference
table and no dataset: only the document-frequency table is needed, and decoding a
test split never reads that split's labels.

  * ``backend='gpu'``: ``csrc/kernels/cider_pairwise.hip``, one workgroup per
    pool, the pool's n-gram vectors in LDS (``cider_score(..., group=G)``).
    Pools within ``G <= 64``, ``T <= 63`` and ``G * (T + 1) <= 2048``;
  * ``backend='cpu'``: the native fp64 twin (``cider_score_cpu(..., group=G)``),
    any ``G >= 2``;
  * ``backend='cpu-ref'``: the Python oracle on index strings, one
    ``CiderD.score_one`` per row.

``out[i]`` = 10 x the mean over the ``G - 1`` other rows ``j`` of ``i``'s pool of
the CIDEr-D similarity with ``i`` as the hypothesis and ``j`` as the reference.
Identical rows of a pool are ordinary peers: a caption drawn three times gets
three votes.
"""
import math

import numpy as np
import torch

from .. import _ext
from ..prepro.ciderdf import unpack_ngram_keys
from ..reward.cider_d_cpu import CiderD
from ..utils.text import array_to_str


def df_hash_table(keys, vals):
    """The open-addressing df hash table of ``csrc/cider_common.h`` as CPU
    tensors ``{'ht_keys', 'ht_vals'}`` (built by the native table builder on an
    empty label table)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    none = torch.zeros(0, dtype=torch.long)
    t = _ext.ops().cider_build_tables(torch.zeros(0, 1, dtype=torch.long), none, none,
                                      torch.from_numpy(keys.view(np.int64)),
                                      torch.from_numpy(vals), 0.0, 0)
    return {'ht_keys': t['ht_keys'], 'ht_vals': t['ht_vals']}


class PeerCiderD:
    """``df``: the ``(keys, vals, ref_len)`` triple of ``dataset.df`` /
    ``load_packed_df``."""

    def __init__(self, df, use_eos=0, device='cpu', backend='auto'):
        if df is None:
            raise ValueError('peer CIDEr-D needs a CIDEr-D document-frequency table')
        keys, vals, ref_len = df
        self.keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self.vals = np.ascontiguousarray(vals, dtype=np.float32)
        self.ref_len = ref_len
        self.log_ref_len = math.log(float(ref_len))
        self.use_eos = int(use_eos)
        self.device = torch.device(device)
        if backend == 'auto':
            backend = 'gpu' if (self.device.type == 'cuda' and _ext.available()) else 'cpu-ref'
            if backend == 'cpu-ref' and _ext.host_available():
                backend = 'cpu'
        if backend not in ('gpu', 'cpu', 'cpu-ref'):
            raise ValueError('unknown backend %r' % (backend,))
        if backend == 'gpu' and self.device.type != 'cuda':
            raise ValueError("backend 'gpu' needs a cuda device, got %s" % (self.device,))
        self.backend = backend
        self._tables = None
        self._oracle = None
        if backend in ('gpu', 'cpu'):
            t = df_hash_table(self.keys, self.vals)
            if backend == 'gpu':
                t = {k: v.to(self.device) for k, v in t.items()}
            self._tables = t

    def _oracle_scorer(self):
        if self._oracle is None:
            df = dict(zip(unpack_ngram_keys(self.keys), self.vals.astype(np.float64).tolist()))
            self._oracle = CiderD({'document_frequency': df, 'ref_len': self.ref_len})
        return self._oracle

    @staticmethod
    def _check(hyps, group):
        group = int(group)
        if hyps.dim() != 2:
            raise ValueError('hyps: (N, T) token ids')
        if group < 2:
            raise ValueError('a peer pool has at least 2 rows, got group = %d' % group)
        if hyps.size(0) % group:
            raise ValueError('%d rows are not whole pools of %d' % (hyps.size(0), group))
        return group

    def score_reference(self, hyps, group):
        """fp64 oracle (pure Python): ``(N,)`` float64 numpy."""
        group = self._check(hyps, group)
        oracle = self._oracle_scorer()
        h = hyps.detach().cpu().numpy()
        strs = [array_to_str(r, self.use_eos) for r in h]
        out = np.zeros(len(strs), dtype=np.float64)
        for p0 in range(0, len(strs), group):
            pool = strs[p0:p0 + group]
            for i in range(group):
                out[p0 + i] = oracle.score_one(pool[i], pool[:i] + pool[i + 1:])
        return out

    def score(self, hyps, group):
        """hyps: (N, T) long tensor, ``N = B * group``, rows ``[k * group,
        (k + 1) * group)`` the pool of video ``k``.  Returns (N,) float32 peer
        scores on ``hyps.device``.  The GPU backend launches one kernel and does
        not synchronise."""
        group = self._check(hyps, group)
        if self.backend == 'gpu':
            h = hyps.contiguous()
            return _ext.ops().cider_score(h, h.new_zeros(0), self._tables, self.log_ref_len,
                                          self.use_eos, group=group)
        if self.backend == 'cpu':
            h = hyps.detach().cpu().contiguous()
            s = _ext.ops().cider_score_cpu(h, h.new_zeros(0), self._tables, self.log_ref_len,
                                           self.use_eos, group=group)
            return s.to(hyps.device)
        s = self.score_reference(hyps, group)
        return torch.from_numpy(s.astype(np.float32)).to(hyps.device)

    def select(self, hyps, group):
        """``(best (B,), scores (B, G))``: ``best[k]`` is the lowest pool index
        among the rows that equal the pool's maximum score (index 0, the
        standard decode, wins ties).  Stays on ``hyps.device``, no host
        synchronisation."""
        scores = self.score(hyps, group).view(-1, int(group))
        return select_best(scores), scores


def select_best(scores):
    """(B, G) scores -> (B,) int64: the lowest index among each row's maxima
    (written out: the tie order of ``argmax`` is not specified)."""
    G = scores.size(1)
    idx = torch.arange(G, device=scores.device).expand_as(scores)
    top = scores.max(dim=1, keepdim=True).values
    return torch.where(scores == top, idx, torch.full_like(idx, G)).min(dim=1).values
