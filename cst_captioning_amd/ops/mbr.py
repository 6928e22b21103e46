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

:class:`PeerMix` (``--mbr_mix``) scores the same pools under a weighted sum of
peer CIDEr-D, sentence BLEU-4 and ROUGE-L, so a model trained with
``--reward_mix`` is decoded under the utility it was trained on
(``csrc/kernels/peer_mix.hip``, one launch).
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


class PeerMix:
    """Peer scores under a mixed utility (``--mbr_mix``): ``w_c * CIDErD + w_b *
    BLEU4 + w_r * ROUGE_L`` of every row against the other rows of its pool.

    ``parts[i] = (peer CIDEr-D as PeerCiderD, sentence BLEU-4, ROUGE-L of
    eval/metrics.py with the G - 1 other rows as references)``; a metric of
    weight 0 is not computed and its column is exactly 0.  ``df`` is the
    ``(keys, vals, ref_len)`` triple of :class:`PeerCiderD`; it is read only when
    ``w_c > 0`` and may be None otherwise.  ``vocab_size``: the model's, when
    known.  The interface is :class:`PeerCiderD`'s (``score`` is the
    blend), so ``CaptionModel.sample_mbr`` takes either.

      * ``backend='gpu'``: ``csrc/kernels/peer_mix.hip``, one launch
        (``metric_score('mix', ..., group=G)``), the limits of the CIDEr-D kernel;
      * ``backend='cpu'``: the native twin (``metric_score_cpu('mix', ...,
        group=G)``), any ``G >= 2``;
      * ``backend='cpu-ref'``: ``CiderD.score_one`` and the ``Bleu`` / ``Rouge``
        classes on index strings.

    The native backends pack n-grams at 16 bits per token: a vocabulary with ids
    over 65,534 is refused here.
    """

    def __init__(self, df, weights, use_eos=0, device='cpu', backend='auto', vocab_size=None):
        from .reward_mix import MAX_TOKEN
        weights = tuple(float(x) for x in weights)
        if len(weights) != 3:
            raise ValueError('weights: (CIDEr, Bleu_4, ROUGE_L), got %r' % (weights,))
        if any(not math.isfinite(x) or x < 0 for x in weights) or not any(weights):
            raise ValueError('weights must be finite, non-negative and not all zero, got %r'
                             % (weights,))
        if weights[0] and df is None:
            raise ValueError('peer CIDEr-D has weight %g and needs a CIDEr-D document-frequency '
                             'table' % weights[0])
        if not weights[0]:
            df = None  # (never read)
        self.weights = weights
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
        if backend != 'cpu-ref' and vocab_size is not None and vocab_size - 1 > MAX_TOKEN:
            raise ValueError('vocabulary of %d entries: token ids over 65,534 do not fit the '
                             'packed n-gram keys' % vocab_size)
        self.backend = backend
        # CIDEr-D: the oracle and the df hash table are PeerCiderD's
        self.cider = None if df is None else PeerCiderD(df, use_eos, device, backend)
        self.log_ref_len = 0.0 if self.cider is None else self.cider.log_ref_len
        self._tables = None if self.cider is None else self.cider._tables

    _check = staticmethod(PeerCiderD._check)

    def parts_reference(self, hyps, group):
        """(N, 3) fp64 scores of the Python oracles (0 where the weight is 0)."""
        from ..eval.metrics import Bleu, Rouge
        group = self._check(hyps, group)
        w_c, w_b, w_r = self.weights
        h = hyps.detach().cpu().numpy()
        parts = np.zeros((len(h), 3), dtype=np.float64)
        if w_c:
            parts[:, 0] = self.cider.score_reference(hyps, group)
        if w_b or w_r:
            strs = [array_to_str(r, self.use_eos) for r in h]
            res = {i: [s] for i, s in enumerate(strs)}
            gts = {}
            for p0 in range(0, len(strs), group):
                pool = strs[p0:p0 + group]
                for i in range(group):
                    gts[p0 + i] = pool[:i] + pool[i + 1:]
            if w_b and len(strs):
                parts[:, 1] = np.asarray(Bleu(4).compute_score(gts, res)[1][-1])
            if w_r and len(strs):
                parts[:, 2] = np.asarray(Rouge().compute_score(gts, res)[1])
        return parts

    def score_reference(self, hyps, group):
        """fp64 blend of the Python oracles: ``(N,)`` float64 numpy."""
        return self.parts_reference(hyps, group) @ np.asarray(self.weights, dtype=np.float64)

    def score_both(self, hyps, group):
        """``(out (N,), parts (N, 3))`` float32 on ``hyps.device``.  The GPU
        backend launches one kernel and does not synchronise."""
        group = self._check(hyps, group)
        if self.backend == 'gpu':
            h = hyps.contiguous()
            out, parts = _ext.ops().metric_score(
                'mix', h, h.new_zeros(0), None, self.use_eos, cider_tables=self._tables,
                log_ref_len=self.log_ref_len, weights=list(self.weights), group=group)
            return out, parts
        if self.backend == 'cpu':
            h = hyps.detach().cpu().contiguous()
            out, parts = _ext.ops().metric_score_cpu(
                'mix', h, h.new_zeros(0), None, self.use_eos, cider_tables=self._tables,
                log_ref_len=self.log_ref_len, weights=list(self.weights), group=group)
            return out.to(hyps.device), parts.to(hyps.device)
        parts = self.parts_reference(hyps, group).astype(np.float32)
        w = np.asarray(self.weights, dtype=np.float32)
        out = (w[0] * parts[:, 0] + w[1] * parts[:, 1]) + w[2] * parts[:, 2]  # (fp32, as the kernel)
        return (torch.from_numpy(out.astype(np.float32)).to(hyps.device),
                torch.from_numpy(parts).to(hyps.device))

    def score_parts(self, hyps, group):
        """(N, 3) float32: peer CIDEr-D, BLEU-4, ROUGE-L of every row."""
        return self.score_both(hyps, group)[1]

    def score(self, hyps, group):
        """(N,) float32 blended peer scores on ``hyps.device``."""
        return self.score_both(hyps, group)[0]

    def select(self, hyps, group):
        """``(best (B,), scores (B, G))`` under the blend, the tie rule of
        :func:`select_best`; stays on ``hyps.device``."""
        scores = self.score(hyps, group).view(-1, int(group))
        return select_best(scores), scores


def select_best(scores):
    """(B, G) scores -> (B,) int64: the lowest index among each row's maxima
    (written out: the tie order of ``argmax`` is not specified)."""
    G = scores.size(1)
    idx = torch.arange(G, device=scores.device).expand_as(scores)
    top = scores.max(dim=1, keepdim=True).values
    return torch.where(scores == top, idx, torch.full_like(idx, G)).min(dim=1).values
