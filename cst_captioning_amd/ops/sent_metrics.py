"""Sentence-level BLEU-4 / ROUGE-L reward scorer: on-GPU HIP kernels, or CPU
scorers (``--eval_metric Bleu_4 | ROUGE_L`` with ``use_rl=1``).

The reference scores these rewards like CIDEr-D, on the host from Python
strings (``train.py:119-124`` -> ``utils.py:169-226``).  Here, as for CIDEr-D
(:mod:`.cider_d`):

  * per video, the union of the references' packed n-grams with their clip
    counts, the reference lengths (BLEU) and the reduced reference token rows
    (ROUGE) are built ONCE per dataset by the native host builder
    (``csrc/host/metric_host.cpp``) and uploaded;
  * ``csrc/kernels/sent_metrics.hip`` scores one hypothesis per wavefront in
    one launch, so the RL step stays capturable as one graph.

The scores follow :mod:`..eval.metrics` (``Bleu(4)`` per-sentence scores,
``Rouge.calc_score``), which is also the fp64 oracle of
:meth:`SentenceMetricScorer.score_reference`.  ``backend='cpu'`` is the native
C++ scorer on the same tables; ``backend='cpu-ref'`` reproduces the reference
cost model (strings + Python scorer).

Limits of the table-based backends (checked, with an error): hypotheses and
reduced references of at most 64 tokens; token ids up to 65,534 in the
references, and for BLEU in the CPU scorer's hypotheses (16 bits per token in
the packed n-gram keys; the kernel treats a larger hypothesis token as one that
matches nothing).
"""
import numpy as np
import torch

from .. import _ext
from ..reward.rewards import score_hypotheses

METRICS = ('Bleu_4', 'ROUGE_L')


class SentenceMetricScorer:
    def __init__(self, dataset, metric, use_eos=0, device='cpu', backend='auto'):
        if metric not in METRICS:
            raise ValueError('metric must be one of %s, got %r' % (METRICS, metric))
        self.ds = dataset
        self.metric = metric
        self.use_eos = int(use_eos)
        self.device = torch.device(device)
        if backend == 'auto':
            backend = 'gpu' if (self.device.type == 'cuda' and _ext.available()) else 'cpu-ref'
            if backend == 'cpu-ref' and _ext.host_available():
                backend = 'cpu'
        if backend not in ('gpu', 'cpu', 'cpu-ref'):
            raise ValueError('unknown backend %r' % (backend,))
        self.backend = backend
        self._tables = None
        self._oracle = None
        if backend in ('gpu', 'cpu'):
            self._build_tables()

    def _build_tables(self):
        lab = np.ascontiguousarray(self.ds.labels, dtype=np.int64)
        st = np.ascontiguousarray(self.ds.label_start_ix, dtype=np.int64)
        en = np.ascontiguousarray(self.ds.label_end_ix, dtype=np.int64)
        t = _ext.ops().metric_build_tables(torch.from_numpy(lab), torch.from_numpy(st),
                                           torch.from_numpy(en), self.use_eos)
        if self.backend == 'gpu':
            t = {k: v.to(self.device) for k, v in t.items()}
        self._tables = t

    def _oracle_scorer(self):
        if self._oracle is None:
            from ..eval.metrics import Bleu, Rouge
            self._oracle = Bleu(4) if self.metric == 'Bleu_4' else Rouge()
        return self._oracle

    def score(self, hyps, video_index):
        """hyps: (N, T <= 64) long tensor; video_index: (N,) dataset video
        indices.  Returns (N,) float32 scores on ``hyps.device``."""
        if self.backend == 'gpu':
            return _ext.ops().metric_score(self.metric, hyps.contiguous(),
                                           video_index.contiguous(), self._tables, self.use_eos)
        if self.backend == 'cpu':
            s = _ext.ops().metric_score_cpu(self.metric, hyps.detach().cpu().contiguous(),
                                            video_index.detach().cpu().contiguous(),
                                            self._tables, self.use_eos)
            return s.to(hyps.device)
        s = self.score_reference(hyps, video_index)
        return torch.from_numpy(s.astype(np.float32)).to(hyps.device)

    def score_reference(self, hyps, video_index):
        """fp64 oracle (pure Python, :mod:`..eval.metrics`)."""
        h = hyps.detach().cpu().numpy()
        v = video_index.detach().cpu().numpy()
        gts = [self.ds.gts_of(int(x)) for x in v]
        return score_hypotheses(self._oracle_scorer(), h, gts, seq_per_img=1, expand_feat=1,
                                use_eos=self.use_eos)
