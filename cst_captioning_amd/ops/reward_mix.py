"""Mixed-metric RL reward (``--reward_mix CIDEr:1,Bleu_4:5,ROUGE_L:5``): the
reward of a caption is ``w_c * CIDErD + w_b * BLEU4 + w_r * ROUGE_L``.

Each term is exactly what the single-metric reward scorers return
(:class:`.cider_d.CiderDScorer`: CIDEr-D on its x10 scale with the dataset's
df table; :class:`.sent_metrics.SentenceMetricScorer`: ``eval/metrics.py``
sentence scores), with one ``use_eos`` for all three.  Weights are
non-negative, so the sum has no cancellation.  METEOR is scored on the host
and cannot be mixed.

:class:`MixedRewardScorer` has the surface of those scorers (``backend``,
``score``, ``score_reference``), so the trainer's RL loss uses it unchanged:

  * ``backend='gpu'``: ``csrc/kernels/reward_mix.hip`` scores a hypothesis
    under the metrics in use and blends them in ONE launch (capturable), on the
    tables the component scorers' builders make, built once;
  * ``backend='cpu'`` / ``'cpu-ref'``: the component scorers' ``score`` (native
    C++ twins / Python scorers), blended on the host.

A metric of weight 0 is never built or scored: a dataset without a df table is
fine when ``w_c = 0``.  Limits are the intersection of the components' in use:
hypotheses of at most 64 tokens (63 with CIDEr-D in the mix), token ids up to
65,534 (checked where the host sees them: the dataset's vocabulary and
references when the scorer is built, the hypotheses of the host backends when
they are scored; the kernel cannot raise, and as ``bleu4_kernel`` treats a
larger hypothesis token as one that matches nothing).
"""
import copy
import math

import numpy as np
import torch

from .. import _ext

METRICS = ('CIDEr', 'Bleu_4', 'ROUGE_L')
MAX_TOKEN = 65534


def parse_reward_mix(spec, flag='--reward_mix'):
    """``'CIDEr:1,Bleu_4:5'`` -> ``(w_c, w_b, w_r)`` floats in the order of
    :data:`METRICS`; a metric left out has weight 0.  ``ValueError`` naming the
    problem for an unknown metric, METEOR, a metric given twice, a malformed,
    negative or non-finite weight, and all weights zero.  ``flag``: the
    command-line flag the messages name (``--mbr_mix`` takes the same grammar)."""
    def bad(msg):
        return ValueError('%s: %s' % (flag, msg))

    if not isinstance(spec, str) or not spec.strip():
        raise bad('empty specification')
    w = {}
    for item in spec.split(','):
        name, sep, val = item.strip().partition(':')
        name, val = name.strip(), val.strip()
        if not sep or not name or not val:
            raise bad('%r is not METRIC:WEIGHT' % (item.strip(),))
        if name == 'METEOR':
            raise bad('METEOR is scored on the host only and cannot be '
                      'mixed (use --eval_metric METEOR for a METEOR reward)')
        if name not in METRICS:
            raise bad('unknown metric %r (one of %s)' % (name, ', '.join(METRICS)))
        if name in w:
            raise bad('metric %s appears twice' % name)
        try:
            x = float(val)
        except ValueError:
            raise bad('weight %r of %s is not a number' % (val, name))
        if not math.isfinite(x):
            raise bad('weight %r of %s is not finite' % (val, name))
        if x < 0:
            raise bad('weight %r of %s is negative' % (val, name))
        w[name] = x
    weights = tuple(w.get(m, 0.0) for m in METRICS)
    if not any(weights):
        raise bad('all weights are zero')
    return weights


def opt_weights(opt):
    """The weights of ``opt.reward_mix``, or None when the flag is off."""
    spec = getattr(opt, 'reward_mix', '') or ''
    return parse_reward_mix(spec) if spec else None


def check_consensus_route(opt):
    """CST / WXE baselines under a mix come from ``--consensus_scorer tokens``
    (``ops/consensus.py`` blends the same metrics); the scores of a file are
    coco CIDEr on another scale, blending them would mis-weight the baseline."""
    if (opt_weights(opt) is not None and getattr(opt, 'use_cst', 0) == 1
            and getattr(opt, 'consensus_scorer', 'file') != 'tokens'
            and getattr(opt, 'train_bcmrscores_pkl', None)):
        raise ValueError('--reward_mix with --use_cst 1 cannot take its consensus scores from '
                         '--train_bcmrscores_pkl (one metric, coco CIDEr on another scale): use '
                         '--consensus_scorer tokens, which scores them in the mixed metric')


def blend(weights, parts):
    """fp64 weighted sum of (..., 3) scores."""
    return np.asarray(parts, dtype=np.float64) @ np.asarray(weights, dtype=np.float64)


def reward_mix_score(hyps, hyp_video, cider_tables, sent_tables, log_ref_len, use_eos, weights):
    """The GPU op: ``(out (N,), parts (N, 3))`` fp32 of ``reward_mix_kernel`` in
    one launch, capturable.  ``cider_tables`` / ``sent_tables`` are the device
    tables of ``cider_build_tables`` / ``metric_build_tables``, None for metrics
    of weight 0.  The extension's set of bound names is pinned
    (``tests/golden/ext_entry_points.txt``), so the op is the ``'mix'`` mode of
    the extension's ``metric_score``, as peer CIDEr-D is a mode of
    ``cider_score``.  Raises before the launch for a width over the limit."""
    out, parts = _ext.ops().metric_score('mix', hyps, hyp_video, sent_tables, use_eos,
                                         cider_tables=cider_tables, log_ref_len=log_ref_len,
                                         weights=list(weights))
    return out, parts


class MixedRewardScorer:
    def __init__(self, dataset, weights, use_eos=0, device='cpu', backend='auto'):
        weights = tuple(float(x) for x in weights)
        if len(weights) != 3:
            raise ValueError('weights: (CIDEr, Bleu_4, ROUGE_L), got %r' % (weights,))
        if any(not math.isfinite(x) or x < 0 for x in weights) or not any(weights):
            raise ValueError('weights must be finite, non-negative and not all zero, got %r'
                             % (weights,))
        self.ds = dataset
        self.weights = weights
        self.use_eos = int(use_eos)
        self.device = torch.device(device)
        if backend == 'auto':
            backend = 'gpu' if (self.device.type == 'cuda' and _ext.available()) else 'cpu-ref'
            if backend == 'cpu-ref' and _ext.host_available():
                backend = 'cpu'
        if backend not in ('gpu', 'cpu', 'cpu-ref'):
            raise ValueError('unknown backend %r' % (backend,))
        self.backend = backend
        w_c, w_b, w_r = weights
        nvocab = getattr(dataset, 'vocab_size', None)
        if backend != 'cpu-ref' and nvocab is not None and nvocab - 1 > MAX_TOKEN:
            raise ValueError('vocabulary of %d entries: token ids over 65,534 do not fit the '
                             'packed n-gram keys' % nvocab)
        # the component scorers own the tables (their builders, once); one
        # SentenceMetricScorer table set serves BLEU and ROUGE
        from .cider_d import CiderDScorer
        from .sent_metrics import SentenceMetricScorer
        self.cider = CiderDScorer(dataset, use_eos, device, backend) if w_c else None
        self.sent = None
        self._rouge = None
        if w_b or w_r:
            self.sent = SentenceMetricScorer(dataset, 'Bleu_4' if w_b else 'ROUGE_L', use_eos,
                                             device, backend)
            if w_b and w_r:  # (the other metric on the same tables; host backends only)
                self._rouge = copy.copy(self.sent)
                self._rouge.metric, self._rouge._oracle = 'ROUGE_L', None
        self.max_width = 63 if w_c else 64

    # -- components ----------------------------------------------------------------
    def _components(self):
        """(column, scorer) of the metrics in use."""
        w_c, w_b, w_r = self.weights
        out = []
        if w_c:
            out.append((0, self.cider))
        if w_b:
            out.append((1, self.sent))
        if w_r:
            out.append((2, self._rouge if w_b else self.sent))
        return out

    def _check(self, hyps, on_host):
        if hyps.dim() != 2:
            raise ValueError('hyps: (N, T), got %s' % (tuple(hyps.shape),))
        if hyps.shape[1] > self.max_width:
            raise ValueError('hypotheses of %d tokens; at most %d are supported%s'
                             % (hyps.shape[1], self.max_width,
                                ' with CIDEr-D in the mix' if self.weights[0] else ''))
        if on_host and hyps.numel() and int(hyps.max()) > MAX_TOKEN:
            raise ValueError('hypothesis token %d: ids over 65,534 do not fit the packed n-gram '
                             'keys' % int(hyps.max()))

    # -- scoring -------------------------------------------------------------------
    def score_both(self, hyps, video_index):
        """``(out (N,), parts (N, 3))`` of one launch (``backend='gpu'``)."""
        self._check(hyps, on_host=not hyps.is_cuda)
        return reward_mix_score(
            hyps.contiguous(), video_index.contiguous(),
            None if self.cider is None else self.cider._tables,
            None if self.sent is None else self.sent._tables,
            0.0 if self.cider is None else self.cider.log_ref_len, self.use_eos,
            list(self.weights))

    def score_parts(self, hyps, video_index):
        """(N, 3) float32 on ``hyps.device``: CIDEr-D, BLEU-4, ROUGE-L of every
        hypothesis; the column of a zero-weight metric is exactly 0."""
        if self.backend == 'gpu':
            return self.score_both(hyps, video_index)[1]
        if self.backend == 'cpu':
            self._check(hyps.detach().cpu(), on_host=True)
        parts = torch.zeros(hyps.shape[0], 3, dtype=torch.float32, device=hyps.device)
        for col, sc in self._components():
            parts[:, col] = sc.score(hyps, video_index).float()
        return parts

    def score(self, hyps, video_index):
        """hyps: (N, T) long tensor; video_index: (N,) dataset video indices.
        Returns (N,) float32 rewards on ``hyps.device``."""
        if self.backend == 'gpu':
            return self.score_both(hyps, video_index)[0]
        parts = self.score_parts(hyps, video_index).cpu().numpy()
        w = np.asarray(self.weights, dtype=np.float32)
        out = (w[0] * parts[:, 0] + w[1] * parts[:, 1]) + w[2] * parts[:, 2]  # (fp32, as the kernel)
        return torch.from_numpy(out.astype(np.float32)).to(hyps.device)

    def parts_reference(self, hyps, video_index):
        """(N, 3) fp64 scores of the Python oracles (0 where the weight is 0)."""
        parts = np.zeros((hyps.shape[0], 3), dtype=np.float64)
        for col, sc in self._components():
            parts[:, col] = sc.score_reference(hyps, video_index)
        return parts

    def score_reference(self, hyps, video_index):
        """fp64 blend of the Python oracles, for tests."""
        return blend(self.weights, self.parts_reference(hyps, video_index))
