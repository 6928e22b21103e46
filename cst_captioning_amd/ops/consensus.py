"""GT consensus scores ("bcmrscores") in token space: every ground-truth
caption scored against the other captions of its video, on the GPU or through
the native C++ twins (``--consensus_scorer tokens``,
``python -m cst_captioning_amd.prepro.evalscores --scorer tokens``).

The strings route (:func:`..prepro.evalscores.compute_consensus_scores`) scores
Python strings from the coco-format file with the Python scorers, one caption
slot at a time.  Here the captions stay the label rows the RL reward is scored
against, so the consensus baseline and the reward of a sampled caption are the
same function of the same tables:

  * slot ``i`` of video ``v`` is caption ``i % ncap`` of the video's label rows
    (as ``prepro/evalscores.py``); the hypothesis is that label row;
  * leave-one-out (``remove_in_ref``): the scoring kernels take a per-hypothesis
    ``exclude`` index, the caption's own position among the video's references,
    and skip that reference (``csrc/cider_common.h`` ``excluded_ref``; BLEU's
    clip counts come from ``ng_cnt2`` / ``ng_arg`` of the metric tables).  A
    video with one caption keeps it (``rest if rest else refs[v]``);
  * one launch per metric over all ``videos x seq_per_img`` hypotheses; the
    tables are built once per scorer.

Per metric:

  * ``Bleu_4``, ``ROUGE_L``: :class:`.sent_metrics.SentenceMetricScorer`'s scores
    (``eval/metrics.py`` ``Bleu(4)`` per sentence, ``Rouge.calc_score``), same
    ``use_eos``;
  * ``CIDEr``: :class:`.cider_d.CiderDScorer`'s score -- CIDEr-D (clipped,
    Gaussian length penalty) with the DATASET's document-frequency table
    (``dataset.df``), x10.  This is deliberately the score the reward kernel
    gives that caption, NOT coco CIDEr with a per-slot leave-one-out corpus df,
    which is what the strings route computes.  A dataset without a df table
    raises when ``CIDEr`` is asked for;
  * ``METEOR``: the validation kernel's exact + stem alignment
    (``meteor_stats``, segment score of the best reference), without EOS, token
    canonicalisation and stem ids as in :class:`.corpus_metrics.CorpusScorer`.

``backend='cpu-ref'`` runs the Python oracles (``eval/metrics.py`` ``Bleu`` /
``Rouge`` / ``Meteor``, ``reward/cider_d_cpu.py`` ``CiderD``) with the
caption's own row removed from the references.

Limits of the table-based backends are those of the kernels: label rows and
reduced references of at most 64 tokens (63 for CIDEr-D), token ids up to
65,534.
"""
import numpy as np
import torch

from .. import _ext

METRICS = ('Bleu_4', 'METEOR', 'ROUGE_L', 'CIDEr')


def consensus_metric(eval_metric):
    """The consensus metric of an ``--eval_metric`` (as ``build_scorer`` picks
    the reward: CIDEr / MSRVTT / Loss train on CIDEr-D)."""
    return 'CIDEr' if eval_metric in ('CIDEr', 'MSRVTT', 'Loss') else eval_metric


def consensus_slots(label_start_ix, label_end_ix, seq_per_img, remove_in_ref=True):
    """(label rows, video index, exclude) of the ``Nv * S`` consensus slots,
    video-major: slot ``i`` of video ``v`` is caption ``i % ncap``; ``exclude``
    is that caption's index in the video when ``remove_in_ref``, else -1."""
    st = np.asarray(label_start_ix, dtype=np.int64)
    ncap = np.asarray(label_end_ix, dtype=np.int64) - st
    j = np.arange(int(seq_per_img), dtype=np.int64)[None, :] % ncap[:, None]
    rows = (st[:, None] + j).reshape(-1)
    vid = np.repeat(np.arange(len(st), dtype=np.int64), int(seq_per_img))
    ex = j.reshape(-1).copy() if remove_in_ref else np.full(rows.shape, -1, dtype=np.int64)
    return rows, vid, ex


class ConsensusScorer:
    """``scores(seq_per_img)`` -> ``{metric: (Nv, S) float64}`` for the label
    table of ``dataset`` (see the module docstring)."""

    def __init__(self, dataset, use_eos=0, device='cpu', backend='auto'):
        if not dataset.has_label:
            raise ValueError('the consensus scorer needs a split with labels')
        self.ds = dataset
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
        self._dev = self.device if backend == 'gpu' else torch.device('cpu')
        self._tables = {}   # 'sent' | 'meteor' | 'cider' -> dict of tensors (+ extras)
        self._labels = {}   # 'raw' | 'canon' -> (M, L) int64 on the scoring device
        self._vocab = None  # (words, canon, stems)

    # -- tables (once per scorer) ------------------------------------------------
    def _vocab_ids(self):
        if self._vocab is None:
            from .corpus_metrics import vocab_ids
            self._vocab = vocab_ids(self.ds.vocab)
        return self._vocab

    def _ranges(self):
        st = np.ascontiguousarray(self.ds.label_start_ix, dtype=np.int64)
        en = np.ascontiguousarray(self.ds.label_end_ix, dtype=np.int64)
        return torch.from_numpy(st), torch.from_numpy(en)

    def _label_table(self, kind):
        """The hypotheses' source: the label table ('raw'), or its canonical
        token ids ('canon', METEOR), on the scoring device."""
        if kind not in self._labels:
            lab = np.ascontiguousarray(self.ds.labels, dtype=np.int64)
            if kind == 'canon':
                _, canon, _ = self._vocab_ids()
                if lab.size and (lab.min() < 0 or lab.max() >= len(canon)):
                    raise ValueError('label token outside the vocabulary of %d entries'
                                     % len(canon))
                lab = np.ascontiguousarray(canon[lab])
            self._labels[kind] = torch.from_numpy(lab).to(self._dev)
        return self._labels[kind]

    def _upload(self, t):
        return {k: v.to(self._dev) for k, v in t.items()}

    def build_tables(self, metrics=METRICS):
        """Reference tables of ``metrics`` (no-op for those already built and
        for ``backend='cpu-ref'``)."""
        if self.backend == 'cpu-ref':
            return
        ops = _ext.ops()
        for m in metrics:
            if m not in METRICS:
                raise ValueError('metric must be one of %s, got %r' % (METRICS, m))
            if m == 'CIDEr' and self.ds.df is None:
                raise ValueError('dataset has no CIDEr-D document-frequency table')
            key = {'Bleu_4': 'sent', 'ROUGE_L': 'sent', 'METEOR': 'meteor', 'CIDEr': 'cider'}[m]
            if key in self._tables:
                continue
            st, en = self._ranges()
            if key == 'sent':
                lab = torch.from_numpy(np.ascontiguousarray(self.ds.labels, dtype=np.int64))
                t = self._upload(ops.metric_build_tables(lab, st, en, self.use_eos))
            elif key == 'meteor':
                _, _, stems = self._vocab_ids()
                if len(stems) > 65534:
                    raise ValueError('vocabulary of %d entries; the packed n-gram keys hold '
                                     '65,534' % len(stems))
                stems_t = torch.from_numpy(stems)
                t = self._upload(ops.metric_build_tables(self._label_table('canon').cpu(), st, en,
                                                         0, stems_t))
                t = dict(t, _stems=stems_t.to(self._dev))
            else:
                import math
                keys, vals, ref_len = self.ds.df
                keys = np.ascontiguousarray(keys, dtype=np.uint64)
                vals = np.ascontiguousarray(vals, dtype=np.float32)
                lab = torch.from_numpy(np.ascontiguousarray(self.ds.labels, dtype=np.int64))
                log_ref_len = math.log(float(ref_len))
                t = self._upload(ops.cider_build_tables(
                    lab, st, en, torch.from_numpy(keys.view(np.int64)), torch.from_numpy(vals),
                    log_ref_len, self.use_eos))
                t = dict(t, _log_ref_len=log_ref_len)
            self._tables[key] = t

    # -- scoring -------------------------------------------------------------------
    def score_slots(self, metric, rows, vid, exclude, stats=False):
        """One metric of the given slots in one launch: ``rows`` (N) label rows
        (the hypotheses), ``vid`` (N) their videos, ``exclude`` (N) or None, all
        int64 tensors on the scoring device.  Returns an (N,) tensor there
        (fp32; METEOR fp64, with ``stats`` the pair ((N, 6) int32 alignment
        statistics, scores)).  Tables must be built (:meth:`build_tables`)."""
        ops = _ext.ops()
        gpu = self.backend == 'gpu'
        if metric == 'METEOR':
            t = self._tables['meteor']
            hyps = self._label_table('canon').index_select(0, rows)
            tabs = {k: v for k, v in t.items() if not k.startswith('_')}
            fn = ops.meteor_stats if gpu else ops.meteor_stats_cpu
            st, sc = fn(hyps, vid, tabs, t['_stems'], exclude=exclude)
            return (st, sc) if stats else sc
        hyps = self._label_table('raw').index_select(0, rows)
        if metric == 'CIDEr':
            t = self._tables['cider']
            tabs = {k: v for k, v in t.items() if not k.startswith('_')}
            fn = ops.cider_score if gpu else ops.cider_score_cpu
            return fn(hyps, vid, tabs, t['_log_ref_len'], self.use_eos, exclude=exclude)
        fn = ops.metric_score if gpu else ops.metric_score_cpu
        return fn(metric, hyps, vid, self._tables['sent'], self.use_eos, exclude=exclude)

    def scores(self, seq_per_img, metrics=METRICS, remove_in_ref=True):
        """``{metric: (Nv, S) float64 numpy}``: the consensus score of caption
        slot ``i`` of every video (videos in dataset order)."""
        S = int(seq_per_img)
        if S <= 0:
            raise ValueError('seq_per_img must be positive')
        for m in metrics:
            if m not in METRICS:
                raise ValueError('metric must be one of %s, got %r' % (METRICS, m))
        if 'CIDEr' in metrics and self.ds.df is None:
            raise ValueError('dataset has no CIDEr-D document-frequency table')
        rows, vid, ex = consensus_slots(self.ds.label_start_ix, self.ds.label_end_ix, S,
                                        remove_in_ref)
        nv = len(self.ds.label_start_ix)
        if self.backend == 'cpu-ref':
            return {m: self._score_reference(m, rows, vid, ex).reshape(nv, S) for m in metrics}
        self.build_tables(metrics)
        rows_t, vid_t, ex_t = (torch.from_numpy(a).to(self._dev) for a in (rows, vid, ex))
        out = {m: self.score_slots(m, rows_t, vid_t, ex_t) for m in metrics}
        return {m: s.cpu().numpy().astype(np.float64).reshape(nv, S) for m, s in out.items()}

    # -- oracle --------------------------------------------------------------------
    def _score_reference(self, metric, rows, vid, ex):
        """The Python scorers, the caption's own row removed from its video's
        references (kept when it is the only one)."""
        from ..reward.rewards import score_hypotheses
        ds = self.ds
        labels = np.asarray(ds.labels, dtype=np.int64)
        hyps = labels[rows]
        gts = []
        for v, e in zip(vid, ex):
            g = ds.gts_of(int(v))
            if 0 <= e < len(g) and len(g) > 1:
                g = np.delete(g, int(e), axis=0)
            gts.append(g)
        if metric == 'METEOR':
            from ..eval.metrics import Meteor
            from ..utils.text import sequence_tokens
            words = self._vocab_ids()[0]
            sent = lambda row: ' '.join(words[t] for t in sequence_tokens(row, 0))
            met = Meteor()
            met.java = False  # (the native approximation is the oracle)
            res = {i: [sent(h)] for i, h in enumerate(hyps)}
            refs = {i: [sent(r) for r in g] for i, g in enumerate(gts)}
            return np.asarray(met.compute_score(refs, res)[1], dtype=np.float64)
        if metric == 'CIDEr':
            from .cider_d import CiderDScorer
            oracle = CiderDScorer(ds, self.use_eos, 'cpu', 'cpu-ref')._oracle_scorer()
        else:
            from ..eval.metrics import Bleu, Rouge
            oracle = Bleu(4) if metric == 'Bleu_4' else Rouge()
        return score_hypotheses(oracle, hyps, gts, seq_per_img=1, expand_feat=1,
                                use_eos=self.use_eos)


def set_token_consensus(opt, dataset, device):
    """``--consensus_scorer tokens``: compute the training split's
    ``bcmrscores`` with :class:`ConsensusScorer` (``S = train_seq_per_img``,
    leave-one-out, the metric of ``--eval_metric``, or with ``--reward_mix`` the
    same weighted sum of CIDEr-D / BLEU-4 / ROUGE-L as the reward) and set it on
    ``dataset``,
    also in device tensors that are already cached.  Deterministic, so every
    data-parallel rank computes the same table itself.  Returns the matrix."""
    if getattr(opt, 'train_bcmrscores_pkl', None):
        raise ValueError('--consensus_scorer tokens computes the consensus scores itself; '
                         '--train_bcmrscores_pkl must not be given with it')
    from .reward_mix import METRICS as MIX_METRICS, opt_weights
    weights = opt_weights(opt)  # (--reward_mix: the baseline in the mixed metric)
    metric = consensus_metric(opt.eval_metric)
    key = (metric, int(opt.train_seq_per_img), int(opt.use_eos))
    if weights is not None:
        key = (weights, int(opt.train_seq_per_img), int(opt.use_eos))
    if getattr(dataset, '_token_consensus', None) == key:
        return dataset.bcmrscores
    scorer = ConsensusScorer(dataset, use_eos=opt.use_eos, device=device, backend='auto')
    if weights is None:
        bcmr = scorer.scores(opt.train_seq_per_img, (metric,), remove_in_ref=True)[metric]
    else:  # (once at start-up, on the host: fp64 weighted sum of the metrics in use)
        used = tuple(m for m, w in zip(MIX_METRICS, weights) if w)
        per = scorer.scores(opt.train_seq_per_img, used, remove_in_ref=True)
        bcmr = sum(w * per[m] for m, w in zip(MIX_METRICS, weights) if w)
    dataset.bcmrscores = bcmr
    dataset._token_consensus = key
    for d in dataset._device_cache.values():  # (normally empty: set before the first batch)
        some = d['feats'][0]
        d['bcmrscores'] = torch.from_numpy(bcmr).float().to(some.device)
    return bcmr
