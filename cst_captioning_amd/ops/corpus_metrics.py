"""Validation metrics in token space: corpus BLEU-1..4, METEOR, ROUGE-L and
coco CIDEr of one decoded caption per video, on the GPU or through the native
C++ twins (``--val_scorer tokens``).

The default validation route (``--val_scorer strings``) copies every batch to
the host, builds Python strings and runs the pure-Python scorers of
:mod:`..eval.metrics`.  Here the captions stay token ids:

  * per split, ONCE: every vocabulary entry gets a canonical id (tokens with
    equal words share one) and a stem id (:mod:`..eval.stem`); the label table
    is reduced (BOS dropped, stop at the first EOS) into the reference tables of
    ``csrc/host/metric_host.cpp`` (BLEU n-gram unions, ROUGE token rows, METEOR
    stem rows) and ``csrc/host/cider_host.cpp`` (tf-idf vectors with the
    split's own document frequencies, ``log(number of videos)``);
  * per call: ``bleu_stats_kernel`` and ``meteor_stats_kernel``
    (``csrc/kernels/corpus_metrics.hip``) write integer statistics per
    hypothesis, ``rouge_l_kernel`` and the unclipped ``cider_d`` body write
    fp32 sentence scores; the corpus sums (int64) and final formulas are
    evaluated on the host in fp64.

Oracle (``backend='cpu-ref'``): ``Bleu(4)``, ``Meteor()`` (native
approximation), ``Rouge()`` and ``Cider()`` applied to the space-joined
vocabulary words of the reduced rows (no ``ptb_tokenize``).  Differences from
the strings route: references truncated to ``seq_length`` and out-of-vocabulary
words (UNK) come from the label file, not from the coco-format file, and a
``<start>`` inside a decoded caption is dropped.

Limits of the table-based backends (``ValueError``): hypotheses and reduced
references of at most 64 tokens, vocabularies of at most 65,534 entries (16-bit
token packing, as in :mod:`.sent_metrics`).
"""
import math

import numpy as np
import torch

from .. import _ext
from ..utils.text import sequence_tokens

KEYS = ('Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'METEOR', 'ROUGE_L', 'CIDEr')
MAX_TOKENS = 64
BLEU_STATS = ('correct_1', 'correct_2', 'correct_3', 'correct_4', 'guess_1', 'guess_2',
              'guess_3', 'guess_4', 'tlen', 'rlen')
METEOR_STATS = ('n_exact', 'n_stem', 'len_h', 'len_r', 'chunks', 'n_pairs')


def vocab_ids(vocab):
    """(words, canonical ids, stem ids) of a vocabulary: tokens with equal
    words share a canonical id (the first such token), tokens with equal stems
    a stem id."""
    from ..eval.stem import stem
    words = [w.decode() if isinstance(w, bytes) else str(w) for w in vocab]
    canon = np.zeros(len(words), dtype=np.int64)
    stems = np.zeros(len(words), dtype=np.int32)
    first, stem_of = {}, {}
    for i, w in enumerate(words):
        canon[i] = first.setdefault(w, i)
        stems[i] = stem_of.setdefault(stem(w), len(stem_of))
    return words, canon, stems


def corpus_bleu(stats):
    """Bleu_1..4 from (N, 10) per-hypothesis statistics: the corpus expression
    of ``Bleu.compute_score`` on the int64 sums."""
    tot = [int(x) for x in np.asarray(stats, dtype=np.int64).sum(0)]
    tiny, small = 1e-15, 1e-9
    bleus, b = [], 1.0
    for k in range(4):
        b *= (tot[k] + tiny) / (tot[4 + k] + small)
        bleus.append(b ** (1.0 / (k + 1)))
    ratio = (tot[8] + tiny) / (tot[9] + small)
    if ratio < 1:
        bleus = [x * math.exp(1 - 1 / ratio) for x in bleus]
    return bleus


def corpus_meteor(stats):
    """METEOR from the summed (N, 6) alignment statistics of each segment's
    best reference (``Meteor.compute_score`` / ``Meteor._score``)."""
    from ..eval.metrics import Meteor
    ne, ns, lh, lr, chunks, npairs = (int(x) for x in np.asarray(stats, dtype=np.int64).sum(0))
    m = ne * Meteor.w_exact + ns * Meteor.w_stem
    if m <= 0 or lh <= 0 or lr <= 0:
        return 0.0
    P, R = m / lh, m / lr
    fmean = P * R / (Meteor.alpha * P + (1 - Meteor.alpha) * R)
    pen = Meteor.gamma * (chunks / float(npairs)) ** Meteor.beta
    return (1 - pen) * fmean


class CorpusScorer:
    """``score(seqs, video_index)`` -> ``{'scores': {7 keys}, 'segments': {...}}``
    for one decoded caption per video of ``dataset``.

    ``segments``: ``bleu_stats`` (N, 10) int (:data:`BLEU_STATS`),
    ``meteor_stats`` (N, 6) int (:data:`METEOR_STATS`), ``METEOR`` (N,) fp64,
    ``ROUGE_L`` and ``CIDEr`` (N,) sentence scores -- numpy arrays in the order
    of ``seqs``.
    """

    def __init__(self, dataset, device='cpu', backend='auto'):
        if not dataset.has_label:
            raise ValueError('the token-space validation scorer needs a split with labels')
        self.ds = dataset
        self.device = torch.device(device)
        if backend == 'auto':
            backend = 'gpu' if self.device.type == 'cuda' else 'cpu'
        if backend not in ('gpu', 'cpu', 'cpu-ref'):
            raise ValueError('unknown backend %r' % (backend,))
        if backend != 'cpu-ref' and not _ext.host_available():
            raise ValueError('the token-space validation scorer (backend %r) needs the native '
                             'extension, which is not built' % (backend,))
        if backend == 'gpu' and self.device.type != 'cuda':
            raise ValueError("backend 'gpu' needs a cuda device, got %s" % (self.device,))
        self.backend = backend
        self.nv = dataset.num_videos
        self.words, self.canon, self.stems = vocab_ids(dataset.vocab)
        self.log_ref_len = math.log(float(self.nv))
        if backend != 'cpu-ref':
            self._build_tables()

    # -- tables (once per split) -------------------------------------------------
    def _build_tables(self):
        from ..prepro.ciderdf import df_from_token_refs
        ds, V = self.ds, len(self.words)
        if V > 65534:
            raise ValueError('vocabulary of %d entries; the packed n-gram keys hold 65,534' % V)
        labels = np.asarray(ds.labels, dtype=np.int64)
        if labels.size and (labels.min() < 0 or labels.max() >= V):
            raise ValueError('label token outside the vocabulary of %d entries' % V)
        lab = np.ascontiguousarray(self.canon[labels])
        st = np.ascontiguousarray(ds.label_start_ix, dtype=np.int64)
        en = np.ascontiguousarray(ds.label_end_ix, dtype=np.int64)
        ops = _ext.ops()
        lab_t, st_t, en_t = torch.from_numpy(lab), torch.from_numpy(st), torch.from_numpy(en)
        self.stems_t = torch.from_numpy(self.stems)
        mt = ops.metric_build_tables(lab_t, st_t, en_t, 0, self.stems_t)
        # coco CIDEr: document frequencies of the scored split's own references
        refs = [[sequence_tokens(row, 0) for row in lab[a:b]] for a, b in zip(st, en)]
        packed, n = df_from_token_refs(refs)
        keys = np.fromiter(packed.keys(), dtype=np.uint64, count=len(packed))
        vals = np.fromiter(packed.values(), dtype=np.float32, count=len(packed))
        ct = ops.cider_build_tables(lab_t, st_t, en_t, torch.from_numpy(keys.view(np.int64)),
                                    torch.from_numpy(vals), self.log_ref_len, 0)
        self.canon_t = torch.from_numpy(self.canon)
        if self.backend == 'gpu':
            mt = {k: v.to(self.device) for k, v in mt.items()}
            ct = {k: v.to(self.device) for k, v in ct.items()}
            self.stems_t = self.stems_t.to(self.device)
            self.canon_t = self.canon_t.to(self.device)
        self._metric_tables, self._cider_tables = mt, ct

    # -- scoring -------------------------------------------------------------------
    def score(self, seqs, video_index):
        """seqs: (N, T) decoded token ids, video_index: (N,) dataset video
        indices, which must cover every video of the split exactly once (the
        corpus document frequencies assume that)."""
        seqs, vi = [x if torch.is_tensor(x) else torch.from_numpy(np.array(x, dtype=np.int64))
                    for x in (seqs, video_index)]
        if seqs.dim() != 2 or vi.dim() != 1 or vi.numel() != seqs.size(0):
            raise ValueError('seqs (N, T) and video_index (N)')
        if self.backend == 'cpu-ref':
            vi_h = vi.detach().cpu().numpy().astype(np.int64)
            self._check_cover(vi_h)
            return self._score_reference(seqs.detach().cpu().numpy(), vi_h)
        if seqs.size(1) > MAX_TOKENS:
            raise ValueError('hypotheses of %d tokens; at most %d are supported'
                             % (seqs.size(1), MAX_TOKENS))
        dev = self.device if self.backend == 'gpu' else torch.device('cpu')
        seqs = seqs.detach().to(dev, torch.int64).contiguous()
        vi = vi.detach().to(dev, torch.int64).contiguous()
        # (two synchronising checks before any table is indexed: the cover of
        # video_index, then the token range)
        V = self.canon_t.numel()
        ok = vi.numel() == self.nv
        if ok:
            ok = bool((torch.equal(torch.sort(vi).values,
                                   torch.arange(self.nv, device=dev))))
        if not ok:
            self._check_cover(vi.cpu().numpy())
        if seqs.numel() and bool(((seqs < 0) | (seqs >= V)).any()):
            raise ValueError('hypothesis token outside the vocabulary of %d entries' % V)
        hyps = self.canon_t[seqs]
        ops = _ext.ops()
        mt, ct = self._metric_tables, self._cider_tables
        if self.backend == 'gpu':
            bleu = ops.bleu_stats(hyps, vi, mt)
            met, met_seg = ops.meteor_stats(hyps, vi, mt, self.stems_t)
            rouge = ops.metric_score('ROUGE_L', hyps, vi, mt, 0)
            cider = ops.cider_score(hyps, vi, ct, self.log_ref_len, 0, False)
        else:
            bleu = ops.bleu_stats_cpu(hyps, vi, mt)
            met, met_seg = ops.meteor_stats_cpu(hyps, vi, mt, self.stems_t)
            rouge = ops.metric_score_cpu('ROUGE_L', hyps, vi, mt, 0)
            cider = ops.cider_score_cpu(hyps, vi, ct, self.log_ref_len, 0, False)
        seg = {'bleu_stats': bleu.cpu().numpy().astype(np.int64),
               'meteor_stats': met.cpu().numpy().astype(np.int64),
               'METEOR': met_seg.cpu().numpy(),
               'ROUGE_L': rouge.cpu().numpy(),
               'CIDEr': cider.cpu().numpy()}
        return {'scores': self._corpus_scores(seg), 'segments': seg}

    def _check_cover(self, vi):
        if vi.shape[0] != self.nv or not np.array_equal(np.sort(vi), np.arange(self.nv)):
            raise ValueError('video_index must cover every video of the split exactly once '
                             '(%d videos, got %d indices)' % (self.nv, vi.shape[0]))

    @staticmethod
    def _corpus_scores(seg):
        out = {'Bleu_%d' % (k + 1): b for k, b in enumerate(corpus_bleu(seg['bleu_stats']))}
        out['METEOR'] = corpus_meteor(seg['meteor_stats'])
        out['ROUGE_L'] = float(np.mean(seg['ROUGE_L'].astype(np.float64)))
        out['CIDEr'] = float(np.mean(seg['CIDEr'].astype(np.float64)))
        return out

    # -- oracle --------------------------------------------------------------------
    def _sentence(self, row):
        return ' '.join(self.words[t] for t in sequence_tokens(row, 0))

    def _score_reference(self, seqs, vi):
        """The project's validation scorers on space-joined vocabulary words."""
        from ..eval.metrics import Bleu, Meteor, Rouge, _ngrams
        from ..reward.cider_d_cpu import Cider
        gts = {int(v): [self._sentence(r) for r in self.ds.gts_of(int(v))] for v in vi}
        res = {int(v): [self._sentence(seqs[i])] for i, v in enumerate(vi)}
        bleus, _ = Bleu(4).compute_score(gts, res)
        scores = {'Bleu_%d' % (k + 1): b for k, b in enumerate(bleus)}
        met = Meteor()
        met.java = False  # (the native approximation is the oracle)
        scores['METEOR'], met_seg = met.compute_score(gts, res)
        scores['ROUGE_L'], rouge = Rouge().compute_score(gts, res)
        scores['CIDEr'], cider = Cider().compute_score(gts, res)
        # the integer statistics behind the BLEU and METEOR values
        bstats, mstats = [], []
        for k in res:
            hyp = res[k][0].split()
            refs = [r.split() for r in gts[k]]
            maxc = {}
            for r in refs:
                for g, c in _ngrams(r, 4).items():
                    maxc[g] = max(maxc.get(g, 0), c)
            correct = [0] * 4
            for g, c in _ngrams(hyp, 4).items():
                correct[len(g) - 1] += min(c, maxc.get(g, 0))
            tlen = len(hyp)
            rlen = min((abs(len(r) - tlen), len(r)) for r in refs)[1]
            bstats.append(correct + [max(0, tlen - j) for j in range(4)] + [tlen, rlen])
            m, lh, lr, chunks, npairs = max((met._stats(hyp, r) for r in refs), key=met._score)
            n_stem = int(round((npairs * met.w_exact - m) / (met.w_exact - met.w_stem)))
            mstats.append([npairs - n_stem, n_stem, lh, lr, chunks, npairs])
        seg = {'bleu_stats': np.array(bstats, dtype=np.int64).reshape(-1, 10),
               'meteor_stats': np.array(mstats, dtype=np.int64).reshape(-1, 6),
               'METEOR': np.asarray(met_seg, dtype=np.float64),
               'ROUGE_L': np.asarray(rouge, dtype=np.float64),
               'CIDEr': np.asarray(cider, dtype=np.float64)}
        return {'scores': {k: float(scores[k]) for k in KEYS}, 'segments': seg}
