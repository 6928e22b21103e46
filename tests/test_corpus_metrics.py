"""Token-space validation scorer on the CPU: the native C++ twins
(``backend='cpu'``) against the oracle (``backend='cpu-ref'``: the project's
``Bleu(4)`` / ``Meteor()`` / ``Rouge()`` / ``Cider()`` on space-joined words),
and ``Trainer.validate`` with ``--val_scorer tokens``.  Cases and bounds:
``corpus_metric_cases.py``.
"""
import numpy as np
import pytest
import torch

import corpus_metric_cases as cases
from cst_captioning_amd import _ext
from cst_captioning_amd.ops.corpus_metrics import KEYS, CorpusScorer, corpus_bleu, vocab_ids


def test_vocabulary_stems():
    words, canon, stems = vocab_ids(cases.VOCAB)
    assert np.array_equal(canon, np.arange(len(words)))  # (no duplicated words)
    assert len(set(stems[len(cases.SPECIALS):].tolist())) == 19
    assert stems[cases.ID['runs']] == stems[cases.ID['running']] == stems[cases.ID['run']]
    assert stems[cases.ID['man']] != stems[cases.ID['men']]
    # tokens with equal words share a canonical id
    _, canon2, stems2 = vocab_ids(cases.VOCAB + ['dog'])
    assert canon2[-1] == cases.ID['dog'] and stems2[-1] == stems[cases.ID['dog']]


def test_oracle_statistics_reproduce_its_scores():
    """The integer statistics the oracle reports are the ones behind the
    values of ``Bleu.compute_score`` / ``Meteor.compute_score``."""
    ref = cases.reference(24)
    for k, b in enumerate(corpus_bleu(ref['segments']['bleu_stats'])):
        assert abs(b - ref['scores']['Bleu_%d' % (k + 1)]) <= 1e-12 * b
    assert set(ref['scores']) == set(KEYS)
    from cst_captioning_amd.ops.corpus_metrics import corpus_meteor
    m = corpus_meteor(ref['segments']['meteor_stats'])
    assert abs(m - ref['scores']['METEOR']) <= 1e-9 * m
    # the cases do what they are there for: both stages fire, chunks vary
    ms = ref['segments']['meteor_stats']
    assert (ms[:, 0] > 0).any() and (ms[:, 1] > 0).any() and (ms[:, 4] > 1).any()
    # ... and the choice between equidistant candidates decides statistics: with
    # the larger j in place of the smaller the oracle's numbers change, in the
    # exact stage (video 7) and in the stem stage (video 12)
    for nv in (13, 24):
        _, _, vi = cases.make_case(nv)
        changed = set(vi[cases.changed_by_opposite_tie_break(nv)].tolist())
        assert {7, 12} <= changed, changed


@pytest.mark.parametrize('nv', cases.SIZES)
def test_cpu_matches_oracle(nv):
    ds, seqs, vi = cases.make_case(nv)
    got = CorpusScorer(ds, 'cpu', 'cpu').score(torch.from_numpy(seqs.copy()),
                                               torch.from_numpy(vi.copy()))
    assert set(got['scores']) == set(KEYS)
    cases.check_against_oracle(got, nv)


def test_hand_made_alignments():
    """Statistics of the hand-made videos, worked out by hand."""
    ds, seqs, vi = cases.make_case(13)
    got = CorpusScorer(ds, 'cpu', 'cpu').score(seqs, vi)['segments']['meteor_stats']
    by_video = {int(v): got[i].tolist() for i, v in enumerate(vi)}
    assert by_video[0] == [4, 0, 4, 4, 1, 4]      # exact copy: one chunk
    assert by_video[1][:3] == [0, 0, 0]           # empty hypothesis
    assert by_video[1][4:] == [0, 0]
    assert by_video[4] == [4, 0, 4, 4, 1, 4]      # BOS in the middle is dropped
    assert by_video[6] == [5, 0, 5, 5, 3, 5]      # crossing: the dog | walks | a man
    # equidistant candidates, the smaller j wins: (0, 1) | (1, 0) | (2, 5), three
    # chunks (two with the larger j); once in the exact and once in the stem stage
    assert by_video[7] == [3, 0, 3, 6, 3, 3]
    assert by_video[12] == [2, 1, 3, 6, 3, 3]
    assert by_video[8][:2] == [0, 3]              # stem stage only
    assert by_video[3][0] >= 1 and by_video[3][2] == 64


def test_errors():
    ds, seqs, vi = cases.make_case(13)
    sc = CorpusScorer(ds, 'cpu', 'cpu')
    with pytest.raises(ValueError):
        sc.score(np.zeros((13, 65), np.int64), vi)
    with pytest.raises(ValueError):
        sc.score(seqs[:12], vi[:12])                      # partial
    dup = vi.copy()
    dup[0] = dup[1]
    with pytest.raises(ValueError):
        sc.score(seqs, dup)                               # duplicated
    with pytest.raises(ValueError):
        CorpusScorer(ds, 'cpu', 'cpu-ref').score(seqs, dup)
    with pytest.raises(ValueError):
        sc.score(np.full((13, 4), len(cases.VOCAB), np.int64), vi)
    # the unclipped flag leaves the CIDEr-D op as it was
    ops = _ext.ops()
    h, v = torch.from_numpy(seqs[:, :63].copy()), torch.from_numpy(vi.copy())
    a = ops.cider_score_cpu(h, v, sc._cider_tables, sc.log_ref_len, 0)
    b = ops.cider_score_cpu(h, v, sc._cider_tables, sc.log_ref_len, 0, True)
    assert torch.equal(a, b)


def _trainer(val_scorer, **extra):
    from cst_captioning_amd.cli import build_model
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import CaptionLoader, make_synthetic
    from cst_captioning_amd.train.trainer import Trainer
    ds = make_synthetic('msvd', num_videos=10, vocab_size=40, seq_length=10, feat_dims=[16, 8],
                        seed=3)
    kw = dict(batch_size=4, train_seq_per_img=3, test_batch_size=4, test_seq_per_img=3,
              rnn_size=32, input_encoding_size=32, beam_size=2, impl='torch', drop_prob_lm=0.0,
              val_scorer=val_scorer, max_epochs=1, print_log_interval=0)
    kw.update(extra)
    opt = default_opts(**kw)
    dev = torch.device('cpu')
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    opt.vocab_size, opt.seq_length, opt.feat_dims = ds.vocab_size, ds.seq_length, ds.feat_dims
    torch.manual_seed(7)
    model, engine = build_model(opt, dev, 'torch')
    train = CaptionLoader(ds, 4, 3, 'train', dev)
    val = CaptionLoader(ds, 4, 3, 'test', dev)
    return Trainer(opt, model, train, val, None, engine), val, ds


def test_trainer_validate_tokens_cpu():
    tr_s, val_s, _ = _trainer('strings')
    tr_t, val_t, ds = _trainer('tokens')
    res_s = tr_s.validate(val_s)
    res_t = tr_t.validate(val_t)
    assert res_t['predictions'] == res_s['predictions']
    assert res_t['scores']['Loss'] == res_s['scores']['Loss']
    ref = CorpusScorer(ds, 'cpu', 'cpu-ref').score(res_t['sequences'], res_t['video_index'])
    for k in KEYS:
        assert res_t['scores'][k] == round(ref['scores'][k], 5), k
    assert tr_t.corpus_scorer(val_t) is tr_t.corpus_scorer(val_t)  # built once per loader


def test_trainer_validate_tokens_avglogp(tmp_path):
    """``output_logp=1``: the tokens route pads the batches' rows to one width
    before its copy; the avglogp of every prediction, their mean and the GT
    array written beside the model are the strings run's.  Greedy decoding
    (``beam_size=1``) leaves rows without EOS here, and the decoder is wrapped
    so that every second batch comes back two columns narrower: the mean of a
    row without EOS in a narrower batch must not run on into the padding."""
    out = {}
    for mode in ('strings', 'tokens'):
        mf = str(tmp_path / (mode + '.pth'))
        tr, val, _ = _trainer(mode, output_logp=1, beam_size=1, model_file=mf)
        sample, calls, shapes = tr.model.sample, [], []

        def narrow(feats, opts, sample=sample, calls=calls, shapes=shapes):
            seq, logseq = sample(feats, opts)
            calls.append(1)
            if len(calls) % 2 == 0:
                seq, logseq = seq[:, :-2], logseq[:, :-2]
            shapes.append((seq.size(1), bool((seq != 0).all(1).any())))
            return seq, logseq

        tr.model.sample = narrow
        out[mode] = (tr.validate(val), np.load(mf.replace('.pth', '_gt_avglogps.npy')))
        # (the case is there: a narrower batch that holds a row without EOS)
        assert any(w < max(x for x, _ in shapes) and no_eos for w, no_eos in shapes), shapes
    (res_s, gt_s), (res_t, gt_t) = out['strings'], out['tokens']
    assert res_t['predictions'] == res_s['predictions']
    assert all('avglogp' in p for p in res_t['predictions'])
    assert res_t['scores']['avglogp'] == res_s['scores']['avglogp']
    assert res_t['scores']['Loss'] == res_s['scores']['Loss']
    assert np.array_equal(gt_t, gt_s)


def test_trainer_tokens_without_language_eval_builds_no_scorer():
    tr, val, _ = _trainer('tokens', language_eval=0)
    res = tr.validate(val)
    assert set(res['scores']) == {'Loss'} and len(res['predictions']) == 10
    assert tr._corpus_scorers == {}


def test_trainer_tokens_needs_labels():
    from cst_captioning_amd.data import CaptionLoader
    from cst_captioning_amd.data.dataset import VideoCaptionDataset
    tr, _, ds = _trainer('tokens')
    bare = VideoCaptionDataset(ds.vocab, ds.videos, ds.feats)
    bare_loader = CaptionLoader(bare, 4, 3, 'test', 'cpu')
    with pytest.raises(ValueError, match='labels'):
        tr.validate(bare_loader)
    # at set-up, for the validation loader and for the loaders the CLI evaluates
    from cst_captioning_amd.train.trainer import Trainer, check_val_scorer
    with pytest.raises(ValueError, match='labels'):
        Trainer(tr.opt, tr.model, tr.train_loader, bare_loader, None, None)
    with pytest.raises(ValueError, match='labels'):
        check_val_scorer(tr.opt, bare_loader)
    tr.opt.val_scorer = 'strings'
    check_val_scorer(tr.opt, bare_loader)
