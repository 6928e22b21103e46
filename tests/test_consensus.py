"""GT consensus scores in token space (``ops/consensus.py``,
``--consensus_scorer tokens``) on the CPU: the native scorers' leave-one-out
``exclude`` argument against the Python oracles, its no-op conditions, the
``prepro.evalscores --scorer tokens`` round trip and the trainer."""
import numpy as np
import pytest
import torch

import consensus_cases as cases
from sent_metric_cases import ATOL, RTOL

from cst_captioning_amd import _ext

pytestmark = pytest.mark.skipif(not _ext.host_available(), reason='native extension not built')


def _scorer(name, use_eos):
    from cst_captioning_amd.ops.consensus import ConsensusScorer
    return ConsensusScorer(cases.dataset(name), use_eos=use_eos, backend='cpu')


def _check(got, want):
    """Native scores against the oracles: BLEU / ROUGE as tests/sent_metric_cases.py
    (the oracle rounded once to fp32, two ulps), CIDEr-D as the native scorer in
    tests/test_cider.py, METEOR segment scores as tests/test_gpu_corpus_metrics.py."""
    for m in ('Bleu_4', 'ROUGE_L'):
        w32 = want[m].astype(np.float32)
        np.testing.assert_allclose(got[m].astype(np.float32), w32, rtol=RTOL, atol=ATOL,
                                   err_msg=m)
        assert np.array_equal(got[m] == 0, w32 == 0), m
    np.testing.assert_allclose(got['CIDEr'], want['CIDEr'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got['METEOR'], want['METEOR'], rtol=1e-9, atol=0)


@pytest.mark.parametrize('use_eos', [0, 1])
@pytest.mark.parametrize('name', ['hand', 'synthetic'])
def test_native_twins_match_the_oracles(name, use_eos):
    got = _scorer(name, use_eos).scores(cases.S)
    want = cases.reference(name, use_eos)
    nv = cases.dataset(name).num_videos
    assert all(got[m].shape == (nv, cases.S) and got[m].dtype == np.float64 for m in got)
    _check(got, want)


@pytest.mark.parametrize('name', ['hand', 'synthetic'])
def test_meteor_statistics_are_exact(name):
    from cst_captioning_amd.ops.consensus import consensus_slots
    sc = _scorer(name, 0)
    sc.build_tables(('METEOR',))
    ds = cases.dataset(name)
    rows, vid, ex = (torch.from_numpy(a) for a in
                     consensus_slots(ds.label_start_ix, ds.label_end_ix, cases.S, True))
    stats, _ = sc.score_slots('METEOR', rows, vid, ex, stats=True)
    assert np.array_equal(stats.numpy().astype(np.int64), cases.reference_meteor_stats(name))


def test_hand_cases_hold_what_they_are_for():
    """The oracle values that make the hand-made store a test: not vacuous."""
    from cst_captioning_amd.ops.consensus import ConsensusScorer
    ds = cases.dataset('hand')
    loo = cases.reference('hand', 0)
    full = ConsensusScorer(ds, backend='cpu-ref').scores(cases.S, remove_in_ref=False)
    # v0 caption 0: the only holder of "plays" x 3 -> its unigram precision drops
    assert full['Bleu_4'][0, 0] == pytest.approx(1.0) and 0 < loo['Bleu_4'][0, 0] < 1
    # v0 slot 4 cycles to caption 0 (ncap 4 < S)
    assert loo['Bleu_4'][0, 4] == loo['Bleu_4'][0, 0]
    # v2: the same caption twice
    assert loo['Bleu_4'][2, 0] == pytest.approx(1.0) and loo['ROUGE_L'][2, 1] == 1.0
    # v3: a single caption is kept
    assert loo['ROUGE_L'][3, 0] == 1.0 and loo['METEOR'][3, 0] == full['METEOR'][3, 0] > 0
    # v4 caption 0: brevity penalty against length 3 (none) instead of 9
    assert 0 < loo['Bleu_4'][4, 0] < 1
    # v5 caption 0 has a twin through the duplicate vocabulary word (METEOR works
    # on words); caption 1 keeps a stem match ("running" / "runs") with the rest
    assert loo['METEOR'][5, 0] == full['METEOR'][5, 0] and loo['ROUGE_L'][5, 0] < 1
    assert 0 < loo['METEOR'][5, 1] < full['METEOR'][5, 1]
    assert cases.reference_meteor_stats('hand')[5 * cases.S + 1, 1] > 0  # (n_stem)
    assert (loo['ROUGE_L'] < full['ROUGE_L']).any() and (loo['CIDEr'] < full['CIDEr']).any()


@pytest.mark.parametrize('use_eos', [0, 1])
def test_exclude_noop_is_bit_equal(use_eos):
    """``exclude=None``, all -1 and out-of-range entries give the bits of the
    call without the keyword, for every entry point that has it."""
    ops = _ext.ops()
    sc = _scorer('hand', use_eos)
    sc.build_tables()
    ds = cases.dataset('hand')
    rows = torch.arange(ds.labels.shape[0])
    vid = torch.from_numpy(np.repeat(np.arange(ds.num_videos),
                                     ds.label_end_ix - ds.label_start_ix))
    n = rows.numel()
    ncap = torch.from_numpy(ds.label_end_ix - ds.label_start_ix)[vid]
    noops = [None, torch.full((n,), -1, dtype=torch.int64), ncap.clone(), ncap + 100,
             torch.full((n,), -(2 ** 40), dtype=torch.int64)]
    raw, canon = sc._label_table('raw')[rows], sc._label_table('canon')[rows]
    ct = {k: v for k, v in sc._tables['cider'].items() if not k.startswith('_')}
    mt = {k: v for k, v in sc._tables['meteor'].items() if not k.startswith('_')}
    lrl, stems = sc._tables['cider']['_log_ref_len'], sc._tables['meteor']['_stems']
    base = {'Bleu_4': ops.metric_score_cpu('Bleu_4', raw, vid, sc._tables['sent'], use_eos),
            'ROUGE_L': ops.metric_score_cpu('ROUGE_L', raw, vid, sc._tables['sent'], use_eos),
            'CIDEr': ops.cider_score_cpu(raw, vid, ct, lrl, use_eos),
            'METEOR': ops.meteor_stats_cpu(canon, vid, mt, stems)}
    for ex in noops:
        for m in base:
            got = sc.score_slots(m, rows, vid, ex, stats=True)
            if m == 'METEOR':
                assert torch.equal(got[0], base[m][0]) and torch.equal(got[1], base[m][1])
            else:
                assert torch.equal(got, base[m]), (m, ex)
    # without exclusion every GT caption finds itself: ROUGE-L 1 ...
    assert bool((base['ROUGE_L'] == 1).all())
    # ... and with it not all of them do (an ignored argument would)
    own = torch.from_numpy(np.concatenate([np.arange(c) for c in
                                           ds.label_end_ix - ds.label_start_ix]))
    loo = sc.score_slots('ROUGE_L', rows, vid, own)
    assert 0 < int((loo == 1).sum()) < n  # (the twin captions and the single one stay 1)
    for m in ('Bleu_4', 'CIDEr'):
        assert not torch.equal(sc.score_slots(m, rows, vid, own), base[m]), m
    assert not torch.equal(sc.score_slots('METEOR', rows, vid, own), base['METEOR'][1])


def test_table_keys_for_leave_one_out_bleu():
    """ng_cnt2 / ng_arg of the hand store: the only holder of "plays" x 3, the
    "dog" x 2 tie."""
    sc = _scorer('hand', 0)
    sc.build_tables(('Bleu_4',))
    t = sc._tables['sent']
    off = t['vid_ng_off'].numpy()
    keys, cnt, cnt2, arg = (t[k].numpy() for k in ('ng_key', 'ng_cnt', 'ng_cnt2', 'ng_arg'))

    def entry(v, tok):
        g = off[v] + int(np.where(keys[off[v]:off[v + 1]] == tok + 1)[0][0])
        return int(cnt[g]), int(cnt2[g]), int(arg[g])
    assert entry(0, cases.W['plays']) == (3, 2, 0)
    assert entry(0, cases.W['the']) == (1, 0, 3)
    assert entry(1, cases.W['dog']) == (2, 2, -1)
    assert (cnt2 <= cnt).all() and ((arg >= 0) | (cnt2 == cnt)).all()
    # a table dict without the new keys still scores, and refuses an exclusion
    old = {k: v for k, v in t.items() if k not in ('ng_cnt2', 'ng_arg')}
    ops = _ext.ops()
    hyps = sc._label_table('raw')[:4]
    vid = torch.zeros(4, dtype=torch.int64)
    assert torch.equal(ops.metric_score_cpu('Bleu_4', hyps, vid, old, 0),
                       ops.metric_score_cpu('Bleu_4', hyps, vid, t, 0))
    with pytest.raises(ValueError):
        ops.metric_score_cpu('Bleu_4', hyps, vid, old, 0, exclude=torch.arange(4))


def test_cider_needs_a_df_table():
    from cst_captioning_amd.ops.consensus import ConsensusScorer
    ds = cases.make_dataset([[[3, 4], [4, 5]]])
    ds.df = None
    sc = ConsensusScorer(ds, backend='cpu')
    assert set(sc.scores(2, ('Bleu_4', 'ROUGE_L', 'METEOR'))) == {'Bleu_4', 'ROUGE_L', 'METEOR'}
    with pytest.raises(ValueError):
        sc.scores(2, ('CIDEr',))


def test_evalscores_tokens_round_trip(tmp_path):
    """``prepro.evalscores --scorer tokens`` writes what ``load_scores`` and the
    file path of the trainer read back: the scorer's matrices."""
    from cst_captioning_amd.data import formats
    from cst_captioning_amd.prepro import evalscores
    from cst_captioning_amd.prepro.ciderdf import save_df
    ds = cases.dataset('synthetic')
    label_file = str(tmp_path / 'train_sequencelabel.npz')
    formats.save_label_file(label_file, {
        'videos': np.array(ds.videos), 'vocab': np.array(ds.vocab), 'labels': ds.labels,
        'label_start_ix': ds.label_start_ix, 'label_end_ix': ds.label_end_ix})
    keys, vals, ref_len = ds.df
    df_file = str(tmp_path / 'train_ciderdf.pkl')
    save_df(df_file, dict(zip(keys.tolist(), vals.tolist())), ref_len, write_pickle=False)
    out = str(tmp_path / 'train_evalscores.pkl')
    evalscores.main(['unused_cocofmt.json', out, '--scorer', 'tokens', '--label_file', label_file,
                     '--cached_tokens', df_file, '--seq_per_img', str(cases.S), '--use_eos', '1',
                     '--remove_in_ref'])
    want = _scorer('synthetic', 1).scores(cases.S)
    for m in evalscores.METRICS:
        for path in (out, out[:-4] + '.npz'):
            assert np.array_equal(evalscores.load_scores(path, m), want[m]), m


def _train_argv(tmp_path, *extra):
    return ['--synthetic', 'msvd', '--synthetic_videos', '24', '--synthetic_vocab', '60',
            '--seq_length', '12', '--feat_dims', '8', '6', '--rnn_size', '16',
            '--input_encoding_size', '16', '--batch_size', '4', '--train_seq_per_img', '5',
            '--test_seq_per_img', '5', '--test_batch_size', '4', '--use_rl', '1',
            '--use_rl_after', '0', '--use_cst', '1', '--scb_baseline', '1', '--scb_captions', '5',
            '--use_mixer', '1', '--mixer_from', '1', '--use_eos', '1', '--impl', 'torch',
            '--precision', 'fp32', '--language_eval', '0', '--max_epochs', '1',
            '--loglevel', 'ERROR', '--consensus_scorer', 'tokens'] + list(extra)


@pytest.mark.parametrize('metric', ['CIDEr', 'ROUGE_L'])
def test_trainer_takes_a_cst_step_on_token_consensus(tmp_path, metric):
    """CPU torch path: the trainer computes bcmrscores itself (the synthetic
    split comes without), a batch carries the scorer's rows, a CST step runs."""
    from cst_captioning_amd.cli import build_model, load_splits
    from cst_captioning_amd.config import parse_opts
    from cst_captioning_amd.data import CaptionLoader
    from cst_captioning_amd.ops.consensus import ConsensusScorer
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.train.trainer import Trainer
    opt = parse_opts(_train_argv(tmp_path, '--eval_metric', metric))
    tr_ds, _, _ = load_splits(opt)
    assert tr_ds.bcmrscores is None  # (no Python consensus pass in this mode)
    dev = torch.device('cpu')
    loader = CaptionLoader(tr_ds, opt.batch_size, opt.train_seq_per_img, 'train', dev, seed=1)
    opt.vocab, opt.vocab_size = loader.get_vocab(), loader.get_vocab_size()
    opt.seq_length, opt.feat_dims = loader.get_seq_length(), loader.get_feat_dims()
    torch.manual_seed(0)
    model, engine = build_model(opt, dev, 'torch')
    trainer = Trainer(opt, model, loader, None, DistContext(device=dev), engine)
    want = ConsensusScorer(tr_ds, use_eos=1, backend='cpu').scores(5, (metric,))[metric]
    assert np.array_equal(tr_ds.bcmrscores, want)
    trainer.rl_training = True
    batch = loader.get_batch()
    assert np.array_equal(batch['bcmrscores'].numpy(),
                          want[batch['vids']].astype(np.float32))
    out = trainer.train_step(batch, 0)
    assert np.isfinite(float(out['loss']))
    # scb_baseline 1: the logged baseline is the mean consensus score of the batch
    np.testing.assert_allclose(float(out['b']), want[batch['vids']].astype(np.float32).mean(),
                               rtol=1e-5)


def test_train_main_with_token_consensus(tmp_path):
    from cst_captioning_amd.cli import train_main
    infos = train_main(_train_argv(tmp_path))
    assert infos['iter'] > 0


def test_token_consensus_refuses_a_scores_file(tmp_path):
    from cst_captioning_amd.cli import load_splits
    from cst_captioning_amd.config import parse_opts
    from cst_captioning_amd.ops.consensus import set_token_consensus
    opt = parse_opts(_train_argv(tmp_path, '--train_bcmrscores_pkl', str(tmp_path / 'x.pkl')))
    with pytest.raises(ValueError):
        load_splits(opt)
    with pytest.raises(ValueError):
        set_token_consensus(opt, cases.dataset('synthetic'), torch.device('cpu'))
