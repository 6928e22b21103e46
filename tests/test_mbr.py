"""Consensus (MBR) decoding on the CPU: the native peer CIDEr-D twin and the
Python backend against the fp64 oracle, the independent construction (pool rows
as a reference table + leave-one-out), argument errors, the tie rule,
``CaptionModel.sample_mbr`` on the torch path, ``Trainer.validate`` and the test
command with ``--decode mbr``."""
import json

import numpy as np
import pytest
import torch

import mbr_cases as mc

CASES = mc.cases()


def _scorer(use_eos, backend, device='cpu'):
    from cst_captioning_amd.ops.mbr import PeerCiderD
    return PeerCiderD(mc.df_table(), use_eos=use_eos, device=device, backend=backend)


@pytest.mark.parametrize('case', CASES, ids=mc.case_ids())
@pytest.mark.parametrize('backend', ['cpu', 'cpu-ref'])
def test_peer_scores_match_oracle(case, backend):
    ref = mc.oracle(case)
    got = _scorer(case.use_eos, backend).score(torch.from_numpy(case.hyps), case.G)
    assert got.dtype == torch.float32 and got.shape == (len(case.hyps),)
    err = np.abs(got.numpy() - ref).max()
    print(case.name, backend, 'max err %.3g of %.3g' % (err, ref.max()))
    assert err < mc.tolerance(ref)


def _independent(hyps, G, use_eos, score, device='cpu'):
    """The definition of the feature: the pool rows as the reference table of
    'video' k, row i scored with its own reference left out."""
    import math
    from cst_captioning_amd import _ext
    keys, vals, ref_len = mc.df_table()
    N = len(hyps)
    lab = torch.from_numpy(hyps)
    st = torch.arange(0, N, G)
    t = _ext.ops().cider_build_tables(lab, st, st + G, torch.from_numpy(keys.view(np.int64)),
                                      torch.from_numpy(vals), math.log(ref_len), use_eos)
    t = {k: v.to(device) for k, v in t.items()}
    i = torch.arange(N)
    return score(lab.to(device), (i // G).to(device), t, math.log(ref_len), use_eos,
                 exclude=(i % G).to(device)), t


@pytest.mark.parametrize('case', CASES, ids=mc.case_ids())
def test_twin_matches_independent_construction(case):
    from cst_captioning_amd import _ext
    want, _ = _independent(case.hyps, case.G, case.use_eos, _ext.ops().cider_score_cpu)
    got = _scorer(case.use_eos, 'cpu').score(torch.from_numpy(case.hyps), case.G)
    # (the reference table stores its values in fp32, the twin keeps fp64)
    assert np.abs(got.numpy() - want.numpy()).max() < mc.tolerance(want.numpy())


def test_group_zero_is_the_old_call_bit_for_bit():
    import math
    from cst_captioning_amd import _ext
    case = CASES[-1]
    ops = _ext.ops()
    a, t = _independent(case.hyps, case.G, case.use_eos, ops.cider_score_cpu)
    N = len(case.hyps)
    i = torch.arange(N)
    lrl = math.log(mc.df_table()[2])
    hy = torch.from_numpy(case.hyps)
    b = ops.cider_score_cpu(hy, i // case.G, t, lrl, case.use_eos, exclude=i % case.G, group=0)
    assert torch.equal(a, b)
    for clipped in (True, False):
        a = ops.cider_score_cpu(hy, i // case.G, t, lrl, case.use_eos, clipped)
        b = ops.cider_score_cpu(hy, i // case.G, t, lrl, case.use_eos, clipped, None, 0)
        assert torch.equal(a, b)


def test_argument_errors():
    import math
    from cst_captioning_amd import _ext
    from cst_captioning_amd.ops.mbr import PeerCiderD, df_hash_table
    keys, vals, ref_len = mc.df_table()
    t = df_hash_table(keys, vals)
    assert set(t) == {'ht_keys', 'ht_vals'}  # peer mode reads nothing else
    f = _ext.ops().cider_score_cpu
    hy = torch.from_numpy(CASES[0].hyps)  # 4 rows
    none = torch.zeros(0, dtype=torch.long)
    lrl = math.log(ref_len)
    assert f(hy, none, t, lrl, 0, group=2).shape == (4,)  # (hyp_video is ignored)
    with pytest.raises(RuntimeError, match='at least 2'):
        f(hy, none, t, lrl, 0, group=1)
    with pytest.raises(RuntimeError, match='at least 2'):
        f(hy, none, t, lrl, 0, group=-3)
    with pytest.raises(RuntimeError, match='whole pools'):
        f(hy, none, t, lrl, 0, group=3)
    with pytest.raises(RuntimeError, match='exclude'):
        f(hy, none, t, lrl, 0, exclude=torch.zeros(4, dtype=torch.long), group=2)
    with pytest.raises(RuntimeError, match='clipped'):
        f(hy, none, t, lrl, 0, clipped=False, group=2)
    sc = PeerCiderD(mc.df_table(), backend='cpu')
    with pytest.raises(ValueError, match='at least 2'):
        sc.score(hy, 1)
    with pytest.raises(ValueError, match='whole pools'):
        sc.score(hy, 3)
    with pytest.raises(ValueError, match='document-frequency'):
        PeerCiderD(None)
    with pytest.raises(ValueError, match='backend'):
        PeerCiderD(mc.df_table(), backend='tpu')
    # the CPU twin takes pools beyond the kernel's limit
    big = torch.from_numpy(np.tile(CASES[-1].hyps[:21], (10, 1))[:200])
    assert sc.score(big, 100).shape == (200,)


def test_select_tie_rule():
    from cst_captioning_amd.ops.mbr import select_best
    s = torch.tensor([[1.0, 3.0, 3.0, 2.0], [0.0, 0.0, 0.0, 0.0], [2.0, 1.0, 2.0, 2.0],
                      [0.0, 1.0, 2.0, 3.0]])
    assert select_best(s).tolist() == [1, 0, 0, 3]
    for case in CASES:
        sc = _scorer(case.use_eos, 'cpu')
        best, scores = sc.select(torch.from_numpy(case.hyps), case.G)
        assert scores.shape == (len(case.hyps) // case.G, case.G)
        s = scores.numpy()
        want = [int(np.flatnonzero(r == r.max())[0]) for r in s]
        assert best.tolist() == want
        if case.best is not None:
            assert best.tolist() == case.best.tolist(), case.name


# -- decoder ----------------------------------------------------------------------
def _model(beam_size=1, **extra):
    from cst_captioning_amd.cli import build_model
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import make_synthetic
    ds = make_synthetic('msvd', num_videos=10, vocab_size=40, seq_length=10, feat_dims=[16, 8],
                        seed=3)
    kw = dict(batch_size=4, train_seq_per_img=3, rnn_size=32, input_encoding_size=32,
              beam_size=beam_size, impl='torch', drop_prob_lm=0.0)
    kw.update(extra)
    opt = default_opts(**kw)
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    opt.vocab_size, opt.seq_length, opt.feat_dims = ds.vocab_size, ds.seq_length, ds.feat_dims
    torch.manual_seed(7)
    model, _ = build_model(opt, torch.device('cpu'), 'torch')
    model.eval()
    return model, ds


def _ds_oracle(ds, pool, use_eos):
    """Oracle peer scores of a (B, G, T) pool under the dataset's df."""
    from cst_captioning_amd.ops.mbr import PeerCiderD
    B, G, T = pool.shape
    ref = PeerCiderD(ds.df, use_eos=use_eos, backend='cpu-ref').score_reference(
        pool.reshape(B * G, T).cpu(), G)
    return ref.reshape(B, G)


@pytest.mark.parametrize('beam_size', [1, 3])
def test_sample_mbr_torch_path(beam_size):
    from cst_captioning_amd.data import CaptionLoader
    from cst_captioning_amd.ops.mbr import PeerCiderD
    model, ds = _model(beam_size)
    feats = CaptionLoader(ds, 4, 3, 'test', 'cpu').get_batch_at(0)['feats']
    scorer = PeerCiderD(ds.df, use_eos=1, backend='cpu')
    opt = {'decode': 'mbr', 'beam_size': beam_size, 'mbr_samples': 6, 'mbr_temperature': 1.0,
           'mbr_scorer': scorer}
    before = model.seq_per_img
    torch.manual_seed(11)
    seq, lp, info = model.sample_mbr(feats, opt)
    assert model.seq_per_img == before and model.feat_expander.n == before
    pool, scores, best = info['pool'], info['scores'], info['best']
    B, G, T = pool.shape
    assert (B, G) == (4, 7) and scores.shape == (B, G) and best.shape == (B,)
    assert seq.shape == (B, T) and lp.shape == (B, T)
    # row 0 is the standard decode
    std, std_lp = model.sample(feats, {'beam_size': beam_size})
    assert torch.equal(pool[:, 0, :std.size(1)], std) and not pool[:, 0, std.size(1):].any()
    # the returned row is the selected one, with its log-probs
    for k in range(B):
        assert torch.equal(seq[k], pool[k, best[k]])
    zero = best == 0
    assert torch.equal(lp[zero][:, :std.size(1)], std_lp[zero].float())
    # scores and selection against the oracle
    ref = _ds_oracle(ds, pool, 1)
    assert np.abs(scores.numpy() - ref).max() < mc.tolerance(ref)
    s = scores.numpy()
    assert best.tolist() == [int(np.flatnonzero(r == r.max())[0]) for r in s]
    # sample() dispatches and returns the first two values; the seed fixes the pool
    torch.manual_seed(11)
    seq2, lp2 = model.sample(feats, opt)
    assert torch.equal(seq2, seq) and torch.equal(lp2, lp)
    torch.manual_seed(11)
    assert torch.equal(model.sample_mbr(feats, opt)[2]['pool'], pool)
    torch.manual_seed(12)
    assert not torch.equal(model.sample_mbr(feats, opt)[2]['pool'], pool)
    with pytest.raises(ValueError, match='mbr_scorer'):
        model.sample(feats, {'decode': 'mbr'})


# -- trainer, CLI -------------------------------------------------------------------
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


def test_trainer_validate_mbr_both_scorers():
    res = {}
    for mode in ('strings', 'tokens'):
        tr, val, ds = _trainer(mode, decode='mbr', mbr_samples=5, mbr_temperature=0.8, use_eos=1)
        assert tr.mbr_scorer is not None and tr.mbr_scorer.use_eos == 1
        assert tr.decode_opts()['mbr_samples'] == 5
        torch.manual_seed(3)
        res[mode] = tr.validate(val)
    s, t = res['strings'], res['tokens']
    assert len(s['predictions']) == 10
    assert all('mbr_score' in p and isinstance(p['mbr_score'], float) for p in s['predictions'])
    assert t['predictions'] == s['predictions']  # (same seed: same pools, same choice)
    assert t['scores']['Loss'] == s['scores']['Loss']
    from cst_captioning_amd.ops.corpus_metrics import CorpusScorer
    ref = CorpusScorer(ds, 'cpu', 'cpu-ref').score(t['sequences'], t['video_index'])
    for k in ('Bleu_4', 'METEOR', 'ROUGE_L', 'CIDEr'):
        assert t['scores'][k] == round(ref['scores'][k], 5), k
    # the standard layout is unchanged: no mbr_score, the decode options as before
    tr, val, _ = _trainer('tokens')
    assert tr.mbr_scorer is None and tr.decode_opts() == {'beam_size': 2}
    std = tr.validate(val)
    assert all(set(p) == {'image_id', 'caption'} for p in std['predictions'])


def test_mbr_without_df_fails_at_setup():
    from cst_captioning_amd.train.trainer import Trainer
    tr, val, ds = _trainer('strings')
    tr.opt.decode = 'mbr'
    df, ds.df = ds.df, None
    try:
        with pytest.raises(ValueError, match='document-frequency'):
            Trainer(tr.opt, tr.model, tr.train_loader, val, None, None)
    finally:
        ds.df = df
    tr.opt.mbr_samples = 0
    with pytest.raises(ValueError, match='mbr_samples'):
        Trainer(tr.opt, tr.model, tr.train_loader, val, None, None)


def test_flags_default_to_standard():
    from cst_captioning_amd.config import parse_opts
    opt = parse_opts([])
    assert (opt.decode, opt.mbr_samples, opt.mbr_temperature) == ('standard', 20, 1.0)
    with pytest.raises(SystemExit):
        parse_opts(['--decode', 'other'])


def test_cli_test_with_mbr(tmp_path):
    from cst_captioning_amd.cli import test_main as run_test_cli
    from cst_captioning_amd.cli import train_main
    base = ['--synthetic', 'msvd', '--synthetic_videos', '24', '--synthetic_vocab', '40',
            '--seq_length', '10', '--rnn_size', '32', '--input_encoding_size', '32',
            '--feat_dims', '16', '8', '--batch_size', '6', '--train_seq_per_img', '4',
            '--test_batch_size', '8', '--test_seq_per_img', '4', '--beam_size', '2',
            '--impl', 'torch', '--loglevel', 'WARNING', '--print_log_interval', '0']
    mf = str(tmp_path / 'm.pth')
    train_main(base + ['--max_epochs', '1', '--model_file', mf])
    rf = str(tmp_path / 'mbr.json')
    out = run_test_cli(base + ['--model_file', mf, '--result_file', rf, '--decode', 'mbr',
                               '--mbr_samples', '4', '--mbr_temperature', '0.7'])
    res = json.load(open(rf))
    assert len(res['predictions']) == 8 and all('mbr_score' in p for p in res['predictions'])
    assert res['scores'] == out['scores'] and 'CIDEr' in res['scores']
    # a file-based test run names its df table up front
    with pytest.raises(ValueError, match='train_cached_tokens'):
        run_test_cli(['--model_file', mf, '--decode', 'mbr', '--loglevel', 'WARNING'])
