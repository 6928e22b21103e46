"""Consensus (MBR) decoding under a mixed utility (``--mbr_mix``) on the CPU: the
native twin of ``csrc/kernels/peer_mix.hip`` and the Python backend against the
fp64 oracles and against the table scorers with leave-one-out, zero weights,
non-vacuity of the cases, the hand-made selection, the flag's grammar,
``Trainer.validate`` and the test command."""
import numpy as np
import pytest
import torch

import mbr_cases as mc
import peer_mix_cases as pc

CASES = pc.cases()
IDS = pc.case_ids()


def _scorer(use_eos, backend, weights=pc.WEIGHTS, df=True):
    from cst_captioning_amd.ops.mbr import PeerMix
    return PeerMix(mc.df_table() if df else None, weights, use_eos=use_eos, backend=backend)


@pytest.mark.parametrize('case', CASES, ids=IDS)
@pytest.mark.parametrize('backend', ['cpu', 'cpu-ref'])
def test_columns_match_oracle(case, backend):
    ref = pc.oracle(case)
    sc = _scorer(case.use_eos, backend)
    hy = torch.from_numpy(case.hyps)
    out, parts = sc.score_both(hy, case.G)
    assert out.dtype == torch.float32 and out.shape == (len(case.hyps),)
    pc.check_parts(parts.numpy(), ref)
    # the blend: three products and two sums in fp32
    want = pc.blend(parts.numpy())
    assert (np.abs(out.numpy() - want) <= 2.0 ** -21 * want).all()
    assert torch.equal(sc.score(hy, case.G), out) and torch.equal(sc.score_parts(hy, case.G), parts)
    # cpu-ref is the Python oracle itself
    assert np.allclose(sc.score_reference(hy, case.G), pc.blend(ref), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_twin_matches_table_scorers_with_exclude(case):
    """The second reference: the pool rows as the reference table of one video,
    row i scored with its own reference left out -- the same integers and the
    same fp64 formulas, so the same bits."""
    from cst_captioning_amd import _ext
    parts = _scorer(case.use_eos, 'cpu').score_parts(torch.from_numpy(case.hyps), case.G).numpy()
    tab = pc.table_columns(_ext.ops().metric_score_cpu, case.hyps, case.G, case.use_eos)
    assert np.array_equal(parts[:, 1], tab['Bleu_4'])
    assert np.array_equal(parts[:, 2], tab['ROUGE_L'])


@pytest.mark.parametrize('backend', ['cpu', 'cpu-ref'])
def test_zero_weights(backend):
    from cst_captioning_amd.ops.mbr import PeerCiderD, PeerMix
    case = CASES[IDS.index('rand_G5_B3_eos1')]
    hy = torch.from_numpy(case.hyps)
    full = _scorer(case.use_eos, backend).score_parts(hy, case.G)
    # no CIDEr: no df table anywhere
    sc = _scorer(case.use_eos, backend, (0.0, 5.0, 5.0), df=False)
    assert sc.cider is None and sc._tables is None
    out, parts = sc.score_both(hy, case.G)
    assert not parts[:, 0].any() and torch.equal(parts[:, 1:], full[:, 1:])
    for w, col in (((0.0, 3.0, 0.0), 1), ((0.0, 0.0, 0.7), 2), ((3.0, 0.0, 0.0), 0)):
        out, parts = _scorer(case.use_eos, backend, w, df=bool(w[0])).score_both(hy, case.G)
        assert torch.equal(parts[:, col], full[:, col])
        others = [c for c in range(3) if c != col]
        assert not parts[:, others].any()
        assert torch.equal(out, torch.tensor(w[col], dtype=torch.float32) * parts[:, col])
    # (w_c, 0, 0) is w_c x the CIDEr-D scorer
    peer = PeerCiderD(mc.df_table(), use_eos=case.use_eos, backend=backend).score(hy, case.G)
    out = _scorer(case.use_eos, backend, (2.0, 0.0, 0.0)).score(hy, case.G)
    assert torch.equal(out, 2.0 * peer)
    with pytest.raises(ValueError, match='document-frequency'):
        PeerMix(None, (1.0, 0.0, 1.0), backend=backend)
    for bad in ((0.0, 0.0, 0.0), (1.0, -1.0, 0.0), (1.0, float('nan'), 0.0), (1.0, 2.0)):
        with pytest.raises(ValueError, match='weights'):
            PeerMix(mc.df_table(), bad, backend=backend)


def test_argument_errors():
    from cst_captioning_amd import _ext
    from cst_captioning_amd.ops.mbr import PeerMix, df_hash_table
    keys, vals, _ = mc.df_table()
    t = df_hash_table(keys, vals)
    f = _ext.ops().metric_score_cpu
    hy = torch.from_numpy(CASES[0].hyps)  # 4 rows
    none = torch.zeros(0, dtype=torch.long)
    w = list(pc.WEIGHTS)
    out, parts = f('mix', hy, none, None, 0, cider_tables=t, log_ref_len=3.0, weights=w, group=2)
    assert out.shape == (4,) and parts.shape == (4, 3)
    with pytest.raises(RuntimeError, match='at least 2'):
        f('mix', hy, none, None, 0, cider_tables=t, log_ref_len=3.0, weights=w, group=1)
    with pytest.raises(RuntimeError, match='whole pools'):
        f('mix', hy, none, None, 0, cider_tables=t, log_ref_len=3.0, weights=w, group=3)
    with pytest.raises(RuntimeError, match='exclude'):
        f('mix', hy, none, None, 0, exclude=torch.zeros(4, dtype=torch.long), cider_tables=t,
          log_ref_len=3.0, weights=w, group=2)
    with pytest.raises(RuntimeError, match='weights'):
        f('mix', hy, none, None, 0, cider_tables=t, log_ref_len=3.0, group=2)
    with pytest.raises(RuntimeError, match='df tables'):
        f('mix', hy, none, None, 0, log_ref_len=3.0, weights=w, group=2)
    with pytest.raises(RuntimeError, match='metric mix'):
        f('Bleu_4', hy, none, None, 0, weights=w, group=2)
    with pytest.raises(ValueError, match='zero'):
        f('mix', hy, none, None, 0, weights=[0.0, 0.0, 0.0], group=2)
    # without group the binding is the table scorer of before
    with pytest.raises(RuntimeError, match='Bleu_4 or ROUGE_L'):
        f('mix', hy, torch.zeros(4, dtype=torch.long), {}, 0)
    with pytest.raises(RuntimeError, match='peer mode'):
        f('Bleu_4', hy, torch.zeros(4, dtype=torch.long), {}, 0, weights=w)
    # token ids the packed keys cannot hold: refused by BLEU / CIDEr-D, not by ROUGE-L
    big = torch.tensor([[5, 70000, 6, 0], [5, 6, 7, 0]])
    with pytest.raises(ValueError, match='65534'):
        f('mix', big, none, None, 0, weights=[0.0, 1.0, 1.0], group=2)
    assert f('mix', big, none, None, 0, weights=[0.0, 0.0, 1.0], group=2)[0].shape == (2,)
    with pytest.raises(ValueError, match='65,534'):
        PeerMix(None, (0.0, 1.0, 0.0), backend='cpu', vocab_size=70000)
    assert PeerMix(None, (0.0, 1.0, 0.0), backend='cpu-ref', vocab_size=70000).backend == 'cpu-ref'
    sc = PeerMix(None, (0.0, 1.0, 1.0), backend='cpu')
    with pytest.raises(ValueError, match='at least 2'):
        sc.score(hy, 1)
    with pytest.raises(ValueError, match='whole pools'):
        sc.score(hy, 3)
    # the twin takes pools beyond the kernel's limit, and empty batches
    many = torch.from_numpy(np.tile(CASES[-2].hyps[:21], (10, 1))[:200])
    assert sc.score(many, 100).shape == (200,)
    assert sc.score(hy[:0], 2).shape == (0,)


def test_cases_are_not_vacuous():
    """On the oracle alone: the columns are non-trivial and the utilities
    disagree about the consensus caption."""
    rows = over = pos = 0
    differ = {1: 0, 2: 0}
    for case in CASES:
        ref = pc.oracle(case)
        rows += len(ref)
        over += int((ref[:, 1] > 1e-3).sum())
        pos += int((ref[:, 2] > 0).sum())
        pools = ref.reshape(-1, case.G, 3)
        best = [[int(np.flatnonzero(p[:, c] == p[:, c].max())[0]) for p in pools]
                for c in range(3)]
        for c in (1, 2):
            differ[c] += sum(a != b for a, b in zip(best[0], best[c]))
    assert over >= 0.5 * rows, (over, rows)
    assert pos >= 0.8 * rows, (pos, rows)
    assert differ[1] >= 5 and differ[2] >= 5, differ


@pytest.mark.parametrize('backend', ['cpu', 'cpu-ref'])
def test_hand_made_selection(backend):
    """ROUGE-L picks the interleaved row (longest common subsequence), CIDEr-D
    the row that shares n-grams with every peer (peer_mix_cases.HAND_ROWS)."""
    hy = torch.from_numpy(pc.HAND.hyps)
    ref = pc.oracle(pc.HAND)
    assert int(ref[:, 0].argmax()) == pc.HAND_BEST['CIDEr'] == 0
    assert int(ref[:, 2].argmax()) == pc.HAND_BEST['ROUGE_L'] == 1
    np.testing.assert_allclose(ref[:, 2], [0.557077626, 0.586538462, 1 / 3, 1 / 3], rtol=1e-8)
    best, scores = _scorer(0, backend, (0.0, 0.0, 1.0), df=False).select(hy, 4)
    assert best.tolist() == [1] and scores.shape == (1, 4)
    best, _ = _scorer(0, backend, (1.0, 0.0, 0.0)).select(hy, 4)
    assert best.tolist() == [0]


def test_mbr_mix_flag_grammar():
    from cst_captioning_amd.config import parse_opts
    from cst_captioning_amd.ops.reward_mix import parse_reward_mix
    assert parse_opts([]).mbr_mix == ''
    assert parse_opts(['--mbr_mix', 'CIDEr:1,Bleu_4:5,ROUGE_L:5']).mbr_mix == \
        'CIDEr:1,Bleu_4:5,ROUGE_L:5'
    assert parse_reward_mix('ROUGE_L:2, Bleu_4:0.5', '--mbr_mix') == (0.0, 0.5, 2.0)
    bad = {'METEOR:1': 'METEOR', 'CIDEr:1,METEOR:2': 'METEOR', 'Foo:1': 'unknown metric',
           'CIDEr:1,CIDEr:2': 'twice', 'CIDEr': 'METRIC:WEIGHT', 'CIDEr:': 'METRIC:WEIGHT',
           ':1': 'METRIC:WEIGHT', 'CIDEr:x': 'not a number', 'CIDEr:nan': 'not finite',
           'CIDEr:inf': 'not finite', 'Bleu_4:-1': 'negative', 'CIDEr:0,Bleu_4:0': 'all weights',
           ' ': 'empty'}
    for spec, why in bad.items():
        with pytest.raises(ValueError, match=why) as e:
            parse_reward_mix(spec, '--mbr_mix')
        assert str(e.value).startswith('--mbr_mix: '), spec
        # the training flag's messages are the same text under its own name
        with pytest.raises(ValueError) as e0:
            parse_reward_mix(spec)
        assert str(e0.value) == str(e.value).replace('--mbr_mix', '--reward_mix', 1)
        if spec.strip():
            with pytest.raises(SystemExit):
                parse_opts(['--mbr_mix', spec])


# -- trainer, CLI -------------------------------------------------------------------
def _trainer(df=True, **extra):
    from cst_captioning_amd.cli import build_model
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import CaptionLoader, make_synthetic
    from cst_captioning_amd.train.trainer import Trainer
    ds = make_synthetic('msvd', num_videos=10, vocab_size=40, seq_length=10, feat_dims=[16, 8],
                        seed=3)
    if not df:
        ds.df = None
    kw = dict(batch_size=4, train_seq_per_img=3, test_batch_size=4, test_seq_per_img=3,
              rnn_size=32, input_encoding_size=32, beam_size=2, impl='torch', drop_prob_lm=0.0,
              val_scorer='tokens', max_epochs=1, print_log_interval=0, decode='mbr',
              mbr_samples=5, mbr_temperature=0.8, use_eos=1)
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


def test_trainer_validate_rouge_without_df_table():
    from cst_captioning_amd.ops.mbr import PeerCiderD, PeerMix, select_best
    tr, val, ds = _trainer(df=False, mbr_mix='ROUGE_L:1')
    assert isinstance(tr.mbr_scorer, PeerMix) and tr.mbr_scorer.weights == (0.0, 0.0, 1.0)
    assert tr.mbr_scorer.cider is None and tr.mbr_scorer.use_eos == 1
    seen = []
    sample_mbr = tr.model.sample_mbr

    def recording(feats, o):
        seq, lp, info = sample_mbr(feats, o)
        seen.append((seq, info))
        return seq, lp, info
    tr.model.sample_mbr = recording
    torch.manual_seed(3)
    res = tr.validate(val)
    assert len(res['predictions']) == 10 and len(seen) == 3
    assert all(0.0 <= p['mbr_score'] <= 1.0 for p in res['predictions'])
    got = []
    for seq, info in seen:
        pool = info['pool']
        B, G, T = pool.shape
        assert G == 6
        ref = pc.oracle_parts(pool.reshape(B * G, T).numpy(), G, 1, cider=False)[:, 2]
        best = select_best(torch.from_numpy(ref.astype(np.float32)).view(B, G))
        assert torch.equal(best, info['best'])
        assert torch.equal(seq, pool[torch.arange(B), best])
        got += info['scores'].gather(1, best.view(-1, 1)).view(-1).tolist()
    assert [p['mbr_score'] for p in res['predictions']] == got
    assert max(got) > 0
    # with a df table and no --mbr_mix the scorer is today's
    tr, _, _ = _trainer()
    assert isinstance(tr.mbr_scorer, PeerCiderD)
    tr, _, _ = _trainer(mbr_mix='CIDEr:1,Bleu_4:5,ROUGE_L:5')
    assert isinstance(tr.mbr_scorer, PeerMix) and tr.mbr_scorer.cider is not None


def test_without_mbr_mix_the_df_table_is_still_required():
    with pytest.raises(ValueError, match='document-frequency'):
        _trainer(df=False)
    with pytest.raises(ValueError, match='document-frequency'):
        _trainer(df=False, mbr_mix='CIDEr:1,ROUGE_L:1')


def test_cli_test_with_mbr_mix(tmp_path):
    import json
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
    run_test_cli(base + ['--model_file', mf, '--result_file', rf, '--decode', 'mbr',
                         '--mbr_samples', '4', '--mbr_mix', 'CIDEr:1,Bleu_4:5,ROUGE_L:5'])
    res = json.load(open(rf))
    assert len(res['predictions']) == 8
    assert all(0.0 <= p['mbr_score'] <= 20.0001 for p in res['predictions'])
    # a file-based run whose utility has no CIDEr term passes the df check (and
    # stops later, at the data files it was not given) ...
    with pytest.raises(Exception) as e:
        run_test_cli(['--model_file', mf, '--decode', 'mbr', '--mbr_mix', 'Bleu_4:1',
                      '--loglevel', 'WARNING'])
    assert 'train_cached_tokens' not in str(e.value)
    # ... and with one it names its df table up front, as without --mbr_mix
    with pytest.raises(ValueError, match='train_cached_tokens'):
        run_test_cli(['--model_file', mf, '--decode', 'mbr', '--mbr_mix', 'CIDEr:1,Bleu_4:1',
                      '--loglevel', 'WARNING'])
