"""Mixed-metric RL reward (``--reward_mix``, ``ops/reward_mix.py``) on the CPU:
the specification parser, ``MixedRewardScorer`` on the host backends against
the fp64 blend of the Python oracles, the ``build_scorer`` dispatch, SCST / CST
steps of the torch path and the CST baselines in the mixed metric.
Inputs, oracles and tolerances: tests/reward_mix_cases.py.
"""
import numpy as np
import pytest
import torch

import consensus_cases
import reward_mix_cases as cases
import sent_metric_cases as sm
from cst_captioning_amd import _ext
from cst_captioning_amd.ops.reward_mix import MixedRewardScorer, parse_reward_mix

W = cases.WEIGHTS


def _need_ext():
    if not _ext.host_available():
        pytest.skip('native extension not built')


# -- the flag ---------------------------------------------------------------------
def test_parser_accepts_the_example_and_omissions():
    assert parse_reward_mix('CIDEr:1,Bleu_4:5,ROUGE_L:5') == (1.0, 5.0, 5.0)
    assert parse_reward_mix('ROUGE_L:0.5, CIDEr:2') == (2.0, 0.0, 0.5)  # (fixed order)
    assert parse_reward_mix('Bleu_4:3') == (0.0, 3.0, 0.0)
    assert parse_reward_mix('CIDEr:0,Bleu_4:1e-1') == (0.0, 0.1, 0.0)


@pytest.mark.parametrize('spec,message', [
    ('CIDEr:1,SPICE:2', 'unknown metric'),
    ('CIDEr:1,METEOR:1', 'host'),
    ('CIDEr:1,CIDEr:2', 'twice'),
    ('CIDEr:-1', 'negative'),
    ('CIDEr:inf', 'finite'),
    ('Bleu_4:nan', 'finite'),
    ('CIDEr:0,Bleu_4:0', 'all weights are zero'),
    ('CIDEr', 'METRIC:WEIGHT'),
    ('CIDEr:x', 'not a number'),
])
def test_parser_rejections_name_the_problem(spec, message, capsys):
    from cst_captioning_amd.config import parse_opts
    with pytest.raises(ValueError, match=message):
        parse_reward_mix(spec)
    with pytest.raises(SystemExit):  # (at parse time)
        parse_opts(['--reward_mix', spec])
    assert message in capsys.readouterr().err


def test_flag_default_is_off():
    from cst_captioning_amd.config import default_opts, parse_opts
    assert default_opts().reward_mix == ''
    assert parse_opts(['--reward_mix', 'CIDEr:1,Bleu_4:5']).reward_mix == 'CIDEr:1,Bleu_4:5'


# -- the scorer on the host backends ------------------------------------------------
@pytest.mark.parametrize('use_eos', [0, 1])
def test_cases_are_not_vacuous(use_eos):
    all3, discordant = cases.check_not_vacuous(use_eos)
    print('use_eos %d: all three positive %.3f, discordant pairs %.3f'
          % (use_eos, all3, discordant))


@pytest.mark.parametrize('use_eos', [0, 1])
@pytest.mark.parametrize('backend', ['cpu-ref', 'cpu'])
def test_scorer_matches_the_oracle_blend(backend, use_eos):
    if backend == 'cpu':
        _need_ext()
    ds, hyps, vid, _ = cases.main_case()
    sc = MixedRewardScorer(ds, W, use_eos=use_eos, device='cpu', backend=backend)
    assert sc.backend == backend
    n = len(hyps) if backend == 'cpu' else 60  # (the Python scorers: a slice is enough)
    h, v = torch.from_numpy(hyps[:n]), torch.from_numpy(vid[:n])
    parts = sc.score_parts(h, v)
    out = sc.score(h, v)
    assert parts.dtype == torch.float32 and parts.shape == (n, 3)
    assert out.dtype == torch.float32 and out.shape == (n,)
    cases.check_parts(parts.numpy(), use_eos, rows=slice(0, n))
    # the blend of the returned parts: three products and two sums in fp32
    want = parts.numpy().astype(np.float64) @ np.asarray(W)
    np.testing.assert_allclose(out.numpy(), want, rtol=2.0 ** -21, atol=0)
    # the class's own oracle is the blend of the Python oracles
    ref = sc.score_reference(h[:40], v[:40])
    assert ref.dtype == np.float64
    np.testing.assert_array_equal(ref, cases.oracle_blend(use_eos)[:40])
    np.testing.assert_allclose(out.numpy()[:40], ref, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize('weights', [(0.0, 5.0, 5.0), (2.0, 0.0, 0.0), (0.0, 0.0, 3.0),
                                     (1.0, 0.0, 4.0)])
def test_zero_weight_columns_are_exactly_zero(weights):
    _need_ext()
    ds, hyps, vid, _ = cases.main_case()
    sc = MixedRewardScorer(ds, weights, use_eos=1, device='cpu', backend='cpu')
    assert (sc.cider is None) == (weights[0] == 0)
    assert (sc.sent is None) == (weights[1] == 0 and weights[2] == 0)
    parts = sc.score_parts(torch.from_numpy(hyps), torch.from_numpy(vid)).numpy()
    cases.check_parts(parts, 1, weights)
    for col in range(3):
        assert bool(parts[:, col].any()) == bool(weights[col])


@pytest.mark.parametrize('backend', ['cpu-ref', 'cpu'])
def test_no_df_table_is_fine_without_cider(backend):
    if backend == 'cpu':
        _need_ext()
    ds, hyps, vid, _ = sm.main_case()
    assert ds.df is None
    sc = MixedRewardScorer(ds, (0.0, 1.0, 2.0), use_eos=0, device='cpu', backend=backend)
    h, v = torch.from_numpy(hyps[:30]), torch.from_numpy(vid[:30])
    want = sm.oracle('main', 'Bleu_4', 0)[:30] + 2.0 * sm.oracle('main', 'ROUGE_L', 0)[:30]
    np.testing.assert_allclose(sc.score(h, v).numpy(), want, rtol=1e-6, atol=1e-30)
    with pytest.raises(ValueError, match='document-frequency'):
        MixedRewardScorer(ds, (1.0, 1.0, 0.0), device='cpu', backend=backend)


def test_scorer_rejects_bad_weights_and_inputs():
    _need_ext()
    ds, hyps, vid, _ = cases.main_case()
    for bad in ((0.0, 0.0, 0.0), (-1.0, 1.0, 1.0), (float('nan'), 1.0, 1.0), (1.0, 2.0)):
        with pytest.raises(ValueError):
            MixedRewardScorer(ds, bad, device='cpu', backend='cpu')
    v2 = torch.zeros(2, dtype=torch.long)
    sc = MixedRewardScorer(ds, W, device='cpu', backend='cpu')
    with pytest.raises(ValueError, match='at most 63'):  # (CIDEr-D in the mix)
        sc.score(torch.full((2, 64), 5), v2)
    with pytest.raises(ValueError, match='65,534'):
        sc.score(torch.tensor([[5, 70000, 6, 0], [5, 6, 7, 0]]), v2)
    sent = MixedRewardScorer(ds, (0.0, 1.0, 1.0), device='cpu', backend='cpu')
    assert sent.score(torch.full((2, 64), 5), v2).shape == (2,)
    with pytest.raises(ValueError, match='at most 64'):
        sent.score(torch.full((2, 65), 5), v2)


# -- build_scorer -------------------------------------------------------------------
@pytest.mark.parametrize('reward_device,backend', [('gpu', 'cpu'), ('cpu', 'cpu-ref')])
def test_build_scorer_dispatch(reward_device, backend):
    _need_ext()
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.ops.cider_d import CiderDScorer, GenericScorer
    from cst_captioning_amd.ops.sent_metrics import SentenceMetricScorer
    from cst_captioning_amd.train.trainer import build_scorer
    ds, hyps, vid, _ = cases.main_case()
    dev = torch.device('cpu')
    before = {'CIDEr': CiderDScorer, 'MSRVTT': CiderDScorer, 'Loss': CiderDScorer,
              'Bleu_4': SentenceMetricScorer, 'ROUGE_L': SentenceMetricScorer,
              'METEOR': GenericScorer}
    for metric, kind in before.items():  # without the flag: exactly as before
        opt = default_opts(eval_metric=metric, use_eos=1, reward_device=reward_device)
        assert type(build_scorer(opt, ds, dev)) is kind, metric
        opt.reward_mix = 'CIDEr:1,Bleu_4:5,ROUGE_L:5'  # (the reward no longer follows it)
        sc = build_scorer(opt, ds, dev)
        assert type(sc) is MixedRewardScorer and sc.weights == W and sc.use_eos == 1
        assert sc.backend == backend
    got = sc.score(torch.from_numpy(hyps[:20]), torch.from_numpy(vid[:20])).numpy()
    np.testing.assert_allclose(got, cases.oracle_blend(1)[:20], rtol=1e-5, atol=1e-4)


# -- training steps on the torch path -------------------------------------------------
def _train_argv(*extra):
    return ['--synthetic', 'msvd', '--synthetic_videos', '24', '--synthetic_vocab', '60',
            '--seq_length', '12', '--feat_dims', '8', '6', '--rnn_size', '16',
            '--input_encoding_size', '16', '--batch_size', '4', '--train_seq_per_img', '5',
            '--test_seq_per_img', '5', '--test_batch_size', '4', '--use_rl', '1',
            '--use_rl_after', '0', '--use_mixer', '1', '--mixer_from', '1', '--use_eos', '1',
            '--impl', 'torch', '--precision', 'fp32', '--language_eval', '0', '--max_epochs', '1',
            '--loglevel', 'ERROR', '--reward_mix', 'CIDEr:1,Bleu_4:5,ROUGE_L:5'] + list(extra)


def _trainer(*extra):
    from cst_captioning_amd.cli import build_model, load_splits
    from cst_captioning_amd.config import parse_opts
    from cst_captioning_amd.data import CaptionLoader
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.train.trainer import Trainer
    opt = parse_opts(_train_argv(*extra))
    tr_ds, _, _ = load_splits(opt)
    dev = torch.device('cpu')
    loader = CaptionLoader(tr_ds, opt.batch_size, opt.train_seq_per_img, 'train', dev, seed=1)
    opt.vocab, opt.vocab_size = loader.get_vocab(), loader.get_vocab_size()
    opt.seq_length, opt.feat_dims = loader.get_seq_length(), loader.get_feat_dims()
    torch.manual_seed(0)
    model, engine = build_model(opt, dev, 'torch')
    trainer = Trainer(opt, model, loader, None, DistContext(device=dev), engine)
    trainer.rl_training = True
    return trainer, loader, tr_ds, opt


@pytest.mark.parametrize('extra', [('--use_cst', '0'),
                                   ('--use_cst', '1', '--scb_baseline', '2',
                                    '--scb_captions', '5')], ids=['scst', 'cst'])
def test_rl_step_rewards_the_mix(extra):
    """The step's mean sample score is the mean oracle blend of its own
    samples (fp32 scores and mean: rtol 1e-5)."""
    _need_ext()
    trainer, loader, ds, opt = _trainer(*extra)
    batch = loader.get_batch()
    out = trainer.train_step(batch, 0)
    assert type(trainer.scorer) is MixedRewardScorer and trainer.scorer.weights == W
    assert np.isfinite(float(out['loss']))
    seq = out['seq']
    vid = batch['video_index'].repeat_interleave(5)
    want = trainer.scorer.score_reference(seq, vid)
    assert (want > 0).any()
    np.testing.assert_allclose(float(out['m']), want.mean(), rtol=1e-5, atol=1e-8)


def test_log_line_labels_the_reward_mix(caplog):
    import logging
    _need_ext()
    trainer, loader, ds, opt = _trainer('--use_cst', '0')
    out = trainer.train_step(loader.get_batch(), 0)
    with caplog.at_level(logging.INFO):
        trainer._log(out, 0.0)
    assert 'mix (m)' in caplog.text and 'mix (b)' in caplog.text
    assert 'CIDEr (m)' not in caplog.text


# -- CST / WXE baselines ---------------------------------------------------------------
@pytest.mark.parametrize('use_eos', [0, 1])
def test_token_consensus_in_the_mixed_metric(use_eos):
    _need_ext()
    import copy
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.ops.consensus import set_token_consensus
    ds = copy.copy(consensus_cases.dataset('hand'))  # (the shared one stays as it is)
    ds._device_cache = {}
    opt = default_opts(reward_mix='CIDEr:1,Bleu_4:5,ROUGE_L:5', use_eos=use_eos,
                       train_seq_per_img=consensus_cases.S, eval_metric='METEOR')
    got = set_token_consensus(opt, ds, torch.device('cpu'))
    assert got is ds.bcmrscores and got.dtype == np.float64
    ref = consensus_cases.reference('hand', use_eos)
    want = sum(w * ref[m] for m, w in zip(cases.COLS, W))
    # per metric: BLEU / ROUGE the oracle rounded to fp32 within two ulps,
    # CIDEr-D rtol = atol = 1e-5 (tests/test_consensus.py); weighted and summed
    tol = sum(w * (sm.RTOL * np.abs(ref[m]) if m != 'CIDEr' else 1e-5 * np.abs(ref[m]) + 1e-5)
              + w * 2.0 ** -24 * np.abs(ref[m]) for m, w in zip(cases.COLS, W))
    assert (np.abs(got - want) <= tol).all(), np.abs(got - want).max()
    assert ds._token_consensus[0] == W
    assert set_token_consensus(opt, ds, torch.device('cpu')) is got  # (cached)
    opt.reward_mix = 'CIDEr:1,Bleu_4:5'  # (other weights: computed again)
    other = set_token_consensus(opt, ds, torch.device('cpu'))
    assert other is not got and not np.array_equal(other, got)


def test_scores_file_with_the_mix_is_refused(tmp_path):
    from cst_captioning_amd.cli import load_splits
    from cst_captioning_amd.config import parse_opts
    from cst_captioning_amd.ops.reward_mix import check_consensus_route
    opt = parse_opts(_train_argv('--use_cst', '1', '--train_bcmrscores_pkl',
                                 str(tmp_path / 'x.pkl')))
    with pytest.raises(ValueError, match='--consensus_scorer tokens'):
        load_splits(opt)
    with pytest.raises(ValueError, match='--consensus_scorer tokens'):
        check_consensus_route(opt)
    opt.use_cst = 0  # (SCST reads no consensus scores)
    check_consensus_route(opt)
