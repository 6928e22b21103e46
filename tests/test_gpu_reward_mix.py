"""Mixed-metric RL reward on the GPU: ``reward_mix_kernel``
(``csrc/kernels/reward_mix.hip``) against the Python oracles and the
single-metric kernels, and the RL training steps that use it (``--reward_mix``:
captured SCST step, CST step with token-space consensus baselines).
Inputs, oracles and tolerances: tests/reward_mix_cases.py.
"""
import numpy as np
import pytest
import torch

import reward_mix_cases as cases
import sent_metric_cases as sm

pytestmark = pytest.mark.gpu

DEV = 'cuda'
W = cases.WEIGHTS
SPEC = 'CIDEr:1,Bleu_4:5,ROUGE_L:5'


def _mix(ds, weights, use_eos):
    from cst_captioning_amd.ops.reward_mix import MixedRewardScorer
    sc = MixedRewardScorer(ds, weights, use_eos=use_eos, device=torch.device(DEV))
    assert sc.backend == 'gpu'
    return sc


def _sent(ds, metric, use_eos):
    from cst_captioning_amd.ops.sent_metrics import SentenceMetricScorer
    return SentenceMetricScorer(ds, metric, use_eos=use_eos, device=torch.device(DEV),
                                backend='gpu')


def _both(sc, h, v):
    """(out, parts) of ONE launch."""
    out, parts = sc.score_both(h, v)
    return out, parts


@pytest.mark.parametrize('use_eos', [0, 1])
def test_kernel_matches_oracles_and_single_metric_kernels(use_eos):
    """Main case (N = 249, 70 references: past one wavefront), weights (1, 5, 5)."""
    from cst_captioning_amd.ops.cider_d import CiderDScorer
    ds, hyps, vid, _ = cases.main_case()
    cases.check_not_vacuous(use_eos)
    sc = _mix(ds, W, use_eos)
    h, v = torch.from_numpy(hyps).to(DEV), torch.from_numpy(vid).to(DEV)
    out, parts = _both(sc, h, v)
    out2, parts2 = _both(sc, h, v)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.shape == (len(hyps),) and out.is_cuda
    assert parts.dtype == torch.float32 and parts.shape == (len(hyps), 3)
    # two calls on the same inputs: bit-equal
    assert torch.equal(out, out2) and torch.equal(parts, parts2)
    assert torch.equal(sc.score(h, v), out) and torch.equal(sc.score_parts(h, v), parts)
    p = parts.cpu().numpy()
    # BLEU / ROUGE: bit for bit the single-metric kernels, and the oracle
    for col, metric in ((1, 'Bleu_4'), (2, 'ROUGE_L')):
        assert torch.equal(parts[:, col], _sent(ds, metric, use_eos).score(h, v)), metric
        sm.check(np.ascontiguousarray(p[:, col]), 'main', metric, use_eos)
    # CIDEr-D: the bound of test_cider_kernel_matches_oracle
    cases.check_parts(p, use_eos)
    ref = cases.oracle_parts(use_eos)[:, 0]
    assert np.abs(p[:, 0] - ref).max() < 1e-4 * max(1.0, ref.max())
    single = CiderDScorer(ds, use_eos, torch.device(DEV), 'gpu').score(h, v).cpu().numpy()
    print('use_eos %d: max |CIDEr-D column - cider_d_kernel| = %.3g (max score %.3g), '
          'bit-equal rows %d / %d' % (use_eos, np.abs(p[:, 0] - single).max(), single.max(),
                                      int((p[:, 0] == single).sum()), len(single)))
    # the blend: three products and two sums, each rounded once, at most 2^-24
    # each relative to a non-negative partial sum: 5 * 2^-24 < 2^-21
    want = p.astype(np.float64) @ np.asarray(W)
    err = np.abs(out.cpu().numpy().astype(np.float64) - want)
    assert (err <= 2.0 ** -21 * want).all(), (err / np.maximum(want, 1e-300)).max()


@pytest.mark.parametrize('n', [7, 1])
@pytest.mark.parametrize('use_eos', [0, 1])
def test_no_cider_tables_at_all(n, use_eos):
    """w_c = 0 on the tiny case (T = 64, ids up to 65,534, a dataset without a
    df table): BLEU / ROUGE bit-equal to their kernels; N = 7 and N = 1."""
    ds, hyps, vid, _ = cases.tiny_case()
    assert ds.df is None and len(hyps) == 7 and hyps.shape[1] == 64
    weights = (0.0, 5.0, 5.0)
    sc = _mix(ds, weights, use_eos)
    assert sc.cider is None
    h, v = torch.from_numpy(hyps[:n]).to(DEV), torch.from_numpy(vid[:n]).to(DEV)
    out, parts = _both(sc, h, v)
    assert not parts[:, 0].any().item()
    for col, metric in ((1, 'Bleu_4'), (2, 'ROUGE_L')):
        assert torch.equal(parts[:, col], _sent(ds, metric, use_eos).score(h, v)), metric
        np.testing.assert_allclose(parts[:, col].cpu().numpy(),
                                   sm.oracle('tiny', metric, use_eos)[:n].astype(np.float32),
                                   rtol=sm.RTOL, atol=sm.ATOL)
    want = parts.cpu().numpy().astype(np.float64) @ np.asarray(weights)
    err = np.abs(out.cpu().numpy().astype(np.float64) - want)
    assert (err <= 2.0 ** -21 * want).all()
    # one metric alone: the others' columns exactly 0, its own unchanged
    for weights1, col in (((0.0, 2.0, 0.0), 1), ((0.0, 0.0, 3.0), 2)):
        o1, p1 = _both(_mix(ds, weights1, use_eos), h, v)
        assert torch.equal(p1[:, col], parts[:, col])
        assert not p1[:, [c for c in range(3) if c != col]].any().item()
        assert np.array_equal(o1.cpu().numpy(),
                              np.float32(weights1[col]) * p1[:, col].cpu().numpy())


@pytest.mark.parametrize('n', [249, 5, 1])
def test_cider_alone_is_one_rounded_product(n):
    """w_b = w_r = 0 on the main case: no sentence-metric tables, out = w_c
    times the CIDEr-D column, a single rounding."""
    ds, hyps, vid, _ = cases.main_case()
    sc = _mix(ds, (3.0, 0.0, 0.0), 1)
    assert sc.sent is None
    oracle = cases.oracle_parts(1)[:, 0]
    # (all rows, or the first n whose CIDEr-D is positive: row 0 scores 0)
    sel = np.arange(n) if n == len(hyps) else np.flatnonzero(oracle > 0)[:n]
    h, v = torch.from_numpy(hyps[sel]).to(DEV), torch.from_numpy(vid[sel]).to(DEV)
    out, parts = _both(sc, h, v)
    p = parts.cpu().numpy()
    assert p.shape == (n, 3) and not p[:, 1:].any()
    assert np.abs(p[:, 0] - oracle[sel]).max() < 1e-4 * max(1.0, oracle.max())
    assert (p[:, 0] > 0).any()
    assert np.array_equal(out.cpu().numpy(), np.float32(3.0) * p[:, 0])


def test_over_limit_inputs_raise_before_any_launch():
    from cst_captioning_amd import _ext
    from cst_captioning_amd.ops.reward_mix import MixedRewardScorer, reward_mix_score
    ds, hyps, vid, _ = cases.main_case()
    v2 = torch.zeros(2, dtype=torch.long, device=DEV)
    sc = _mix(ds, W, 0)
    with pytest.raises(ValueError, match='at most 63'):  # (CIDEr-D in the mix)
        sc.score(torch.full((2, 64), 5, device=DEV), v2)
    with pytest.raises(RuntimeError, match='at most 63'):  # (the op itself)
        reward_mix_score(torch.full((2, 64), 5, device=DEV), v2, sc.cider._tables,
                         sc.sent._tables, sc.cider.log_ref_len, 0, W)
    sent = _mix(ds, (0.0, 1.0, 1.0), 0)
    assert sent.score(torch.full((2, 64), 5, device=DEV), v2).shape == (2,)
    with pytest.raises(RuntimeError, match='at most 64'):
        reward_mix_score(torch.full((2, 65), 5, device=DEV), v2, None, sent.sent._tables, 0.0, 0,
                         (0.0, 1.0, 1.0))
    with pytest.raises(RuntimeError, match='no tables'):
        reward_mix_score(torch.full((2, 8), 5, device=DEV), v2, None, sent.sent._tables, 0.0, 0, W)
    # the single-metric modes of the extension's op take none of the mix's arguments
    with pytest.raises(RuntimeError, match='mix only'):
        _ext.ops().metric_score('Bleu_4', torch.full((2, 8), 5, device=DEV), v2,
                                sent.sent._tables, 0, weights=[0.0, 1.0, 1.0])
    # a token id over 65,534: in the references, or possible in the hypotheses
    # (the vocabulary), raises when the scorer is built
    big = sm.TableDataset(np.array([[1, 5, 70000, 0]]), (1,))
    with pytest.raises(ValueError, match='65534'):
        MixedRewardScorer(big, (0.0, 1.0, 1.0), device=torch.device(DEV))
    wide = sm.TableDataset(np.array([[1, 5, 6, 0]]), (1,))
    wide.vocab_size = 70000
    with pytest.raises(ValueError, match='65,534'):
        MixedRewardScorer(wide, (0.0, 1.0, 1.0), device=torch.device(DEV))


def _trainer(graph, **kw):
    """tests/test_gpu_sent_metrics.py::_trainer with the mix: the smoke() shape
    (4 videos x 20 captions, V = 1000, H = 512)."""
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import make_synthetic, CaptionLoader
    from cst_captioning_amd.cli import build_model
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.train.trainer import Trainer
    B, S, H = 4, 20, 512
    ds = make_synthetic('msrvtt', num_videos=64, vocab_size=1000, seed=0)
    args = dict(batch_size=B, train_seq_per_img=S, rnn_size=H, input_encoding_size=H,
                drop_prob_lm=0.5, use_rl=1, use_rl_after=0, use_cst=0, use_mixer=1, mixer_from=1,
                use_eos=1, impl='hip', cuda_graph=graph, learning_rate=1e-3, eval_metric='CIDEr',
                reward_mix=SPEC, vocab_size=ds.vocab_size, seq_length=ds.seq_length,
                feat_dims=ds.feat_dims)
    args.update(kw)
    opt = default_opts(**args)
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    torch.manual_seed(0)
    dev = torch.device(DEV)
    model, engine = build_model(opt, dev, 'hip')
    assert engine is not None
    loader = CaptionLoader(ds, B, S, 'train', dev, seed=0)
    tr = Trainer(opt, model, loader, None, DistContext(device=dev), engine)
    tr.rl_training = True
    return tr, loader, ds


def _count_calls(scorer):
    calls = []
    inner = scorer.score

    def score(hyps, video_index):
        calls.append(hyps.shape[0])
        return inner(hyps, video_index)
    scorer.score = score
    return calls


def test_graph_scst_step_with_the_mix():
    """One SCST step as test_gpu_sent_metrics.py::
    test_graph_scst_step_with_sentence_reward defines it: eager warm-up, capture,
    one replay, alongside an eager twin (seeds pinned on the device).  The
    replayed step's samples, rescored, equal the oracle blend, as does the mean
    sample score the step reports."""
    from cst_captioning_amd import _ext
    from cst_captioning_amd.ops import featpool as fp
    from cst_captioning_amd.ops.reward_mix import MixedRewardScorer
    ops = _ext.ops()
    ops.reset_device_errors(0)
    fixed = torch.tensor([12345, 67890], dtype=torch.int32, device=DEV)
    a, la, ds = _trainer(graph=0)
    b, lb, _ = _trainer(graph=1)
    for tr in (a, b):
        tr.engine._rng = lambda dev: fixed
        assert type(tr._ensure_scorer()) is MixedRewardScorer
        assert tr.scorer.backend == 'gpu' and tr.scorer.weights == W
    calls = _count_calls(a.scorer)
    old = fp.SEED_SOURCE
    fp.SEED_SOURCE = lambda dev: fixed
    try:
        for step in range(3):
            da, db = la.get_batch(), lb.get_batch()
            oa = a.train_step(da, 0)
            ob = b.train_step(db, 0)
            torch.cuda.synchronize()
            assert (b._graph is not None) == (step >= 1)
            assert torch.isfinite(ob['loss']).item()
            assert torch.equal(oa['seq'], ob['seq'])
            torch.testing.assert_close(oa['reward'], ob['reward'], rtol=1e-5, atol=1e-6)
            for k in ('loss', 'm', 'b'):
                torch.testing.assert_close(torch.as_tensor(oa[k]).float(),
                                           torch.as_tensor(ob[k]).float(), rtol=1e-5, atol=1e-6)
    finally:
        fp.SEED_SOURCE = old
    assert b._graph is not None and a._graph is None
    # the sampled rows and the per-video greedy rows both went through the scorer
    assert calls in ([80, 4] * 3, [4, 80] * 3), calls
    # the replayed (third) step: its samples rescored, against the oracle blend
    seq = ob['seq']
    vid = db['video_index'].repeat_interleave(20)
    parts = b.scorer.score_parts(seq, vid).cpu().numpy()
    want_parts = b.scorer.parts_reference(seq, vid)
    ref_c = want_parts[:, 0]
    assert np.abs(parts[:, 0] - ref_c).max() < 1e-4 * max(1.0, ref_c.max())
    for col in (1, 2):
        np.testing.assert_allclose(parts[:, col], want_parts[:, col].astype(np.float32),
                                   rtol=sm.RTOL, atol=sm.ATOL)
    want = b.scorer.score_reference(seq, vid)
    got = b.scorer.score(seq, vid).cpu().numpy()
    # (the parts' bounds, weighted, plus the blend's 2^-21)
    tol = (1e-4 * max(1.0, ref_c.max()) + 5 * sm.RTOL * want_parts[:, 1]
           + 5 * sm.RTOL * want_parts[:, 2] + 2.0 ** -20 * want)
    assert (np.abs(got - want) <= tol).all()
    assert (want > 0).any()
    # (fp32 mean of 80 scores in the loss kernel)
    np.testing.assert_allclose(float(ob['m']), want.mean(), rtol=1e-5, atol=1e-8)
    assert ops.device_errors(0) == 0


def test_cst_step_with_the_mix_and_token_consensus():
    """CST with the MIXER schedule and GT consensus baselines (scb_baseline 1,
    --consensus_scorer tokens): the baselines are the weighted sum of the
    token-space consensus scores, the step goes through the fused cst_loss."""
    from cst_captioning_amd.ops import scst_loss as sl
    from cst_captioning_amd.ops.consensus import ConsensusScorer
    tr, loader, ds = _trainer(graph=0, use_cst=1, use_mixer=1, scb_baseline=1, scb_captions=20,
                              consensus_scorer='tokens')
    per = ConsensusScorer(ds, use_eos=1, device=torch.device(DEV)).scores(20, cases.COLS)
    want = sum(w * per[m] for m, w in zip(cases.COLS, W))
    assert np.array_equal(ds.bcmrscores, want) and (want > 0).any()
    assert tr._ensure_scorer().backend == 'gpu'
    calls = _count_calls(tr.scorer)
    seen = []
    inner = sl.cst_loss
    sl.cst_loss = lambda *a, **k: (seen.append(1), inner(*a, **k))[1]
    try:
        out = tr.train_step(loader.get_batch(), 0)
        torch.cuda.synchronize()
    finally:
        sl.cst_loss = inner
    assert torch.isfinite(out['loss']).item()
    assert calls == [80] and seen == [1]
