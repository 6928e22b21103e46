"""Sentence BLEU-4 / ROUGE-L rewards on the GPU: ``bleu4_kernel`` and
``rouge_l_kernel`` (``csrc/kernels/sent_metrics.hip``) against
``eval/metrics.py`` called directly, and the RL training steps that use them
(``--eval_metric Bleu_4 | ROUGE_L``: captured SCST step, CST step) plus the
capture guard for host-scored rewards (METEOR).
Inputs, oracle and tolerance: tests/sent_metric_cases.py.
"""
import numpy as np
import pytest
import torch

import sent_metric_cases as cases

pytestmark = pytest.mark.gpu

DEV = 'cuda'
METRICS = ('Bleu_4', 'ROUGE_L')


def _scorer(ds, metric, use_eos, backend='auto'):
    from cst_captioning_amd.ops.sent_metrics import SentenceMetricScorer
    return SentenceMetricScorer(ds, metric, use_eos=use_eos, device=torch.device(DEV),
                                backend=backend)


@pytest.mark.parametrize('use_eos', [0, 1])
@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('case', ['main', 'tiny'])
def test_kernels_match_oracle(case, metric, use_eos):
    """Every hypothesis of the case (N = 250: the last block is partial; 70
    references: the reference loop passes one wavefront) against the oracle;
    two launches are bit-identical; the native CPU scorer agrees within the
    same tolerance (not asserted bit-identical: the device's pow / exp, and
    the fused multiply-adds the device compiler may contract the fp64 ROUGE
    formula into, can differ from the host's in the last fp64 bits)."""
    ds, hyps, vid, _ = getattr(cases, case + '_case')()
    cases.check_not_vacuous(use_eos)
    sc = _scorer(ds, metric, use_eos)
    assert sc.backend == 'gpu'
    h, v = torch.from_numpy(hyps).to(DEV), torch.from_numpy(vid).to(DEV)
    got = sc.score(h, v)
    again = sc.score(h, v)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.device.type == 'cuda'
    cases.check(got.cpu().numpy(), case, metric, use_eos)
    assert torch.equal(got, again)
    cpu = _scorer(ds, metric, use_eos, backend='cpu').score(h, v)
    np.testing.assert_allclose(got.cpu().numpy(), cpu.cpu().numpy(), rtol=cases.RTOL,
                               atol=cases.ATOL)


def test_gpu_entry_rejects_over_limit_width():
    ds, hyps, vid, _ = cases.main_case()
    sc = _scorer(ds, 'ROUGE_L', 0)
    with pytest.raises(RuntimeError, match='at most 64'):
        sc.score(torch.full((2, 65), 5, device=DEV), torch.zeros(2, dtype=torch.long, device=DEV))


def _trainer(metric, graph, big=True, **kw):
    """The smoke() shape (4 videos x 20 captions, V = 1000, H = 512), or the
    small shape of test_gpu_graph.py."""
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import make_synthetic, CaptionLoader
    from cst_captioning_amd.cli import build_model
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.train.trainer import Trainer
    if big:
        B, S, H = 4, 20, 512
        ds = make_synthetic('msrvtt', num_videos=64, vocab_size=1000, seed=0)
    else:
        B, S, H = 8, 5, 128
        ds = make_synthetic('msrvtt', num_videos=48, vocab_size=500, seq_length=12,
                            feat_dims=[64, 32], seed=0)
    args = dict(batch_size=B, train_seq_per_img=S, rnn_size=H, input_encoding_size=H,
                drop_prob_lm=0.5, use_rl=1, use_rl_after=0, use_cst=0, use_mixer=1, mixer_from=1,
                use_eos=1, impl='hip', cuda_graph=graph, learning_rate=1e-3, eval_metric=metric,
                vocab_size=ds.vocab_size, seq_length=ds.seq_length, feat_dims=ds.feat_dims)
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


@pytest.mark.parametrize('metric', METRICS)
def test_graph_scst_step_with_sentence_reward(metric):
    """One SCST step per metric as test_gpu_graph.py::
    test_graph_scst_step_matches_eager_with_fixed_seeds defines it (same
    sampled tokens, rewards / loss / means within rtol 1e-5, atol 1e-6 of the
    eagerly enqueued step, seeds pinned on the device): eager warm-up,
    capture, one replay.  The replayed step's samples are scored again and
    must equal the oracle, as must the mean sample score the step reports."""
    from cst_captioning_amd import _ext
    from cst_captioning_amd.ops import featpool as fp
    from cst_captioning_amd.ops.sent_metrics import SentenceMetricScorer
    ops = _ext.ops()
    ops.reset_device_errors(0)
    fixed = torch.tensor([12345, 67890], dtype=torch.int32, device=DEV)
    a, la, ds = _trainer(metric, graph=0)
    b, lb, _ = _trainer(metric, graph=1)
    for tr in (a, b):
        tr.engine._rng = lambda dev: fixed
        assert isinstance(tr._ensure_scorer(), SentenceMetricScorer)
        assert tr.scorer.backend == 'gpu' and tr.scorer.metric == metric
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
    # the replayed (third) step: scores of its samples against the oracle
    seq = ob['seq']
    vid = db['video_index'].repeat_interleave(20)
    got = b.scorer.score(seq, vid).cpu().numpy()
    want = cases.direct_oracle(ds, seq.cpu().numpy(), vid.cpu().numpy(), metric, 1)
    np.testing.assert_allclose(got, want.astype(np.float32), rtol=cases.RTOL, atol=cases.ATOL)
    assert (want > 0).any()
    # (fp32 mean of 80 scores in the loss kernel)
    np.testing.assert_allclose(float(ob['m']), want.mean(), rtol=1e-5, atol=1e-8)
    assert ops.device_errors(0) == 0


def test_cst_step_with_rouge_reward():
    """CST with the MIXER schedule and the self-consensus baseline scores the
    samples with the new scorer and goes through the fused cst_loss."""
    from cst_captioning_amd.ops import scst_loss as sl
    tr, loader, ds = _trainer('ROUGE_L', graph=0, use_cst=1, use_mixer=1, scb_baseline=2,
                              scb_captions=20)
    assert tr._ensure_scorer().backend == 'gpu' and tr.scorer.metric == 'ROUGE_L'
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


def test_meteor_reward_runs_eagerly_with_the_engine():
    """METEOR is scored on the host: the RL step must not be captured."""
    from cst_captioning_amd.ops.cider_d import GenericScorer
    tr, loader, _ = _trainer('METEOR', graph=1, big=False)
    for _ in range(2):
        out = tr.train_step(loader.get_batch(), 0)
        torch.cuda.synchronize()
        assert torch.isfinite(out['loss']).item()
    assert isinstance(tr.scorer, GenericScorer) and tr.scorer.backend == 'cpu-ref'
    assert tr._graph is None
