"""Sentence BLEU-4 / ROUGE-L rewards on the CPU: the native C++ scorer
(``csrc/host/metric_host.cpp``, the tables the GPU kernels read) and the
Python reward path (``score_hypotheses`` with the coco-style scorers,
``build_scorer`` dispatch) against ``eval/metrics.py`` called directly.
Inputs, oracle and tolerance: tests/sent_metric_cases.py.
"""
import numpy as np
import pytest
import torch

import sent_metric_cases as cases
from cst_captioning_amd import _ext
from cst_captioning_amd.eval.metrics import Bleu, Meteor, Rouge
from cst_captioning_amd.reward.rewards import score_hypotheses
from cst_captioning_amd.utils.text import array_to_str

METRICS = ('Bleu_4', 'ROUGE_L')


def _need_ext():
    if not _ext.host_available():
        pytest.skip('native extension not built')


def _tables(ds, use_eos):
    return _ext.ops().metric_build_tables(torch.from_numpy(ds.labels),
                                          torch.from_numpy(ds.label_start_ix),
                                          torch.from_numpy(ds.label_end_ix), use_eos)


@pytest.mark.parametrize('use_eos', [0, 1])
def test_generator_is_not_vacuous(use_eos):
    cases.check_not_vacuous(use_eos)


@pytest.mark.parametrize('use_eos', [0, 1])
@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('case', ['main', 'tiny'])
def test_native_cpu_scorer_matches_oracle(case, metric, use_eos):
    _need_ext()
    ds, hyps, vid, _ = getattr(cases, case + '_case')()
    got = _ext.ops().metric_score_cpu(metric, torch.from_numpy(hyps), torch.from_numpy(vid),
                                      _tables(ds, use_eos), use_eos)
    cases.check(got.numpy(), case, metric, use_eos)


@pytest.mark.parametrize('use_eos', [0, 1])
@pytest.mark.parametrize('metric', METRICS)
def test_scorer_class_cpu_backend_matches_oracle(metric, use_eos):
    _need_ext()
    from cst_captioning_amd.ops.sent_metrics import SentenceMetricScorer
    ds, hyps, vid, _ = cases.main_case()
    sc = SentenceMetricScorer(ds, metric, use_eos=use_eos, device='cpu', backend='cpu')
    assert sc.backend == 'cpu'
    got = sc.score(torch.from_numpy(hyps), torch.from_numpy(vid))
    assert got.dtype == torch.float32 and got.device.type == 'cpu'
    cases.check(got.numpy(), 'main', metric, use_eos)
    # the Python oracle path of the class is the direct call
    ref = sc.score_reference(torch.from_numpy(hyps[:40]), torch.from_numpy(vid[:40]))
    np.testing.assert_array_equal(ref, cases.oracle('main', metric, use_eos)[:40])
    auto = SentenceMetricScorer(ds, metric, use_eos=use_eos, device='cpu')
    assert auto.backend == 'cpu'
    with pytest.raises(ValueError):
        SentenceMetricScorer(ds, 'METEOR')


@pytest.mark.parametrize('use_eos', [0, 1])
def test_score_hypotheses_with_coco_style_scorers(use_eos):
    """Bleu / Rouge / Meteor take res as {i: [str]}; score_hypotheses used to
    hand them CiderD's list form and raise TypeError."""
    ds, hyps, vid, _ = cases.main_case()
    sel = np.arange(0, len(hyps), 7)
    h, v = hyps[sel], vid[sel]
    gts = [ds.gts_of(int(x)) for x in v]
    res = {i: [array_to_str(r, use_eos)] for i, r in enumerate(h)}
    gmap = {i: [array_to_str(r, use_eos) for r in g] for i, g in enumerate(gts)}
    for scorer, direct in ((Bleu(4), lambda: Bleu(4).compute_score(gmap, res)[1][-1]),
                           (Rouge(), lambda: Rouge().compute_score(gmap, res)[1]),
                           (Meteor(), lambda: Meteor().compute_score(gmap, res)[1])):
        got = score_hypotheses(scorer, h, gts, seq_per_img=1, expand_feat=1, use_eos=use_eos)
        assert got.shape == (len(sel),) and got.dtype == np.float64
        np.testing.assert_array_equal(got, np.asarray(direct(), dtype=np.float64))
    np.testing.assert_array_equal(
        score_hypotheses(Bleu(4), h, gts, 1, 1, use_eos),
        cases.oracle('main', 'Bleu_4', use_eos)[sel])


@pytest.mark.parametrize('reward_device,backend', [('gpu', 'cpu'), ('cpu', 'cpu-ref')])
def test_build_scorer_dispatch_on_cpu(reward_device, backend):
    _need_ext()
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.ops.cider_d import GenericScorer
    from cst_captioning_amd.ops.sent_metrics import SentenceMetricScorer
    from cst_captioning_amd.train.trainer import build_scorer
    ds, hyps, vid, _ = cases.main_case()
    opt = default_opts(eval_metric='ROUGE_L', use_eos=1, reward_device=reward_device)
    sc = build_scorer(opt, ds, torch.device('cpu'))
    assert isinstance(sc, SentenceMetricScorer) and sc.metric == 'ROUGE_L'
    assert sc.backend == backend
    n = len(hyps) if backend == 'cpu' else 60  # (the Python scorer: a slice is enough)
    got = sc.score(torch.from_numpy(hyps[:n]), torch.from_numpy(vid[:n])).numpy()
    want = cases.oracle('main', 'ROUGE_L', 1)[:n].astype(np.float32)
    np.testing.assert_allclose(got, want, rtol=cases.RTOL, atol=cases.ATOL)
    opt.eval_metric = 'Bleu_4'
    assert build_scorer(opt, ds, torch.device('cpu')).metric == 'Bleu_4'
    opt.eval_metric = 'METEOR'
    assert isinstance(build_scorer(opt, ds, torch.device('cpu')), GenericScorer)


def test_over_limit_inputs_raise():
    _need_ext()
    ops = _ext.ops()
    ds, hyps, vid, _ = cases.main_case()
    t = _tables(ds, 0)
    v1 = torch.zeros(1, dtype=torch.long)
    for metric in METRICS:  # T = 65
        with pytest.raises(ValueError, match='at most 64'):
            ops.metric_score_cpu(metric, torch.full((1, 65), 5, dtype=torch.long), v1, t, 0)
    big = torch.tensor([[5, 70000, 6, 0]])
    with pytest.raises(ValueError, match='65534'):
        ops.metric_score_cpu('Bleu_4', big, v1, t, 0)
    assert ops.metric_score_cpu('ROUGE_L', big, v1, t, 0).shape == (1,)  # no packing there
    with pytest.raises(ValueError, match='outside the tables'):
        ops.metric_score_cpu('ROUGE_L', big, torch.tensor([4]), t, 0)
    with pytest.raises(RuntimeError, match='Bleu_4 or ROUGE_L'):
        ops.metric_score_cpu('METEOR', big, v1, t, 0)
    # references: longer than 64 tokens, and a token the packing cannot hold
    one = torch.tensor([0]), torch.tensor([1])
    with pytest.raises(ValueError, match='at most 64'):
        ops.metric_build_tables(torch.full((1, 66), 7, dtype=torch.long), one[0], one[1], 0)
    with pytest.raises(ValueError, match='65534'):
        ops.metric_build_tables(torch.tensor([[1, 5, 70000, 0]]), one[0], one[1], 0)
    # 64 tokens + the kept EOS = 65 with use_eos
    row = torch.cat([torch.full((1, 64), 7, dtype=torch.long), torch.zeros(1, 1, dtype=torch.long)], 1)
    ops.metric_build_tables(row, one[0], one[1], 0)
    with pytest.raises(ValueError, match='at most 64'):
        ops.metric_build_tables(row, one[0], one[1], 1)
