"""Token-space validation scorer on the GPU: ``bleu_stats_kernel`` and
``meteor_stats_kernel`` (``csrc/kernels/corpus_metrics.hip``), ``rouge_l_kernel``
and the unclipped CIDEr kernel against the oracle (``backend='cpu-ref'``) and
against the native CPU twins, and ``Trainer.validate`` with the fused engine
and ``--val_scorer tokens``.  Cases and bounds: ``corpus_metric_cases.py``.
"""
import numpy as np
import pytest
import torch

import corpus_metric_cases as cases

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _scorer(ds, backend):
    from cst_captioning_amd.ops.corpus_metrics import CorpusScorer
    return CorpusScorer(ds, torch.device(DEV), backend)


@pytest.mark.parametrize('nv', cases.SIZES)
def test_gpu_matches_oracle_and_cpu(nv):
    """N = 1, 13 (the last block is partial) and 24; 70 references pass one
    wavefront's width in the reference loops.  Against the oracle with the
    bounds of the CPU test; the integer statistics equal the CPU twin's; two
    launches are identical."""
    ds, seqs, vi = cases.make_case(nv)
    sc = _scorer(ds, 'auto')
    assert sc.backend == 'gpu'
    h, v = torch.from_numpy(seqs.copy()).to(DEV), torch.from_numpy(vi.copy()).to(DEV)
    got = sc.score(h, v)
    again = sc.score(h, v)
    cases.check_against_oracle(got, nv)
    cpu = _scorer(ds, 'cpu').score(h, v)
    for k in ('bleu_stats', 'meteor_stats'):
        assert np.array_equal(got['segments'][k], cpu['segments'][k]), k
        assert np.array_equal(got['segments'][k], again['segments'][k]), k
    for k in ('METEOR', 'ROUGE_L', 'CIDEr'):
        assert np.array_equal(got['segments'][k], again['segments'][k]), k
    np.testing.assert_allclose(got['segments']['METEOR'], cpu['segments']['METEOR'], rtol=1e-9,
                               atol=0)


def test_gpu_errors():
    ds, seqs, vi = cases.make_case(13)
    sc = _scorer(ds, 'gpu')
    with pytest.raises(ValueError):
        sc.score(torch.zeros(13, 65, dtype=torch.long, device=DEV), torch.from_numpy(vi.copy()))
    with pytest.raises(ValueError):
        sc.score(torch.from_numpy(seqs[:12].copy()).to(DEV), torch.from_numpy(vi[:12].copy()))
    dup = vi.copy()
    dup[0] = dup[1]
    with pytest.raises(ValueError):
        sc.score(torch.from_numpy(seqs.copy()).to(DEV), torch.from_numpy(dup))


def test_trainer_validate_tokens_fused_engine():
    """Beam-5 validation of a 24-video split through the fused engine: the
    reported scores are the oracle's scores of the returned sequences, and the
    predictions are those sequences decoded."""
    from cst_captioning_amd.cli import build_model
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import CaptionLoader, make_synthetic
    from cst_captioning_amd.ops.corpus_metrics import KEYS, CorpusScorer
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.train.trainer import Trainer
    from cst_captioning_amd.utils.text import decode_sequence
    ds = make_synthetic('msrvtt', num_videos=24, vocab_size=500, seq_length=12,
                        feat_dims=[64, 32], seed=0)
    opt = default_opts(batch_size=8, train_seq_per_img=5, test_batch_size=10, test_seq_per_img=5,
                       rnn_size=128, input_encoding_size=128, beam_size=5, impl='hip',
                       drop_prob_lm=0.5, val_scorer='tokens', vocab_size=ds.vocab_size,
                       seq_length=ds.seq_length, feat_dims=ds.feat_dims)
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    torch.manual_seed(0)
    dev = torch.device(DEV)
    model, engine = build_model(opt, dev, 'hip')
    assert engine is not None
    train = CaptionLoader(ds, 8, 5, 'train', dev, seed=0)
    val = CaptionLoader(ds, 10, 5, 'test', dev)
    tr = Trainer(opt, model, train, val, DistContext(device=dev), engine)
    res = tr.validate(val)
    assert tr.corpus_scorer(val).backend == 'gpu'
    seqs, vi = res['sequences'], res['video_index']
    assert seqs.shape[0] == 24 and sorted(vi.tolist()) == list(range(24))
    ref = CorpusScorer(ds, 'cpu', 'cpu-ref').score(seqs, vi)
    for k in KEYS:
        assert res['scores'][k] == round(ref['scores'][k], 5), (k, res['scores'][k],
                                                                ref['scores'][k])
    sents = decode_sequence(ds.ix_to_word, seqs)
    assert [p['caption'] for p in res['predictions']] == sents
    assert [p['image_id'] for p in res['predictions']] == ds.video_ids[vi].tolist()
    assert np.isfinite(res['scores']['Loss'])
