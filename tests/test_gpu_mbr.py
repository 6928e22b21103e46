"""Consensus (MBR) decoding on the GPU: ``csrc/kernels/cider_pairwise.hip``
against the fp64 oracle and against the merged reference-table kernel with
leave-one-out, its limits, determinism and selection; ``sample_mbr`` and
``Trainer.validate --decode mbr`` on the fused engine."""
import math

import numpy as np
import pytest
import torch

import mbr_cases as mc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CASES = mc.cases()


def _scorer(use_eos, backend='gpu'):
    from cst_captioning_amd.ops.mbr import PeerCiderD
    return PeerCiderD(mc.df_table(), use_eos=use_eos, device=DEV, backend=backend)


def _limit_pools(G, T, seed):
    """Two pools at an LDS limit: full-width rows without EOS among them."""
    hyps = mc._random_pools(seed, 2, G, T, 60)
    hyps[0] = np.arange(3, 3 + T)  # full width, no EOS, all distinct
    hyps[1] = 5                     # full width, one token: tf = T
    return hyps


@pytest.mark.parametrize('case', CASES, ids=mc.case_ids())
def test_kernel_matches_oracle(case):
    ref = mc.oracle(case)
    got = _scorer(case.use_eos).score(torch.from_numpy(case.hyps).to(DEV), case.G)
    assert got.is_cuda and got.dtype == torch.float32
    err = np.abs(got.cpu().numpy() - ref).max()
    print(case.name, 'max err %.3g of %.3g' % (err, ref.max()))
    assert err < mc.tolerance(ref)


@pytest.mark.parametrize('G,T', [(64, 31), (32, 63)])
@pytest.mark.parametrize('use_eos', [0, 1])
def test_kernel_at_the_lds_limits(G, T, use_eos):
    hyps = _limit_pools(G, T, 5 + G)
    ref = mc.oracle_scores(hyps, G, use_eos)
    sc = _scorer(use_eos)
    h = torch.from_numpy(hyps).to(DEV)
    got = sc.score(h, G)
    err = np.abs(got.cpu().numpy() - ref).max()
    print(G, T, use_eos, 'max err %.3g of %.3g' % (err, ref.max()))
    assert err < mc.tolerance(ref)
    assert torch.equal(got, sc.score(h, G))


@pytest.mark.parametrize('case', CASES, ids=mc.case_ids())
def test_kernel_matches_reference_table_kernel(case):
    """The second, already trusted reference: the pool rows as a reference
    table, ``cider_score`` with ``exclude = i mod G``."""
    from cst_captioning_amd import _ext
    keys, vals, ref_len = mc.df_table()
    N, G = len(case.hyps), case.G
    lab = torch.from_numpy(case.hyps)
    st = torch.arange(0, N, G)
    lrl = math.log(ref_len)
    t = _ext.ops().cider_build_tables(lab, st, st + G, torch.from_numpy(keys.view(np.int64)),
                                      torch.from_numpy(vals), lrl, case.use_eos)
    t = {k: v.to(DEV) for k, v in t.items()}
    i = torch.arange(N, device=DEV)
    want = _ext.ops().cider_score(lab.to(DEV), i // G, t, lrl, case.use_eos, exclude=i % G)
    got = _ext.ops().cider_score(lab.to(DEV), i // G, t, lrl, case.use_eos, group=G)
    want, got = want.cpu().numpy(), got.cpu().numpy()
    assert np.abs(got - want).max() < mc.tolerance(want)
    # group = 0 is the call without the keyword, bit for bit
    a = _ext.ops().cider_score(lab.to(DEV), i // G, t, lrl, case.use_eos, exclude=i % G, group=0)
    assert np.array_equal(a.cpu().numpy(), want)


def test_two_calls_are_bit_equal():
    for case in CASES:
        sc = _scorer(case.use_eos)
        h = torch.from_numpy(case.hyps).to(DEV)
        assert torch.equal(sc.score(h, case.G), sc.score(h, case.G)), case.name


def test_selection():
    """The oracle score of the kernel's choice is within the tolerance of the
    oracle's maximum (exact duplicates and near-ties make index equality the
    wrong test); the hand-made pools match by index."""
    for case in CASES:
        ref = mc.oracle(case).reshape(-1, case.G)
        best, scores = _scorer(case.use_eos).select(torch.from_numpy(case.hyps).to(DEV), case.G)
        assert best.is_cuda and best.dtype == torch.long and scores.shape == ref.shape
        b = best.cpu().numpy()
        assert ((b >= 0) & (b < case.G)).all()
        chosen = ref[np.arange(len(b)), b]
        assert (ref.max(1) - chosen < mc.tolerance(ref)).all(), case.name
        if case.best is not None:
            assert b.tolist() == case.best.tolist(), case.name


def test_over_limit_raises_without_launching():
    from cst_captioning_amd import _ext
    from cst_captioning_amd.ops.mbr import df_hash_table
    keys, vals, ref_len = mc.df_table()
    t = {k: v.to(DEV) for k, v in df_hash_table(keys, vals).items()}
    lrl = math.log(ref_len)
    none = torch.zeros(0, dtype=torch.long, device=DEV)
    f = _ext.ops().cider_score

    def hyps(G, T):
        return torch.zeros(2 * G, T, dtype=torch.long, device=DEV)

    for G, T in ((65, 31), (33, 63), (64, 32), (2, 64), (128, 16), (128, 15), (1024, 1)):
        with pytest.raises(RuntimeError, match='limit'):
            f(hyps(G, T), none, t, lrl, 0, group=G)
    with pytest.raises(RuntimeError, match='at least 2'):
        f(hyps(1, 8), none, t, lrl, 0, group=1)
    with pytest.raises(RuntimeError, match='whole pools'):
        f(hyps(2, 8)[:3], none, t, lrl, 0, group=2)
    with pytest.raises(RuntimeError, match='exclude'):
        f(hyps(2, 8), none, t, lrl, 0, exclude=torch.zeros(4, dtype=torch.long, device=DEV),
          group=2)
    with pytest.raises(RuntimeError, match='clipped'):
        f(hyps(2, 8), none, t, lrl, 0, clipped=False, group=2)
    with pytest.raises(RuntimeError):  # the df table must be on the GPU
        f(hyps(2, 8), none, df_hash_table(keys, vals), lrl, 0, group=2)
    torch.cuda.synchronize()
    assert f(hyps(64, 31), none, t, lrl, 0, group=64).shape == (128,)
    assert f(hyps(32, 63), none, t, lrl, 0, group=32).shape == (64,)
    torch.cuda.synchronize()


# -- fused engine --------------------------------------------------------------------
def _engine_model(C=1, V=200, H=64, B=4, seed=0):
    from cst_captioning_amd.cli import build_model
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import CaptionLoader, make_synthetic
    ds = make_synthetic('msrvtt', num_videos=12, vocab_size=V, seq_length=12, feat_dims=[48, 32],
                        num_chunks=C, seed=seed)
    opt = default_opts(vocab_size=ds.vocab_size, seq_length=ds.seq_length, feat_dims=ds.feat_dims,
                       train_seq_per_img=5, rnn_size=H, input_encoding_size=H, drop_prob_lm=0.0,
                       num_chunks=C, impl='hip', beam_size=3)
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    torch.manual_seed(seed)
    dev = torch.device(DEV)
    model, engine = build_model(opt, dev, 'hip')
    assert engine is not None, 'fused HIP engine not used'
    with torch.no_grad():  # a decoder that says something
        model.logit.weight.mul_(3.0)
    engine.refresh_weights()
    model.eval()
    loader = CaptionLoader(ds, B, 5, 'test', dev)
    return ds, opt, model, engine, loader


@pytest.mark.parametrize('C', [1, 4], ids=['lstm', 'temporal_att'])
def test_sample_mbr_fused_engine(C):
    from cst_captioning_amd.ops.mbr import PeerCiderD
    ds, opt, model, engine, loader = _engine_model(C)
    feats = loader.get_batch_at(0)['feats']
    scorer = PeerCiderD(ds.df, use_eos=1, device=DEV)
    assert scorer.backend == 'gpu'
    o = {'decode': 'mbr', 'beam_size': 3, 'mbr_samples': 5, 'mbr_temperature': 1.0,
         'mbr_scorer': scorer}
    before = model.seq_per_img
    torch.manual_seed(5)
    seq, lp, info = model.sample_mbr(feats, o)
    assert model.seq_per_img == before
    pool, scores, best = info['pool'], info['scores'], info['best']
    B, G, T = pool.shape
    assert (B, G) == (4, 6) and seq.shape == (B, T) and lp.shape == (B, T)
    beam, _ = model.sample_beam(feats, {'beam_size': 3})
    w = beam.size(1)
    assert torch.equal(pool[:, 0, :w], beam) and not pool[:, 0, w:].any()
    assert torch.equal(seq, pool[torch.arange(B, device=DEV), best])
    # selection against the oracle on the returned pool
    ref = scorer.score_reference(pool.reshape(B * G, T).cpu(), G).reshape(B, G)
    assert np.abs(scores.cpu().numpy() - ref).max() < mc.tolerance(ref)
    b = best.cpu().numpy()
    assert (ref.max(1) - ref[np.arange(B), b] < mc.tolerance(ref)).all()
    # the samples differ from one another somewhere (a degenerate pool proves nothing)
    assert len({tuple(r) for r in pool[:, 1:].reshape(-1, T).cpu().tolist()}) > B
    torch.manual_seed(5)
    assert torch.equal(model.sample_mbr(feats, o)[2]['pool'], pool)


def test_trainer_validate_mbr_tokens_fused_engine():
    from cst_captioning_amd.ops.corpus_metrics import KEYS, CorpusScorer
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.data import CaptionLoader
    from cst_captioning_amd.train.trainer import Trainer
    from cst_captioning_amd.utils.text import decode_sequence
    ds, opt, model, engine, val = _engine_model(1)
    opt.val_scorer, opt.decode, opt.mbr_samples, opt.mbr_temperature = 'tokens', 'mbr', 5, 1.0
    opt.test_batch_size, opt.test_seq_per_img, opt.batch_size = 4, 5, 4
    dev = torch.device(DEV)
    train = CaptionLoader(ds, 4, 5, 'train', dev, seed=0)
    tr = Trainer(opt, model, train, val, DistContext(device=dev), engine)
    assert tr.mbr_scorer.backend == 'gpu'
    res = tr.validate(val)
    seqs, vi = res['sequences'], res['video_index']
    assert seqs.shape[0] == 12 and sorted(vi.tolist()) == list(range(12))
    ref = CorpusScorer(ds, 'cpu', 'cpu-ref').score(seqs, vi)
    for k in KEYS:
        assert res['scores'][k] == round(ref['scores'][k], 5), k
    assert [p['caption'] for p in res['predictions']] == decode_sequence(ds.ix_to_word, seqs)
    assert all(0.0 <= p['mbr_score'] <= 10.0001 for p in res['predictions'])
