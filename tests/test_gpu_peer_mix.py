"""Consensus (MBR) decoding under a mixed utility on the GPU:
``csrc/kernels/peer_mix.hip`` against the fp64 oracles and, bit for bit, against
the table kernels with leave-one-out; its limits, determinism, zero weights and
selection; ``sample_mbr`` and ``Trainer.validate --decode mbr --mbr_mix`` on the
fused engine."""
import math

import numpy as np
import pytest
import torch

import mbr_cases as mc
import peer_mix_cases as pc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CASES = pc.cases()
IDS = pc.case_ids()


def _scorer(use_eos, weights=pc.WEIGHTS, backend='gpu', df=True):
    from cst_captioning_amd.ops.mbr import PeerMix
    return PeerMix(mc.df_table() if df else None, weights, use_eos=use_eos, device=DEV,
                   backend=backend)


def _check_blend(out, parts, weights=pc.WEIGHTS):
    """|out - parts . w| <= 2^-21 (parts . w): three products and two sums of
    non-negative terms, each rounded once to fp32 (relative error below
    (1 + 2^-24)^3 - 1 < 2^-22), against the fp64 sum of the fp32 columns."""
    want = pc.blend(parts, weights)
    assert (np.abs(out.astype(np.float64) - want) <= 2.0 ** -21 * want).all()


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_kernel_matches_oracle(case):
    ref = pc.oracle(case)
    sc = _scorer(case.use_eos)
    h = torch.from_numpy(case.hyps).to(DEV)
    out, parts = sc.score_both(h, case.G)
    assert out.is_cuda and parts.is_cuda
    assert out.dtype == torch.float32 and parts.dtype == torch.float32
    assert out.shape == (len(case.hyps),) and parts.shape == (len(case.hyps), 3)
    out, parts = out.cpu().numpy(), parts.cpu().numpy()
    pc.check_parts(parts, ref)
    _check_blend(out, parts)
    # information: the CIDEr-D column beside the CIDEr-D peer kernel's
    from cst_captioning_amd.ops.mbr import PeerCiderD
    peer = PeerCiderD(mc.df_table(), use_eos=case.use_eos, device=DEV).score(h, case.G)
    peer = peer.cpu().numpy()
    print(case.name, 'CIDEr-D column vs cider_score(group): max diff %.3g, %d of %d rows bit-equal'
          % (np.abs(parts[:, 0] - peer).max(), int((parts[:, 0] == peer).sum()), len(peer)))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_kernel_is_bit_equal_to_the_table_kernels(case):
    """BLEU-4 / ROUGE-L against bleu4_kernel / rouge_l_kernel on
    ``metric_build_tables`` of the pool rows with ``exclude = i mod G``: the same
    integers through the same formula code."""
    from cst_captioning_amd import _ext
    h = torch.from_numpy(case.hyps).to(DEV)
    parts = _scorer(case.use_eos).score_parts(h, case.G).cpu().numpy()
    tab = pc.table_columns(_ext.ops().metric_score, case.hyps, case.G, case.use_eos, DEV)
    assert np.array_equal(parts[:, 1], tab['Bleu_4'])
    assert np.array_equal(parts[:, 2], tab['ROUGE_L'])


@pytest.mark.parametrize('G,T', [(64, 31), (32, 63)])
@pytest.mark.parametrize('use_eos', [0, 1])
def test_kernel_at_the_lds_limits(G, T, use_eos):
    hyps = pc.limit_pools(G, T, 5 + G)
    ref = pc.oracle_parts(hyps, G, use_eos)
    sc = _scorer(use_eos)
    h = torch.from_numpy(hyps).to(DEV)
    out, parts = sc.score_both(h, G)
    pc.check_parts(parts.cpu().numpy(), ref)
    _check_blend(out.cpu().numpy(), parts.cpu().numpy())
    out2, parts2 = sc.score_both(h, G)
    assert torch.equal(out, out2) and torch.equal(parts, parts2)


def test_two_calls_are_bit_equal():
    for case in CASES:
        sc = _scorer(case.use_eos)
        h = torch.from_numpy(case.hyps).to(DEV)
        a, b = sc.score_both(h, case.G), sc.score_both(h, case.G)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), case.name


def test_bad_inputs_raise_without_launching():
    from cst_captioning_amd import _ext
    from cst_captioning_amd.ops.mbr import df_hash_table
    keys, vals, ref_len = mc.df_table()
    t = {k: v.to(DEV) for k, v in df_hash_table(keys, vals).items()}
    lrl = math.log(ref_len)
    none = torch.zeros(0, dtype=torch.long, device=DEV)
    w = list(pc.WEIGHTS)
    ops = _ext.ops()

    def f(hy, group, weights=w, tables=t, metric='mix', **kw):
        return ops.metric_score(metric, hy, none, None, 0, cider_tables=tables, log_ref_len=lrl,
                                weights=weights, group=group, **kw)

    def hyps(G, T):
        return torch.zeros(2 * G, T, dtype=torch.long, device=DEV)

    for G, T in ((65, 31), (2, 64), (33, 63), (64, 32), (128, 15), (1024, 1)):
        with pytest.raises(RuntimeError, match='limit'):
            f(hyps(G, T), G)
    with pytest.raises(RuntimeError, match='at least 2'):
        f(hyps(1, 8), 1)
    with pytest.raises(RuntimeError, match='whole pools'):
        f(hyps(2, 8)[:3], 2)
    with pytest.raises(RuntimeError, match='exclude'):
        f(hyps(2, 8), 2, exclude=torch.zeros(4, dtype=torch.long, device=DEV))
    with pytest.raises(RuntimeError, match='weights'):
        f(hyps(2, 8), 2, weights=None)
    with pytest.raises(RuntimeError, match='weights'):
        f(hyps(2, 8), 2, weights=[1.0, 5.0])
    with pytest.raises(RuntimeError, match='zero'):
        f(hyps(2, 8), 2, weights=[0.0, 0.0, 0.0])
    with pytest.raises(RuntimeError, match='negative'):
        f(hyps(2, 8), 2, weights=[1.0, -5.0, 5.0])
    with pytest.raises(RuntimeError, match='df tables'):
        f(hyps(2, 8), 2, tables=None)
    with pytest.raises(RuntimeError, match='metric mix'):
        f(hyps(2, 8), 2, metric='ROUGE_L')
    with pytest.raises(RuntimeError):  # host tensors: the hypotheses, the df table
        f(hyps(2, 8).cpu(), 2)
    with pytest.raises(RuntimeError):
        f(hyps(2, 8), 2, tables=df_hash_table(keys, vals))
    torch.cuda.synchronize()
    for G, T in ((64, 31), (32, 63)):
        out, parts = f(hyps(G, T), G)
        assert out.shape == (2 * G,) and parts.shape == (2 * G, 3)
    torch.cuda.synchronize()


def test_zero_weights():
    from cst_captioning_amd.ops.mbr import PeerCiderD
    for name in ('rand_G5_B3_eos1', 'rand_G21_B7_eos0', 'edge_eos0'):
        case = CASES[IDS.index(name)]
        h = torch.from_numpy(case.hyps).to(DEV)
        full = _scorer(case.use_eos).score_parts(h, case.G)
        # no CIDEr-D: no df table at all
        sc = _scorer(case.use_eos, (0.0, 5.0, 5.0), df=False)
        assert sc._tables is None
        out, parts = sc.score_both(h, case.G)
        assert not parts[:, 0].any() and torch.equal(parts[:, 1:], full[:, 1:])
        pc.check_parts(parts.cpu().numpy(), pc.oracle(case), (0.0, 5.0, 5.0))
        _check_blend(out.cpu().numpy(), parts.cpu().numpy(), (0.0, 5.0, 5.0))
        # one metric alone: out = fl(w * column), the other columns exactly 0
        for w, col in (((3.0, 0.0, 0.0), 0), ((0.0, 0.3, 0.0), 1), ((0.0, 0.0, 0.7), 2)):
            out, parts = _scorer(case.use_eos, w, df=bool(w[0])).score_both(h, case.G)
            assert torch.equal(parts[:, col], full[:, col])
            assert not parts[:, [c for c in range(3) if c != col]].any()
            assert torch.equal(out, torch.tensor(w[col], dtype=torch.float32, device=DEV)
                               * parts[:, col])
        peer = PeerCiderD(mc.df_table(), use_eos=case.use_eos, device=DEV).score(h, case.G)
        got = _scorer(case.use_eos, (1.0, 0.0, 0.0)).score(h, case.G)
        assert np.abs((got - peer).cpu().numpy()).max() < mc.tolerance(peer.cpu().numpy())


def test_selection():
    """The oracle score of the kernel's choice is within the tolerance of the
    oracle's maximum (exact duplicates and near-ties make index equality the
    wrong test); the hand-made pools match by index."""
    for case in CASES:
        ref = pc.blend(pc.oracle(case)).reshape(-1, case.G)
        best, scores = _scorer(case.use_eos).select(torch.from_numpy(case.hyps).to(DEV), case.G)
        assert best.is_cuda and best.dtype == torch.long and scores.shape == ref.shape
        b = best.cpu().numpy()
        assert ((b >= 0) & (b < case.G)).all()
        chosen = ref[np.arange(len(b)), b]
        assert (ref.max(1) - chosen < mc.tolerance(ref)).all(), case.name
    h = torch.from_numpy(pc.HAND.hyps).to(DEV)
    assert _scorer(0, (0.0, 0.0, 1.0), df=False).select(h, 4)[0].tolist() == [1]
    assert _scorer(0, (1.0, 0.0, 0.0)).select(h, 4)[0].tolist() == [0]
    for name in ('hand_consensus', 'identical', 'votes'):  # (clear under every metric)
        case = CASES[IDS.index(name)]
        best, _ = _scorer(case.use_eos).select(torch.from_numpy(case.hyps).to(DEV), case.G)
        assert best.tolist() == case.best.tolist(), name


def test_captured_in_a_graph():
    """One launch without host synchronisation: the op replays from a graph."""
    case = CASES[IDS.index('rand_G21_B3_eos1')]
    sc = _scorer(case.use_eos)
    h = torch.from_numpy(case.hyps).to(DEV)
    want = sc.score_both(h, case.G)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = sc.score_both(h, case.G)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# -- fused engine --------------------------------------------------------------------
def _engine_model(C=1, V=200, H=64, B=4, seed=0):
    """The model set-up of test_gpu_mbr._engine_model."""
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
    from cst_captioning_amd.ops.mbr import PeerMix
    ds, opt, model, engine, loader = _engine_model(C)
    feats = loader.get_batch_at(0)['feats']
    scorer = PeerMix(ds.df, pc.WEIGHTS, use_eos=1, device=DEV)
    assert scorer.backend == 'gpu'
    o = {'decode': 'mbr', 'beam_size': 3, 'mbr_samples': 5, 'mbr_temperature': 1.0,
         'mbr_scorer': scorer}
    torch.manual_seed(5)
    seq, lp, info = model.sample_mbr(feats, o)
    pool, scores, best = info['pool'], info['scores'], info['best']
    B, G, T = pool.shape
    assert (B, G) == (4, 6) and seq.shape == (B, T) and lp.shape == (B, T)
    beam, _ = model.sample_beam(feats, {'beam_size': 3})
    w = beam.size(1)
    assert torch.equal(pool[:, 0, :w], beam) and not pool[:, 0, w:].any()
    assert torch.equal(seq, pool[torch.arange(B, device=DEV), best])
    # scores and selection against the oracle on the returned pool
    ref = scorer.score_reference(pool.reshape(B * G, T).cpu(), G).reshape(B, G)
    assert np.abs(scores.cpu().numpy() - ref).max() < mc.tolerance(ref)
    b = best.cpu().numpy()
    assert (ref.max(1) - ref[np.arange(B), b] < mc.tolerance(ref)).all()
    torch.manual_seed(5)
    assert torch.equal(model.sample_mbr(feats, o)[2]['pool'], pool)


def test_trainer_validate_mbr_mix_tokens_fused_engine():
    from cst_captioning_amd.ops.corpus_metrics import KEYS, CorpusScorer
    from cst_captioning_amd.ops.mbr import PeerMix
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.data import CaptionLoader
    from cst_captioning_amd.train.trainer import Trainer
    from cst_captioning_amd.utils.text import decode_sequence
    ds, opt, model, engine, val = _engine_model(1)
    opt.val_scorer, opt.decode, opt.mbr_samples, opt.mbr_temperature = 'tokens', 'mbr', 5, 1.0
    opt.mbr_mix = 'CIDEr:1,Bleu_4:5,ROUGE_L:5'
    opt.test_batch_size, opt.test_seq_per_img, opt.batch_size = 4, 5, 4
    dev = torch.device(DEV)
    train = CaptionLoader(ds, 4, 5, 'train', dev, seed=0)
    tr = Trainer(opt, model, train, val, DistContext(device=dev), engine)
    assert isinstance(tr.mbr_scorer, PeerMix) and tr.mbr_scorer.backend == 'gpu'
    assert tr.mbr_scorer.weights == (1.0, 5.0, 5.0)
    res = tr.validate(val)
    seqs, vi = res['sequences'], res['video_index']
    assert seqs.shape[0] == 12 and sorted(vi.tolist()) == list(range(12))
    ref = CorpusScorer(ds, 'cpu', 'cpu-ref').score(seqs, vi)
    for k in KEYS:
        assert res['scores'][k] == round(ref['scores'][k], 5), k
    assert [p['caption'] for p in res['predictions']] == decode_sequence(ds.ix_to_word, seqs)
    assert all(0.0 <= p['mbr_score'] <= 20.0001 for p in res['predictions'])
    assert any(p['mbr_score'] > 0 for p in res['predictions'])
