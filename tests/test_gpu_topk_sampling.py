"""Truncated (top-k / nucleus) sampling on the GPU:
``csrc/kernels/topk_sample.hip`` through ``vocab_select`` on logits known
exactly (kept set, log-prob, LSE, tie rule, determinism, draw frequencies),
the decode loop of ``beam_search.cpp`` on tiny models of every engine
configuration against a PyTorch twin on bf16-rounded weights, and
``sample_mbr`` / ``Trainer.validate`` with ``mbr_top_k`` on the fused engine."""
import copy
import math

import numpy as np
import pytest
import torch

import topk_sampling_cases as tc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
MARGIN = 1e-3  # least distance of a nucleus cut from the cumulative mass
KS, RS, TAUS, PS = (1, 2, 5, 8), (1, 70, 640), (1.0, 0.7), (1.0, 0.9, 0.5)


def _ext():
    from cst_captioning_amd import _ext
    assert _ext.available(), 'native extension must be built for GPU tests'
    return _ext.ops()


def _rng(a, b):
    return torch.tensor([a, b], dtype=torch.int32, device=DEV)


# -- the kernel through vocab_select ---------------------------------------------------
@pytest.mark.parametrize('layout', tc.LAYOUTS)
@pytest.mark.parametrize('V', [130, 300, 1000])
def test_kernel_on_exact_logits(V, layout):
    """h = e_0, W[:, 0] = x (exact in bf16), b = 0: every row's logits are x.
    V = 130: the last tile has 2 valid columns, fewer than k."""
    C = _ext()
    x = tc.kernel_logits(V, layout, seed=V)
    lse_x = float(torch.logsumexp(torch.from_numpy(x).double(), 0))
    hd, W, b = tc.select_operands(x, max(RS), device=DEV)
    rng, rng2 = _rng(31337, 271828), _rng(31337, 271829)
    order = np.lexsort((np.arange(V), -x.astype(np.float64)))
    checked_seed = 0
    for k in KS:
        for tau in TAUS:
            for p in PS:
                ex = tc.exact_truncated(x, k, p, tau)
                assert ex.margin >= MARGIN, (k, tau, p, ex.margin)
                assert np.array_equal(ex.order, order[:k])
                kept = set(ex.order[:ex.m].tolist())
                for R in RS:
                    tok, lse, lp = C.vocab_select(hd[:R], W, b, rng, 1, tau, 3, k, p)
                    tok2, lse2, lp2 = C.vocab_select(hd[:R], W, b, rng, 1, tau, 3, k, p)
                    tok3 = C.vocab_select(hd[:R], W, b, rng2, 1, tau, 3, k, p)[0]
                    assert tok.shape == (R,) and tok.dtype == torch.int64
                    assert torch.equal(tok, tok2) and torch.equal(lp, lp2) and torch.equal(lse, lse2)
                    t = tok.cpu().numpy()
                    assert set(t.tolist()) <= kept, (k, tau, p, R, set(t.tolist()) - kept)
                    want_lp = x.astype(np.float64)[t] - lse_x
                    assert np.abs(lp.cpu().numpy() - want_lp).max() < 1e-4
                    torch.testing.assert_close(lse.cpu(), torch.full((R,), lse_x), rtol=1e-5,
                                               atol=1e-4)
                    if k == 1:
                        assert (t == order[0]).all()
                    # another seed, other draws: two independent draws differ
                    # with probability 1 - sum q^2; the check applies where
                    # that lies 4 standard deviations of the mean over R rows
                    # above one half
                    qk = ex.probs[ex.probs > 0]
                    differ = 1.0 - float((qk ** 2).sum())
                    if ex.m >= 2 and qk.max() <= 0.5 and differ - 4 * math.sqrt(0.25 / R) > 0.5:
                        assert (tok3.cpu().numpy() != t).mean() > 0.5, (k, tau, p, R)
                        checked_seed += 1
    assert checked_seed >= 4  # (k in {5, 8}, p in {1, 0.9}, R = 640)


def test_kernel_chi_square():
    from scipy.stats import chisquare
    C = _ext()
    V, k, p, tau, R = 1000, 8, 0.9, 0.7, 40000
    x = tc.kernel_logits(V, 'per_tile', seed=5)
    ex = tc.exact_truncated(x, k, p, tau)
    assert ex.margin >= MARGIN and ex.m >= 4
    hd, W, b = tc.select_operands(x, R, device=DEV)
    tok = C.vocab_select(hd, W, b, _rng(7, 99991), 1, tau, 5, k, p)[0].cpu().numpy()
    counts = np.bincount(tok, minlength=V)
    kept = ex.probs > 0
    assert counts[~kept].sum() == 0
    assert (ex.probs[kept] * R >= 5).all()
    stat, pval = chisquare(counts[kept], ex.probs[kept] * R)
    assert pval > 1e-4, (stat, pval)
    # the step and the row key the draw: another step, other draws
    tok_s = C.vocab_select(hd, W, b, _rng(7, 99991), 1, tau, 6, k, p)[0].cpu().numpy()
    assert (tok_s != tok).mean() > 0.5


def test_vocab_select_entry_unchanged_and_refusals():
    C = _ext()
    x = tc.kernel_logits(300, 'one_tile', seed=1)
    hd, W, b = tc.select_operands(x, 70, device=DEV)
    rng = _rng(11, 22)
    before = [C.vocab_select(hd, W, b, rng, 1, 0.7, 3), C.vocab_select(hd, W, b, rng, 2, 1.0, 0)]
    out = C.vocab_select(hd, W, b, rng, 1, 0.7, 3, 5, 0.9)
    assert len(out) == 3
    after = [C.vocab_select(hd, W, b, rng, 1, 0.7, 3), C.vocab_select(hd, W, b, rng, 2, 1.0, 0),
             C.vocab_select(hd, W, b, rng, 1, 0.7, 3, 0, 1.0)]
    for a, bb in zip(before + before[:1], after):
        assert len(a) == len(bb) == 2
        assert torch.equal(a[0], bb[0]) and torch.equal(a[1], bb[1])
    for args in [(9, 1.0), (3, 0.0), (3, 1.5)]:
        with pytest.raises(RuntimeError):
            C.vocab_select(hd, W, b, rng, 1, 1.0, 3, *args)
    with pytest.raises(RuntimeError):
        C.vocab_select(hd, W, b, rng, 2, 1.0, 3, 3, 1.0)  # greedy takes no top_k


# -- the decode loop ---------------------------------------------------------------------
# (rnn_type, model_type, num_layers, num_chunks): the configurations of
# test_gpu_cells.py / test_gpu_attention.py
CONFIGS = [('lstm', 'concat', 1, 1), ('gru', 'concat', 1, 1), ('rnn', 'concat', 1, 1),
           ('lstm', 'concat', 2, 1), ('lstm', 'standard', 1, 1), ('lstm', 'manet', 1, 1),
           ('lstm', 'concat', 1, 4)]
CIDS = ['%s-%s-l%d-c%d' % c for c in CONFIGS]
EOS_BIAS = 0.5


def _tiny(cell, model_type, layers, C, V=300, H=64, S=5, B=24, L=12, seed=1):
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import make_synthetic, CaptionLoader
    from cst_captioning_amd.models import CaptionModel
    from cst_captioning_amd.models.decoder_engine import DecoderEngine
    ds = make_synthetic('msrvtt', num_videos=40, vocab_size=V, seq_length=L,
                        feat_dims=[48, 32], num_chunks=C, seed=seed)
    opt = default_opts(vocab_size=V, seq_length=L, feat_dims=[48, 32], train_seq_per_img=S,
                       rnn_size=H, input_encoding_size=2 * H if model_type == 'standard' else H,
                       drop_prob_lm=0.0, rnn_type=cell, num_chunks=C, model_type=model_type,
                       num_layers=layers)
    torch.manual_seed(seed)
    model = CaptionModel(opt).to(DEV)
    with torch.no_grad():  # a non-trivial decoder with peaked distributions: few near-ties
        model.logit.weight.mul_(9.0)
        model.core.rnn.weight_hh_l0.mul_(2.0)
        model.logit.bias[0] = EOS_BIAS  # rows end at different steps
    eng = DecoderEngine(model, opt)
    eng.refresh_weights()
    model.eval()
    loader = CaptionLoader(ds, B, S, 'train', DEV, seed=seed)
    twin = copy.deepcopy(model)
    twin.impl = 'torch'
    with torch.no_grad():
        for q in twin.parameters():
            q.copy_(q.bfloat16().float())
    return opt, model, eng, twin, loader.get_batch()['feats']


@pytest.mark.parametrize('cfg', CONFIGS, ids=CIDS)
def test_decode_loop_matches_twin(cfg):
    opt, model, eng, twin, feats = _tiny(*cfg)
    B, S, W = 24, 5, opt.seq_length - 2
    # top_k = 1 against the engine's greedy decode
    g_seq, g_lp = eng.sample(model, feats, {'sample_max': 1})
    seq1, lp1 = eng.sample(model, feats, {'sample_max': 0, 'top_k': 1, 'temperature': 0.7})
    assert seq1.shape == g_seq.shape == (B, W) and lp1.shape == (B, W)
    assert seq1.dtype == torch.int64 and lp1.dtype == torch.float32
    same = (seq1 == g_seq).all(1)
    assert same.float().mean().item() >= 0.8, (seq1, g_seq)
    assert ((lp1 - g_lp).abs()[same] < 0.05).all()
    # membership of top_k = 3, top_p = 0.9 under the twin's teacher-forced log-probs
    k, p, tau = 3, 0.9, 1.0
    o = {'sample_max': 0, 'top_k': k, 'top_p': p, 'temperature': tau, 'expand_feat': 1}
    model.set_seq_per_img(S)
    torch.manual_seed(4)
    seq, lp = eng.sample(model, feats, o)
    assert seq.shape == (B * S, W) and lp.shape == (B * S, W)
    pred = tc.teacher_force(twin, feats, seq, S)
    inside, sure, alive, lp_ref = tc.membership(pred, seq, k, p, tau, near=0.05)
    n = pred.size(1)
    # a token outside the twin's kept set is excused only where the twin's own
    # log-probs put a boundary within 0.05 (the bf16 engine and the fp32 twin
    # may then rank or cut differently); at most 5 % of the pairs
    excused = alive & ~inside & ~sure
    wrong = alive & ~inside & sure
    frac = excused.sum().item() / alive.sum().item()
    print(cfg, 'pairs %d, near a boundary %d, excused %d (%.4f), wrong %d' %
          (alive.sum().item(), (alive & ~sure).sum().item(), excused.sum().item(), frac,
           wrong.sum().item()))
    assert alive.sum().item() >= 200
    assert not wrong.any()
    assert frac <= 0.05, frac
    chk = alive & ~excused
    err = (lp[:, :n].double().cpu() - lp_ref).abs()[chk]
    print(cfg, 'max |lp - twin lp| %.4f' % err.max().item())
    assert err.max().item() < 0.05
    # the rows do not all agree with each other: the sampler samples
    assert len({tuple(r) for r in seq.cpu().tolist()}) > B
    # rows that ended are zero to the full width
    sc = seq.cpu()
    ended = torch.cumprod((sc > 0).long(), 1) == 0
    assert ended.any() and not sc[ended].any()
    # the same seeds, the same bits; top_k = 0 is the call without the keys
    torch.manual_seed(4)
    seq_b, lp_b = eng.sample(model, feats, o)
    assert torch.equal(seq, seq_b) and torch.equal(lp, lp_b)
    plain = {'sample_max': 0, 'temperature': 0.8, 'expand_feat': 1}
    torch.manual_seed(6)
    a = eng.sample(model, feats, plain)
    torch.manual_seed(6)
    bb = eng.sample(model, feats, dict(plain, top_k=0, top_p=1.0))
    assert torch.equal(a[0], bb[0]) and torch.equal(a[1], bb[1])


def test_decode_loop_top_k_over_8_takes_the_torch_path(caplog):
    opt, model, eng, twin, feats = _tiny('lstm', 'concat', 1, 1)
    o = {'sample_max': 0, 'top_k': 9, 'top_p': 0.9}
    torch.manual_seed(8)
    with caplog.at_level('WARNING'):
        seq, lp = eng.sample(model, feats, o)
        eng.sample(model, feats, o)
    assert sum('top_k' in r.getMessage() for r in caplog.records) == 1  # logged once
    assert model.impl == 'hip'
    model.impl = 'torch'
    try:
        torch.manual_seed(8)
        seq_t, lp_t = model.sample(feats, o)
    finally:
        model.impl = 'hip'
    assert torch.equal(seq, seq_t) and torch.equal(lp, lp_t)
    inside, _, alive, _ = tc.membership(tc.teacher_force(model_twin(model), feats, seq, 1), seq,
                                        9, 0.9, 1.0)
    assert inside[alive].all()
    for bad in ({'top_k': -1}, {'top_p': 0.5}, {'top_k': 3, 'top_p': 0.0}, {'top_k': 301}):
        with pytest.raises(ValueError):
            eng.sample(model, feats, dict(bad, sample_max=0))


def model_twin(model):
    """The same weights on the PyTorch path (fp32: the torch path decoded them)."""
    twin = copy.deepcopy(model)
    twin.impl = 'torch'
    return twin


# -- sample_mbr and the trainer on the fused engine --------------------------------------
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
        model.logit.weight.mul_(9.0)
    engine.refresh_weights()
    model.eval()
    loader = CaptionLoader(ds, B, 5, 'test', dev)
    return ds, opt, model, engine, loader


@pytest.mark.parametrize('C', [1, 4], ids=['lstm', 'temporal_att'])
def test_sample_mbr_fused_engine_truncated(C):
    from cst_captioning_amd.ops.mbr import PeerCiderD
    ds, opt, model, engine, loader = _engine_model(C)
    # (the twin first: an engine that holds a captured beam graph does not copy)
    twin = copy.deepcopy(model)
    twin.impl = 'torch'
    with torch.no_grad():
        for q in twin.parameters():
            q.copy_(q.bfloat16().float())
    feats = loader.get_batch_at(0)['feats']
    scorer = PeerCiderD(ds.df, use_eos=1, device=DEV)
    o = {'decode': 'mbr', 'beam_size': 3, 'mbr_samples': 5, 'mbr_temperature': 1.0,
         'mbr_top_k': 3, 'mbr_scorer': scorer}
    before = model.seq_per_img
    torch.manual_seed(5)
    seq, lp, info = model.sample_mbr(feats, o)
    assert model.seq_per_img == before
    pool, best = info['pool'], info['best']
    B, G, T = pool.shape
    assert (B, G) == (4, 6) and seq.shape == (B, T) and lp.shape == (B, T)
    beam, _ = model.sample_beam(feats, {'beam_size': 3})
    w = beam.size(1)
    assert torch.equal(pool[:, 0, :w], beam) and not pool[:, 0, w:].any()
    assert torch.equal(seq, pool[torch.arange(B, device=DEV), best])
    # the pool rows lie in the top 3 of the twin's teacher-forced distributions
    rows = pool[:, 1:].reshape(B * 5, T)[:, :opt.seq_length - 2]
    pred = tc.teacher_force(twin, feats, rows, 5)
    inside, sure, alive, _ = tc.membership(pred, rows, 3, 1.0, 1.0, near=0.05)
    # (excused only within 0.05 of the rank 3 / rank 4 boundary, at most 5 %)
    assert not (alive & ~inside & sure).any()
    assert (alive & ~inside & ~sure).sum().item() <= 0.05 * alive.sum().item()
    assert len({tuple(r) for r in rows.cpu().tolist()}) > B
    torch.manual_seed(5)
    assert torch.equal(model.sample_mbr(feats, o)[2]['pool'], pool)


def test_trainer_validate_mbr_top_k_fused_engine():
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.data import CaptionLoader
    from cst_captioning_amd.train.trainer import Trainer
    ds, opt, model, engine, val = _engine_model(1)
    opt.val_scorer, opt.decode, opt.mbr_samples, opt.mbr_top_k = 'tokens', 'mbr', 5, 3
    opt.test_batch_size, opt.test_seq_per_img, opt.batch_size = 4, 5, 4
    dev = torch.device(DEV)
    train = CaptionLoader(ds, 4, 5, 'train', dev, seed=0)
    tr = Trainer(opt, model, train, val, DistContext(device=dev), engine)
    assert tr.mbr_scorer.backend == 'gpu' and tr.decode_opts()['mbr_top_k'] == 3
    res = tr.validate(val)
    assert res['sequences'].shape[0] == 12
    assert all(0.0 <= p['mbr_score'] <= 10.0001 for p in res['predictions'])
    assert math.isfinite(res['scores']['CIDEr'])
