"""Numerics of the gfx950 HIP kernels against plain PyTorch fp32 references.

Every test here runs the native extension on the GPU (``pytest -m gpu``):
  * CIDEr-D kernel vs the fp64 Python oracle;
  * fused clip + Adam vs clip_grad_norm_ + torch.optim.Adam;
  * fused decoder (teacher forcing, greedy, MIXER rollout) and its backward
    vs the PyTorch CaptionModel path, at bf16 tolerances;
  * Gumbel-max sampler distribution vs softmax;
  * the reference's "all rows emitted EOS" stop rule on the device.
"""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _ext():
    from cst_captioning_amd import _ext
    assert _ext.available(), 'native extension must be built for GPU tests'
    return _ext.ops()


def _tiny(V=300, H=64, feat_dims=(48, 32), S=5, B=6, L=12, seed=0, drop=0.0):
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import make_synthetic, CaptionLoader
    from cst_captioning_amd.models import CaptionModel
    ds = make_synthetic('msrvtt', num_videos=40, vocab_size=V, seq_length=L,
                        feat_dims=list(feat_dims), seed=seed)
    opt = default_opts(vocab_size=V, seq_length=L, feat_dims=list(feat_dims),
                       train_seq_per_img=S, rnn_size=H, input_encoding_size=H,
                       drop_prob_lm=drop)
    torch.manual_seed(seed)
    model = CaptionModel(opt).to(DEV)
    with torch.no_grad():  # make the decoder non-trivial
        model.logit.weight.mul_(3.0)
        model.core.rnn.weight_hh_l0.mul_(2.0)
    loader = CaptionLoader(ds, B, S, 'train', DEV, seed=seed)
    return ds, opt, model, loader


def _engine(model, opt):
    from cst_captioning_amd.models.decoder_engine import DecoderEngine
    return DecoderEngine(model, opt)


def test_extension_loaded_from_tree():
    import cst_captioning_amd
    m = _ext()
    assert cst_captioning_amd.__path__[0] in m.__file__


def test_extension_entry_points_unchanged():
    """The extension binds exactly the names recorded in
    tests/golden/ext_entry_points.txt (one per line): no binding is lost or
    renamed when the host sources are reorganised."""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                          'ext_entry_points.txt')
    with open(golden) as f:
        want = {line.strip() for line in f if line.strip()}
    got = {n for n in dir(_ext()) if not n.startswith('_')}
    assert got == want, (sorted(got - want), sorted(want - got))


def test_cider_kernel_matches_oracle():
    from cst_captioning_amd.data import make_synthetic
    from cst_captioning_amd.ops.cider_d import CiderDScorer
    ds = make_synthetic('msvd', num_videos=60, vocab_size=200, feat_dims=[8], seed=3)
    rng = np.random.RandomState(1)
    N = 333
    hyps = torch.from_numpy(rng.randint(0, 200, size=(N, 28)))
    vid = torch.from_numpy(rng.randint(0, 60, size=N))
    for i in range(0, N, 2):  # half of them close to a reference
        g = ds.gts_of(int(vid[i]))[rng.randint(3)]
        hyps[i, :27] = torch.from_numpy(g[1:28])
    hyps[4] = 0
    hyps[6, 2:] = 1  # BOS in the middle is skipped
    for use_eos in (0, 1):
        sc = CiderDScorer(ds, use_eos=use_eos, device=DEV, backend='gpu')
        got = sc.score(hyps.to(DEV), vid.to(DEV)).cpu().numpy()
        ref = sc.score_reference(hyps, vid)
        assert np.abs(got - ref).max() < 1e-4 * max(1.0, ref.max()), (use_eos, got[:5], ref[:5])


def test_flat_adam_matches_torch():
    from cst_captioning_amd.ops.adam import FlatAdam
    from cst_captioning_amd.parallel import FlatGradBucket
    torch.manual_seed(0)
    shapes = [(37, 5), (1001,), (64, 64), (3,)]
    ps = [torch.randn(s, device=DEV, requires_grad=True) for s in shapes]
    ref = [p.detach().clone().requires_grad_(True) for p in ps]
    bucket = FlatGradBucket(ps)
    opt = FlatAdam(bucket, lr=1e-2, grad_clip=0.25)
    ropt = torch.optim.Adam(ref, lr=1e-2)
    for step in range(4):
        gs = [torch.randn(s, device=DEV) * (step + 1) for s in shapes]
        opt.zero_grad()
        for p, g in zip(ps, gs):
            p.grad.copy_(g)
        opt.step()
        ropt.zero_grad()
        for p, g in zip(ref, gs):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(ref, 0.25)
        ropt.step()
    for p, r in zip(ps, ref):
        torch.testing.assert_close(p.detach(), r.detach(), rtol=1e-5, atol=1e-6)


def test_flat_adam_skip_flag():
    from cst_captioning_amd.ops.adam import FlatAdam
    from cst_captioning_amd.parallel import FlatGradBucket
    p = torch.randn(100, device=DEV, requires_grad=True)
    bucket = FlatGradBucket([p])
    opt = FlatAdam(bucket, lr=1e-2)
    before = p.detach().clone()
    p.grad.fill_(1.0)
    opt.step(skip=torch.ones((), dtype=torch.bool, device=DEV))
    torch.testing.assert_close(p.detach(), before)
    assert opt.step_count == 0 and int(opt.skipped()) == 1


def test_flat_adam_skips_nonfinite_grad_norm_and_folds_grad_scale():
    """A finite loss with an overflowing gradient (inf in one slot) must not
    write NaN into p / m / v: the kernel skips on a non-finite norm, keeps
    the step count and counts the skip.  grad_scale = 1/N (DP sum) equals a
    pre-divided buffer."""
    from cst_captioning_amd.ops.adam import FlatAdam
    from cst_captioning_amd.parallel import FlatGradBucket
    torch.manual_seed(1)
    p = torch.randn(1000, device=DEV, requires_grad=True)
    q = p.detach().clone().requires_grad_(True)
    bp, bq = FlatGradBucket([p]), FlatGradBucket([q])
    op, oq = FlatAdam(bp, lr=1e-2, grad_clip=0.25), FlatAdam(bq, lr=1e-2, grad_clip=0.25)
    op.grad_scale = 0.125
    for _ in range(2):
        g = torch.randn(1000, device=DEV)
        p.grad.copy_(g * 8)
        q.grad.copy_(g)
        op.step()
        oq.step()
    torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-6, atol=1e-7)
    before = (p.detach().clone(), op.exp_avg.clone(), op.exp_avg_sq.clone())
    p.grad[17] = float('inf')
    op.step()
    torch.cuda.synchronize()
    for a, b in zip((p.detach(), op.exp_avg, op.exp_avg_sq), before):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    assert op.step_count == 2 and int(op.skipped()) == 1
    p.grad[17] = 0.0
    op.step()
    assert op.step_count == 3 and torch.isfinite(p).all()


# V = 1299 is not a multiple of the 128-wide vocab tile, 330 rows not of the
# 128-row tile
_SHAPES = [dict(), dict(V=1299, H=512)]
_SHAPE_IDS = ['h64', 'h512']


def _tiny_shape(seed=0, **shape):
    return _tiny(seed=seed, **shape)


@pytest.mark.parametrize('shape', _SHAPES, ids=_SHAPE_IDS)
def test_teacher_forced_logprobs_and_grads_match_torch(shape):
    ds, opt, model, loader = _tiny_shape(**shape)
    eng = _engine(model, opt)
    model.train()  # dropout is 0 in this config; MIOpen RNN backward needs train mode
    data = loader.get_batch()
    labels = data['labels']
    ref_model = copy.deepcopy(model)
    ref_model.impl = 'torch'
    ref_model.set_seq_per_img(5)
    pred = ref_model(data['feats'], labels)[0]
    T = labels.size(1) - 1
    tgt = labels[:, 1:1 + pred.size(1)]
    ref_lp = pred.gather(2, tgt.unsqueeze(2)).squeeze(2)
    model.set_seq_per_img(5)
    g_xe = eng.teacher_forced(model, data['feats'], labels)
    mask = data['masks'][:, 1:]
    n = pred.size(1)
    got = g_xe[:, :n]
    m = mask[:, :n] > 0
    assert (got[m] - ref_lp[m]).abs().max() < 0.08, (got[m] - ref_lp[m]).abs().max()
    # gradients of the XE loss
    from cst_captioning_amd.models import CrossEntropyCriterion
    crit = CrossEntropyCriterion()
    crit(pred, labels[:, 1:], data['masks'][:, 1:]).backward()
    crit(g_xe, labels[:, 1:], data['masks'][:, 1:]).backward()
    for (name, p), (_, q) in zip(model.named_parameters(), ref_model.named_parameters()):
        if q.grad is None:
            continue
        err = (p.grad - q.grad).norm() / (q.grad.norm() + 1e-12)
        assert err < 0.06, (name, float(err))


def test_greedy_sample_matches_torch():
    ds, opt, model, loader = _tiny(seed=1)
    eng = _engine(model, opt)
    model.eval()
    data = loader.get_batch()
    ref = copy.deepcopy(model)
    ref.impl = 'torch'
    seq_ref, lp_ref = ref.sample(data['feats'], {'sample_max': 1})
    seq, lp = eng.sample(model, data['feats'], {'sample_max': 1})
    n = seq_ref.size(1)
    # bf16 may flip near-ties late in the sequence: compare the first steps
    agree = (seq[:, :4] == seq_ref[:, :4]).float().mean().item()
    assert agree > 0.9, agree
    assert (seq[:, n:] == 0).all()
    ok = seq[:, :1] == seq_ref[:, :1]
    assert ((lp[:, :1] - lp_ref[:, :1]).abs()[ok] < 0.05).all()


@pytest.mark.parametrize('K', [2, 3, 5])
def test_beam_search_kernel_matches_torch(K):
    """GPU beam step (beam.hip) vs the batched PyTorch beam search, which
    itself is pinned to a per-video spec of the reference in test_model.py.
    The torch side runs on the same bf16-rounded weights."""
    ds, opt, model, loader = _tiny(seed=2)
    with torch.no_grad():
        model.logit.weight.mul_(3.0)  # peaked distributions: few near-ties
    eng = _engine(model, opt)
    model.eval()
    data = loader.get_batch()
    ref = copy.deepcopy(model)
    ref.impl = 'torch'
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.bfloat16().float())
    seq_ref, lp_ref = ref.sample(data['feats'], {'beam_size': K})
    seq, lp = eng.sample_beam(model, data['feats'], {'beam_size': K})
    assert seq.shape == seq_ref.shape == (data['feats'][0].size(0), opt.seq_length)
    same = (seq == seq_ref).all(1)
    assert same.float().mean().item() >= 0.8, (seq, seq_ref)
    assert ((lp - lp_ref).abs()[same] < 0.05).all()


@pytest.mark.parametrize('shape', _SHAPES, ids=_SHAPE_IDS)
def test_rl_rollout_gradient_matches_torch(shape):
    """REINFORCE gradient through the sampled-token path (y_sel)."""
    ds, opt, model, loader = _tiny_shape(seed=2, **shape)
    eng = _engine(model, opt)
    model.train()  # dropout is 0 in this config
    model.set_mixer_from(1)
    model.set_seq_per_img(5)
    data = loader.get_batch()
    seq, g_sel, _ = eng.rollout(model, data['feats'], data['labels'])
    assert seq.shape == (data['labels'].size(0), data['labels'].size(1) - 2)
    w = torch.randn(seq.size(0), 1, device=DEV)
    from cst_captioning_amd.models import RewardCriterion
    RewardCriterion()(seq, g_sel, w[:, 0]).backward()
    # torch reference: teacher-force the sampled sequence
    ref = copy.deepcopy(model)
    ref.impl = 'torch'
    ref.zero_grad(set_to_none=True)
    ref.set_mixer_from(0)  # teacher-force the sampled tokens (dropout is 0 here)
    lab = torch.cat([data['labels'][:, :1], seq, torch.zeros_like(seq[:, :1])], 1)
    pred = ref(data['feats'], lab)[0]
    lp_ref = pred[:, :seq.size(1)].gather(2, seq[:, :pred.size(1)].unsqueeze(2)).squeeze(2)
    k = lp_ref.size(1)
    assert (g_sel[:, :k] - lp_ref).abs().max() < 0.08
    RewardCriterion()(seq[:, :k], lp_ref, w[:, 0]).backward()
    for (name, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if q.grad is None or q.grad.norm() == 0:
            continue
        err = (p.grad - q.grad).norm() / (q.grad.norm() + 1e-12)
        assert err < 0.08, (name, float(err))


def test_gumbel_sampler_distribution():
    ds, opt, model, loader = _tiny(V=200, seed=4)
    eng = _engine(model, opt)
    model.eval()
    B = 2
    feats = [f[:1].expand(400, *f.shape[1:]).contiguous()
             for f in loader.get_batch()['feats']]
    seq, lp = eng.sample(model, feats, {'sample_max': 0})
    # step-1 tokens are i.i.d. draws from softmax(logits of step 0)
    ref = copy.deepcopy(model)
    ref.impl = 'torch'
    with torch.no_grad():
        ctx = ref._video_ctx(ref.encode([f[:1] for f in feats]))
        st = ref.init_hidden(1)
        out, _ = ref._step(ref.embed(torch.ones(1, dtype=torch.long, device=DEV)), ctx, st)
        p = torch.softmax(ref.logit(out), -1)[0].cpu().numpy()
    counts = np.bincount(seq[:, 0].cpu().numpy(), minlength=p.size)
    top = np.argsort(-p)[:5]
    for v in top:
        expect = 400 * p[v]
        assert abs(counts[v] - expect) < 5 * np.sqrt(expect + 1) + 3, (v, counts[v], expect)


def test_rollout_stops_when_every_row_emits_eos():
    ds, opt, model, loader = _tiny(seed=5)
    with torch.no_grad():
        model.logit.bias[0] = 1e4  # EOS always wins
    eng = _engine(model, opt)
    model.train()
    model.set_mixer_from(1)
    model.set_seq_per_img(5)
    data = loader.get_batch()
    seq, g_sel, _ = eng.rollout(model, data['feats'], data['labels'])
    assert (seq == 0).all()
    assert torch.isfinite(g_sel).all()


@pytest.mark.parametrize('C', [1, 4])
def test_wide_tile_decode_matches_torch(C):
    """Rollout-sized launch (640 rows: 5 row tiles of the fused decode
    kernel, V not a multiple of the 128-wide vocab tile, H = 128, with and
    without temporal attention): teacher-forced log-probs, REINFORCE
    log-probs of sampled tokens and gradients vs the PyTorch path."""
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import make_synthetic, CaptionLoader
    from cst_captioning_amd.models import CaptionModel, CrossEntropyCriterion, RewardCriterion
    V, H, S, B = 1299, 128, 20, 32
    ds = make_synthetic('msrvtt', num_videos=64, vocab_size=V, seq_length=14,
                        feat_dims=[96, 64], num_chunks=C, seed=7)
    opt = default_opts(vocab_size=V, seq_length=14, feat_dims=[96, 64], train_seq_per_img=S,
                       rnn_size=H, input_encoding_size=H, drop_prob_lm=0.0, num_chunks=C)
    torch.manual_seed(7)
    model = CaptionModel(opt).to(DEV)
    with torch.no_grad():
        model.logit.weight.mul_(3.0)
        model.core.rnn.weight_hh_l0.mul_(2.0)
    eng = _engine(model, opt)
    model.train()
    data = CaptionLoader(ds, B, S, 'train', DEV, seed=7).get_batch()
    labels = data['labels']
    assert labels.size(0) == 640
    ref = copy.deepcopy(model)
    ref.impl = 'torch'
    pred = ref(data['feats'], labels)[0]
    n = pred.size(1)
    ref_lp = pred.gather(2, labels[:, 1:1 + n].unsqueeze(2)).squeeze(2)
    g_xe = eng.teacher_forced(model, data['feats'], labels)
    m = data['masks'][:, 1:1 + n] > 0
    assert (g_xe[:, :n][m] - ref_lp[m]).abs().max() < 0.08
    crit = CrossEntropyCriterion()
    crit(pred, labels[:, 1:], data['masks'][:, 1:]).backward()
    crit(g_xe, labels[:, 1:], data['masks'][:, 1:]).backward()
    for (name, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if q.grad is None or q.grad.norm() == 0 or name.endswith('align.bias'):
            continue
        err = (p.grad - q.grad).norm() / (q.grad.norm() + 1e-12)
        assert err < 0.06, (name, float(err))
    # sampled rollout: the engine's log-prob of each sampled token matches the
    # torch model teacher-forced on the same tokens
    model.zero_grad(set_to_none=True)
    model.set_mixer_from(1)
    with torch.no_grad():
        seq, g_sel, _ = eng.rollout(model, data['feats'], labels)
    ref.set_mixer_from(0)
    lab = torch.cat([labels[:, :1], seq, torch.zeros_like(seq[:, :1])], 1)
    with torch.no_grad():
        pr = ref(data['feats'], lab)[0]
    k = min(pr.size(1), seq.size(1))
    lp_ref = pr[:, :k].gather(2, seq[:, :k].unsqueeze(2)).squeeze(2)
    alive = torch.cumprod((seq[:, :k] > 0).long(), 1) > 0
    assert (g_sel[:, :k] - lp_ref).abs()[alive].max() < 0.08


def test_trainer_direct_gradient_slots_match_torch():
    """Through the Trainer the fused backward writes the vocab-head, embedding
    and LSTM weight gradients straight into the flat bucket (no autograd
    accumulate); the video columns of W_ih still arrive through autograd.
    The bucket must hold the same gradient as the PyTorch decoder's."""
    from cst_captioning_amd.models import CrossEntropyCriterion
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.train.trainer import Trainer
    ds, opt, model, loader = _tiny(seed=4)
    ref_model = copy.deepcopy(model)
    ref_model.impl = 'torch'
    eng = _engine(model, opt)
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    tr = Trainer(opt, model, loader, None, DistContext(device=torch.device(DEV)), eng)
    assert set(eng.direct_grad_slots) == {'wlog', 'blog', 'emb', 'wih', 'whh',
                                          'fp_w0', 'fp_b0', 'fp_w1', 'fp_b1'}
    model.train()
    ref_model.train()
    data = loader.get_batch()
    tr.optimizer.zero_grad()
    model.set_seq_per_img(5)
    loss, _ = tr.xe_loss(data)
    loss.backward()
    ref_model.set_seq_per_img(5)
    pred = ref_model(data['feats'], data['labels'])[0]
    CrossEntropyCriterion()(pred, data['labels'][:, 1:], data['masks'][:, 1:]).backward()
    for (name, p), (_, q) in zip(model.named_parameters(), ref_model.named_parameters()):
        if q.grad is None:
            continue
        err = (p.grad - q.grad).norm() / (q.grad.norm() + 1e-12)
        assert err < 0.06, (name, float(err))



def test_forward_full_logprobs_and_gradient_match_torch():
    """``model(feats, seq)`` on the engine: full (R, T, V) log-probs and the
    gradient of an arbitrary function of them (dense dS through the fused
    backward) vs the PyTorch path."""
    ds, opt, model, loader = _tiny(V=700, H=128, seed=6)
    model.impl = 'hip'
    model._engine = _engine(model, opt)
    model.train()
    model.set_seq_per_img(5)
    data = loader.get_batch()
    labels = data['labels']
    ref = copy.deepcopy(model)
    ref.impl = 'torch'
    ref._engine = None
    full, s_seq, s_lp = model(data['feats'], labels)
    pr, r_seq, r_lp = ref(data['feats'], labels)
    n = pr.size(1)
    assert full.shape[0] == pr.shape[0] and full.shape[2] == pr.shape[2]
    assert (full[:, :n] - pr).abs().max().item() < 0.08
    assert torch.equal(s_seq[:, :r_seq.size(1)], r_seq)
    wgt = torch.randn_like(pr) * (torch.rand_like(pr) < 0.05)  # sparse-ish dense weights
    (full[:, :n] * wgt).sum().backward()
    (pr * wgt).sum().backward()
    for (name, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if q.grad is None or q.grad.norm() == 0:
            continue
        err = (p.grad - q.grad).norm() / (q.grad.norm() + 1e-12)
        assert err < 0.06, (name, float(err))


@pytest.mark.parametrize('rows', [64, 6, 520])
def test_fused_featpool_matches_torch(rows):
    """csrc/kernels/featpool.hip (all modalities' Linear -> ReLU -> Dropout
    + concat, and the weight / bias backward) vs the PyTorch FeatPool in fp32:
    the headline modality sizes (2048, 4096, 1024, 300), H = 512; rows that
    are and are not multiples of the 64-row tile."""
    from cst_captioning_amd.models.modules import FeatPool
    from cst_captioning_amd.ops.featpool import featpool, fused_ok
    torch.manual_seed(0)
    dims = [2048, 4096, 1024, 300]
    pool = FeatPool(dims, 512, 0.0).to(DEV).train()
    feats = [torch.randn(rows, 1, d, device=DEV) for d in dims]
    assert fused_ok(pool, feats)
    ref_pool = copy.deepcopy(pool)
    out = featpool(pool, feats)
    ref = ref_pool(feats)
    assert out.shape == ref.shape == (rows, 4 * 512)
    # fp32 operands split into bf16 hi + lo on the bf16 matrix cores (three
    # MFMAs per step): products within ~2^-16 of fp32
    torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-4)
    assert ((out - ref).norm() / ref.norm()).item() < 5e-5
    assert ((out > 0) != (ref > 0)).float().mean().item() < 1e-4
    g = torch.randn_like(out)
    (out * g).sum().backward()
    # backward arithmetic vs fp32 on the fused forward's own ReLU mask (a
    # flipped near-zero unit moves a whole g * x term between the two masks)
    dz = g * (out.detach() > 0).float()
    for f, m in enumerate(pool.feat_list):
        x = feats[f].reshape(rows, -1)
        dzf = dz[:, 512 * f:512 * (f + 1)]
        ref_dw = dzf.t() @ x
        err = ((m[0].weight.grad - ref_dw).norm() / ref_dw.norm()).item()
        assert err < 5e-5, (f, err)
        torch.testing.assert_close(m[0].bias.grad, dzf.sum(0), rtol=1e-4, atol=1e-4)
    # dropout: about half the units kept, survivors scaled by 2, and the
    # backward routes gradient exactly through the survivors
    for m in pool.feat_list:
        m[2].p = 0.5
    pool.zero_grad()
    outd = featpool(pool, feats)
    kept = outd > 0
    pos = out > 0
    frac = (kept.float().sum() / pos.float().sum()).item()
    assert 0.45 < frac < 0.55, frac
    torch.testing.assert_close(outd[kept], 2 * out.detach()[kept], rtol=1e-5, atol=1e-5)
    outd.sum().backward()
    w0 = pool.feat_list[0][0]
    x0 = feats[0].reshape(rows, -1)
    dz = kept[:, :512].float() * 2.0
    torch.testing.assert_close(w0.bias.grad, dz.sum(0), rtol=1e-4, atol=1e-4)
    ref_dw = dz.t() @ x0
    assert ((w0.weight.grad - ref_dw).norm() / ref_dw.norm()).item() < 5e-5


@pytest.mark.parametrize('per_video', [True, False])
def test_fused_scst_loss_matches_torch(per_video):
    """csrc/kernels/loss.hip vs scst_from_scores + RewardCriterion: loss,
    reward, logged means and the gradient w.r.t. the sampled log-probs."""
    from cst_captioning_amd.models import RewardCriterion
    from cst_captioning_amd.ops.scst_loss import scst_loss
    from cst_captioning_amd.reward.rewards import scst_from_scores
    torch.manual_seed(0)
    B, S, T = 64, 20, 28
    R = B * S
    seq = torch.randint(0, 50, (R, T), device=DEV)
    seq[torch.rand(R, T, device=DEV) < 0.1] = 0  # EOS anywhere
    lp = (-torch.rand(R, T, device=DEV) * 5).requires_grad_(True)
    sample = torch.rand(R, device=DEV)
    greedy_v = torch.rand(B, device=DEV)
    greedy = greedy_v if per_video else greedy_v.repeat_interleave(S)
    loss, reward, m, b = scst_loss(seq, lp, sample, greedy)
    lp2 = lp.detach().clone().requires_grad_(True)
    rref, mref, bref = scst_from_scores(sample, greedy_v.repeat_interleave(S))
    ref = RewardCriterion()(seq, lp2, rref)
    torch.testing.assert_close(loss, ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(reward, rref, rtol=0, atol=0)
    torch.testing.assert_close(m, mref, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(b, bref, rtol=1e-6, atol=1e-6)
    (3.0 * loss).backward()
    (3.0 * ref).backward()
    torch.testing.assert_close(lp.grad, lp2.grad, rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize('tshort', [1, 2])
def test_fused_xe_loss_matches_torch(tshort):
    """csrc/kernels/loss.hip XE mode vs the loader's masks (data/dataset.py
    gather: positions < nonzeros + 1) + CrossEntropyCriterion: loss and the
    gradient w.r.t. the gathered log-probs; ragged captions, an empty one,
    a full-length one, and log-prob rows shorter than the label rows."""
    from cst_captioning_amd.models import CrossEntropyCriterion
    from cst_captioning_amd.ops.scst_loss import xe_loss
    torch.manual_seed(0)
    R, L = 1283, 32
    lens = torch.randint(0, L - 1, (R,), device=DEV)
    lens[0], lens[1] = 0, L - 2
    pos = torch.arange(L, device=DEV)[None, :]
    labels = torch.where((pos >= 1) & (pos <= lens[:, None]),
                         torch.randint(1, 500, (R, L), device=DEV), torch.zeros_like(pos))
    n = (labels != 0).sum(1, keepdim=True) + 1
    masks = (pos < n).float()
    T = L - tshort
    lp = (-torch.rand(R, T, device=DEV) * 5).requires_grad_(True)
    loss = xe_loss(labels, lp, 1)
    lp2 = lp.detach().clone().requires_grad_(True)
    ref = CrossEntropyCriterion()(lp2, labels[:, 1:], masks[:, 1:])
    torch.testing.assert_close(loss, ref, rtol=1e-5, atol=1e-6)
    (3.0 * loss).backward()
    (3.0 * ref).backward()
    torch.testing.assert_close(lp.grad, lp2.grad, rtol=1e-5, atol=1e-8)


def test_exp_store_backward_matches_dense_path():
    """The training backward (exp store, one-hot terms folded into E, no dS
    pass: csrc/kernels/vocab_grad.hip) against the dense-dS backward of the
    full log-prob API on the same rollout: MIXER sampling with both a sampled
    token term and an XE target term per row, including rows whose two
    weights cancel (a + b = 0) on different tokens and on the same token."""
    from cst_captioning_amd.models.decoder_engine import SEL_GT, SEL_SAMPLE
    ds, opt, model, loader = _tiny(V=1299, H=128, seed=4)
    eng = _engine(model, opt)
    model.train()
    model.set_seq_per_img(5)
    data = loader.get_batch()
    labels = data['labels']
    R, T = labels.size(0), labels.size(1) - 1
    modes = [SEL_GT if t + 1 < 4 else SEL_SAMPLE for t in range(T - 1)]
    gen = torch.Generator(device=DEV).manual_seed(11)
    w1 = torch.randn(R, T - 1, device=DEV, generator=gen)
    w2 = torch.randn(R, T, device=DEV, generator=gen)
    w2[::3, :T - 1] = -w1[::3]  # cancelling weights (GT steps: same token)

    def grads():
        return {n: p.grad.detach().clone() for n, p in model.named_parameters()
                if p.grad is not None}

    torch.manual_seed(5)
    seq, g_sel, g_xe, _ = eng._run(model, data['feats'], labels, modes, want_xe=True,
                                   use_counts=False, use_unfinished=False)
    model.zero_grad()
    ((g_sel * w1).sum() + (g_xe * w2).sum()).backward()
    got = grads()
    torch.manual_seed(5)
    seq2, g_sel2, _, full = eng._run(model, data['feats'], labels, modes, want_xe=True,
                                     use_counts=False, use_unfinished=False, want_full=True)
    assert torch.equal(seq, seq2)
    lp_xe = full.gather(2, labels[:, 1:1 + full.size(1)].unsqueeze(2)).squeeze(2)
    model.zero_grad()
    ((g_sel2 * w1).sum() + (lp_xe * w2[:, :lp_xe.size(1)]).sum()).backward()
    ref = grads()
    assert got.keys() == ref.keys()
    for n in ref:
        err = (got[n] - ref[n]).norm() / (ref[n].norm() + 1e-12)
        assert err < 2e-2, (n, float(err))


def test_exp_store_lse_jump_rows_recomputed():
    """Exp-store range guard (csrc/kernels/vocab_grad.hip vgrad_fix).  The
    decode kernel saves E = bf16(exp(x - lse_{t-1})); rows whose LSE jumps by
    about +-100 between steps overflow (inf) or underflow (0) there.  Saved
    tensors are built here exactly as the decode kernel writes them, with the
    vocab input of chosen rows scaled x60 on alternate steps (LSE ~7 <-> ~120);
    the backward must list and recompute those rows and give the fp32
    softmax gradient of the vocab head (no NaN, no lost rows)."""
    ops = _ext()
    torch.manual_seed(7)
    n, R, H, E, V = 4, 64, 128, 128, 1299
    ldl = (V + 63) // 64 * 64
    bf = torch.bfloat16
    wlog = (torch.rand(V, H, device=DEV) * 0.2 - 0.1).to(bf)
    blog = torch.randn(V, device=DEV) * 0.1
    scale = torch.ones(n, R, 1, device=DEV)
    jump = torch.arange(R, device=DEV) % 3 == 0  # every third row jumps
    scale[1::2, jump] = 60.0  # steps 1, 3: peaked (overflow); steps 2: back (underflow)
    hd = (torch.randn(n, R, H, device=DEV) * scale).to(bf)
    x = hd.float() @ wlog.float().t() + blog  # (n, R, V) fp32 logits
    lse = torch.logsumexp(x, 2)
    off = torch.cat([lse[:1], lse[:-1]], 0)  # step 0: its own LSE (exp_convert)
    Es = torch.zeros(n, R, ldl, device=DEV, dtype=bf)
    Es[:, :, :V] = torch.exp(x - off.unsqueeze(2)).to(bf)
    d = (lse[1:] - lse[:-1]).abs()
    n_jump = int((d > 60).sum())
    assert n_jump >= 2 * int(jump.sum()) and not torch.isfinite(Es.float()).all()
    T_sel = n
    seq = torch.multinomial(torch.softmax(x.view(-1, V), 1), 1).view(n, R).t().contiguous()
    dg_sel = torch.randn(R, T_sel, device=DEV)
    toks = torch.cat([torch.ones(1, R, dtype=torch.long, device=DEV), seq.t()[:-1]], 0).reshape(-1)
    wx = (torch.randn(4 * H, E + H, device=DEV) * 0.05).to(bf)
    emb = (torch.randn(V, E, device=DEV) * 0.1).to(bf)
    gates = (torch.rand(n, R, 4 * H, device=DEV)).to(bf)
    c_all = torch.randn(n, R, H, device=DEV) * 0.1
    h_all = (torch.randn(n, R, H, device=DEV) * 0.1).to(bf)
    empty = torch.empty(0, device=DEV)
    fix_total = torch.zeros(1, dtype=torch.int32, device=DEV)
    Es_fresh = Es.clone()  # the backward folds / rewrites rows of E in place
    res = ops.decoder_backward(wx, wlog, emb, lse.contiguous(), Es, hd.contiguous(), gates, c_all,
                               h_all, seq, torch.empty(0, dtype=torch.long, device=DEV), toks,
                               dg_sel, empty, 0.0, torch.empty(0, dtype=torch.int32, device=DEV),
                               empty, empty, 0, [], empty, empty, 0, [], [], blog, fix_total, 1, empty, [], 0, 0.0)
    torch.cuda.synchronize()
    assert int(fix_total) == n_jump
    dWlog, dblog = res[1], res[2]
    # fp32 reference: dS = a (onehot(ys) - p)
    p = torch.softmax(x, 2)
    a = dg_sel.t()  # (n, R)
    dS = -a.unsqueeze(2) * p
    dS.scatter_add_(2, seq.t().unsqueeze(2), a.unsqueeze(2))
    ref_w = dS.reshape(-1, V).t() @ hd.float().reshape(-1, H)
    ref_b = dS.reshape(-1, V).sum(0)
    assert torch.isfinite(dWlog).all() and torch.isfinite(dblog).all()
    for got, ref in ((dWlog, ref_w), (dblog, ref_b)):
        err = (got - ref).norm() / ref.norm()
        assert err < 2e-2, float(err)
    # without the guard (no bias given) the same inputs are not usable
    res0 = ops.decoder_backward(wx, wlog, emb, lse.contiguous(), Es, hd.contiguous(), gates,
                                c_all, h_all, seq, torch.empty(0, dtype=torch.long, device=DEV),
                                toks, dg_sel, empty, 0.0,
                                torch.empty(0, dtype=torch.int32, device=DEV), empty, empty, 0,
                                [], empty, empty, 0, [], [], empty, empty, 1, empty, [], 0, 0.0)
    bad = res0[1]
    assert (not torch.isfinite(bad).all()) or (bad - ref_w).norm() / ref_w.norm() > 0.1
    # X = E W from the rollout (decoder_backward.cpp have_x, "X in the rollout"): the listed rows'
    # X is recomputed from their exact E, the loop adds the one-hot rows, and
    # every gradient equals the X-less path's
    xw = (Es_fresh[:, :, :V].float() @ wlog.float()).contiguous()  # inf / nan rows included
    fix2 = torch.zeros(1, dtype=torch.int32, device=DEV)
    res2 = ops.decoder_backward(wx, wlog, emb, lse.contiguous(), Es_fresh, hd.contiguous(), gates,
                                c_all, h_all, seq, torch.empty(0, dtype=torch.long, device=DEV),
                                toks, dg_sel, empty, 0.0,
                                torch.empty(0, dtype=torch.int32, device=DEV), empty, empty, 0,
                                [], empty, empty, 0, [], [], blog, fix2, 1, xw, [], 0, 0.0)
    torch.cuda.synchronize()
    assert int(fix2) == n_jump
    for k in (0, 1, 2, 3, 4):  # dWx (the loop's dG), dWlog, dblog, d_emb, d_vgate
        a, b = res2[k], res[k]
        assert torch.isfinite(a).all(), k
        err = (a - b).norm() / (b.norm() + 1e-12)
        assert err < 2e-2, (k, float(err))


@pytest.mark.parametrize('batched', [False, True])
def test_tuned_blaslt_gemm_matches_torch(batched):
    """csrc/host/blaslt_tuned.cpp: the measured-choice hipBLASLt GEMM (bf16
    operands, fp32 output) against the fp32 product of the same bf16 values:
    a transposed A operand with a leading dimension wider than the row, a
    strided output (column slice of a wider matrix), and the strided batch
    (the dW_logit split-K groups of decoder_backward)."""
    from cst_captioning_amd import _ext
    ops = _ext.ops()
    torch.manual_seed(0)
    if not batched:
        K, M, N = 64, 300, 200
        a = torch.randn(K, M + 8, device=DEV).to(torch.bfloat16)[:, :M]  # (K, M), ld M + 8
        b = torch.randn(K, N, device=DEV).to(torch.bfloat16)
        wide = torch.full((M, N + 40), 7.0, device=DEV)
        out = wide[:, 20:20 + N]
        ops.gemm_bf16_tuned(out, a, True, b, False)
        ref = a.float().t() @ b.float()
        torch.testing.assert_close(out, ref, rtol=2e-5, atol=2e-4)
        assert (wide[:, :20] == 7.0).all() and (wide[:, 20 + N:] == 7.0).all()
    else:
        B, K, M, N, ld = 4, 256, 520, 48, 536
        rows = torch.randn(B * K, ld, device=DEV).to(torch.bfloat16)
        a = rows.as_strided((B, K, M), (K * ld, ld, 1))
        b = torch.randn(B, K, N, device=DEV).to(torch.bfloat16)
        out = torch.empty(B, M, N, device=DEV)
        ops.gemm_bf16_tuned_batched(out, a, True, b, False)
        ref = torch.bmm(a.float().transpose(1, 2), b.float())
        torch.testing.assert_close(out, ref, rtol=2e-5, atol=2e-4)


def test_tuned_blaslt_gemm_timed_choice_and_tiny_shapes():
    """The tuner's two paths (csrc/host/blaslt_tuned.cpp).  A GEMM of at least
    4 GFLOP (520 x 4096, K = 1024: 4.36 GFLOP) is timed: its candidates'
    timings are recorded, the choice is the FIRST candidate within 4 % of the
    fastest (near-ties must not alternate between runs), and the result
    matches the fp32 product (atol: the K = 256 bound of the test above times
    4, rounding error growing at most linearly in K).  A GEMM below the
    threshold takes the heuristic's first candidate without any timing."""
    from cst_captioning_amd import _ext
    ops = _ext.ops()
    torch.manual_seed(1)

    def choice(M, N, K):
        c = [r for r in ops.gemm_tuned_choices() if (r[0], r[1], r[2]) == (N, M, K)]
        assert len(c) == 1, c
        return int(c[0][3]), c[0][4]

    K, M, N = 1024, 520, 4096
    a = torch.randn(K, M, device=DEV).to(torch.bfloat16)
    b = torch.randn(K, N, device=DEV).to(torch.bfloat16)
    out = torch.empty(M, N, device=DEV)
    ops.gemm_bf16_tuned(out, a, True, b, False)
    torch.testing.assert_close(out, a.float().t() @ b.float(), rtol=2e-5, atol=8e-4)
    us = ops.gemm_tuned_timings(out, a, True, b, False)
    assert len(us) >= 1 and min(us) > 0
    _, chosen_us = choice(M, N, K)
    first_in_band = next(t for t in us if t <= min(us) * 1.04)
    assert abs(chosen_us - first_in_band) < 1e-9, (chosen_us, us)

    K, M, N = 72, 136, 264  # 5 MFLOP
    a = torch.randn(K, M, device=DEV).to(torch.bfloat16)
    b = torch.randn(K, N, device=DEV).to(torch.bfloat16)
    out = torch.empty(M, N, device=DEV)
    ops.gemm_bf16_tuned(out, a, True, b, False)
    torch.testing.assert_close(out, a.float().t() @ b.float(), rtol=2e-5, atol=2e-4)
    assert ops.gemm_tuned_timings(out, a, True, b, False) == []
    assert choice(M, N, K) == (0, -1.0)
