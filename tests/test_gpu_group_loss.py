"""``--rl_objective`` on the fused path: the group-loss kernels
(``csrc/kernels/loss.hip`` group objectives, ``ops/scst_loss.py:group_loss``)
against ``GroupCriterion`` in fp64 on the same inputs, bit-equal between
launches, refused outside their limits; the existing fused losses unchanged
by the new trailing arguments; and the objective inside the eager and the
replayed HIP-graph training step."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
OBJECTIVES = ('risk', 'softmax_margin', 'multi_margin')

# name: (B, S, T, alpha, kappa, seed).  The seeds are fixed so that the
# multi-margin hinges of the fp64 reference stay away from their kink (see
# test_kernel_matches_criterion_fp64); chosen on the CPU, from the inputs alone.
CASES = {
    'headline': (64, 20, 28, 1.0, 1.0, 10),      # the training shape
    'partial_wg': (3, 5, 7, 0.25, 3.0, 0),       # B % 4 != 0: a partly empty workgroup
    'full_wave': (2, 64, 30, 1.0, 1.0, 0),       # S = 64
    'pair': (5, 2, 3, 1.0, 1.0, 0),              # S = 2
    'one_token': (4, 3, 1, 1.0, 1.0, 0),         # T = 1
    'long': (2, 4, 70, 1.0, 1.0, 0),             # T > 64: lanes stride over the row
    'alpha8': (6, 20, 28, 8.0, 1.0, 0),          # wide spread of s: the max subtraction
    'eos_first': (3, 5, 7, 1.0, 1.0, 0),         # rows whose first token is EOS
    'equal_video': (3, 5, 7, 1.0, 1.0, 1),       # a video whose scores are all equal
    'ties': (5, 6, 7, 1.0, 2.0, 0),              # the maximum attained twice, not first at 0
}
_CACHE = {}


def _case(name):
    """(seq, lp fp32, scores, alpha, kappa) on the CPU, drawn as
    tests/test_gpu_cst.py draws them (scores on a coarse grid)."""
    if name not in _CACHE:
        B, S, T, alpha, kappa, seed = CASES[name]
        g = torch.Generator().manual_seed(seed)
        R = B * S
        seq = torch.randint(0, 50, (R, T), generator=g)
        seq[torch.rand(R, T, generator=g) < 0.1] = 0
        lp = -torch.rand(R, T, generator=g) * 5
        scores = torch.randint(0, 12, (B, S), generator=g).float() / 8.0
        if name == 'eos_first':
            seq[::2, 0] = 0
            seq[1] = 0
        if name == 'equal_video':
            scores[1] = 0.75
        if name == 'ties':
            top = scores.max(1)[0] + 0.125
            scores[:, 2] = top
            scores[:, 4] = top
        _CACHE[name] = (seq, lp, scores, alpha, kappa)
    return _CACHE[name]


def _reference(name, objective):
    """GroupCriterion in fp64 on the CPU: (loss, reward, m, b, d(2 loss)/dlp)."""
    key = (name, objective)
    if key not in _CACHE:
        from cst_captioning_amd.models import GroupCriterion
        seq, lp, scores, alpha, kappa = _case(name)
        lp64 = lp.double().requires_grad_(True)
        loss, reward, m, b = GroupCriterion(objective, alpha, kappa)(seq, lp64, scores)
        (2.0 * loss).backward()
        _CACHE[key] = tuple(t.detach() for t in (loss, reward, m, b, lp64.grad))
    return _CACHE[key]


def _hinge_distance(name):
    """min |h_j| over j != i* of the fp64 reference, h_j = c_j - s_{i*} + s_j."""
    from cst_captioning_amd.models import reward_mask
    seq, lp, scores, alpha, kappa = _case(name)
    B, S = scores.shape
    m = reward_mask(seq).double()
    s = (alpha * (lp.double() * m).sum(1) / m.sum(1)).view(B, S)
    r = scores.double()
    istar = r.argmax(1, keepdim=True)
    h = kappa * (r.max(1, keepdim=True)[0] - r) - s.gather(1, istar) + s
    h.scatter_(1, istar, float('inf'))
    return h.abs().min().item()


def _fused(name, objective):
    from cst_captioning_amd.ops.scst_loss import group_loss
    seq, lp, scores, alpha, kappa = _case(name)
    lpd = lp.to(DEV).requires_grad_(True)
    loss, reward, m, b = group_loss(seq.to(DEV), lpd, scores.to(DEV), objective, alpha, kappa)
    (2.0 * loss).backward()
    return loss.detach(), reward, m, b, lpd.grad


@pytest.mark.parametrize('objective', OBJECTIVES)
@pytest.mark.parametrize('name', list(CASES))
def test_kernel_matches_criterion_fp64(name, objective):
    """Loss, reward, logged means and the log-prob gradient of the fused group
    loss against GroupCriterion in fp64, at the tolerances of the fused losses
    (tests/test_gpu_cst.py).  multi_margin is discontinuous where a hinge
    h_j = 0: the inputs (fixed seeds) keep every |h_j|, j != i*, above 1e-3 in
    the fp64 reference -- a condition on the inputs, asserted here."""
    if objective == 'multi_margin':
        assert _hinge_distance(name) >= 1e-3
    if name == 'ties':
        sc = _case(name)[2]
        assert ((sc == sc.max(1, keepdim=True)[0]).sum(1) == 2).all() and sc.argmax(1).eq(2).all()
    want = _reference(name, objective)
    got = _fused(name, objective)
    for g, w, what in zip(got, want, ('loss', 'reward', 'm', 'b', 'grad')):
        g, w = g.double().cpu(), w.double()
        print(name, objective, what, 'max abs err %.3e' % (g - w).abs().max().item())
    loss, reward, m, b, grad = (t.double().cpu() for t in got)
    torch.testing.assert_close(loss, want[0], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(reward, want[1], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(m, want[2], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(b, want[3], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(grad, want[4], rtol=1e-5, atol=1e-8)
    if name == 'equal_video' and objective == 'risk':
        S, T = CASES[name][1], CASES[name][2]
        assert torch.equal(grad[S:2 * S], torch.zeros(S, T, dtype=torch.float64))


@pytest.mark.parametrize('objective', OBJECTIVES)
def test_two_launches_bit_equal(objective):
    a = _fused('headline', objective)
    b = _fused('headline', objective)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_refused_outside_limits():
    """S = 65, S = 1 and R % S != 0 raise before any launch."""
    from cst_captioning_amd import _ext
    from cst_captioning_amd.ops.scst_loss import group_loss
    T = 5
    for B, S in ((2, 65), (4, 1)):
        seq = torch.ones(B * S, T, dtype=torch.long, device=DEV)
        lp = torch.zeros(B * S, T, device=DEV)
        with pytest.raises(RuntimeError, match='2 <= S <= 64'):
            group_loss(seq, lp, torch.zeros(B, S, device=DEV), 'risk')
    R, S = 10, 3
    seq = torch.ones(R, T, dtype=torch.long, device=DEV)
    lp = torch.zeros(R, T, device=DEV)
    none = torch.empty(0, device=DEV)
    with pytest.raises(RuntimeError, match='dividing R'):
        _ext.ops().cst_loss_forward(seq, lp, torch.zeros(R, device=DEV), none, S, 0, 1, 1.0, 1.0)
    with pytest.raises(RuntimeError, match='objective'):
        _ext.ops().cst_loss_forward(seq, lp, torch.zeros(R, device=DEV), none, 5, 0, 4, 1.0, 1.0)
    with pytest.raises(RuntimeError, match='alpha'):
        _ext.ops().cst_loss_forward(seq, lp, torch.zeros(R, device=DEV), none, 5, 0, 1, 0.0, 1.0)
    with pytest.raises(ValueError):
        group_loss(seq, lp, torch.zeros(2, 5, device=DEV), 'risk', alpha=float('nan'))
    torch.cuda.synchronize()


def test_existing_fused_losses_unchanged():
    """cst_loss and scst_loss, called as tests/test_gpu_cst.py and
    tests/test_gpu_kernels.py call them, are bit-equal to the extension's
    entry points called without the new trailing arguments."""
    from cst_captioning_amd import _ext
    from cst_captioning_amd.ops.scst_loss import cst_loss, scst_loss
    ops = _ext.ops()
    torch.manual_seed(21)
    B, S, T = 64, 20, 28
    R = B * S
    seq = torch.randint(0, 50, (R, T), device=DEV)
    seq[torch.rand(R, T, device=DEV) < 0.1] = 0
    lp0 = -torch.rand(R, T, device=DEV) * 5
    scores = torch.randint(0, 12, (B, S), device=DEV).float() / 8.0
    bcmr = torch.randint(0, 12, (B, S), device=DEV).float() / 7.0
    two = torch.full((1,), 2.0, device=DEV)
    none = torch.empty(0, device=DEV)
    for scb_baseline, k in ((1, 20), (2, 7), (2, 0)):
        lp = lp0.clone().requires_grad_(True)
        loss, reward, m, b = cst_loss(seq, lp, scores, bcmr, k, scb_baseline)
        (2.0 * loss).backward()
        bref = bcmr.reshape(-1) if (k > 0 and scb_baseline == 1) else none
        l2, out, r2 = ops.cst_loss_forward(seq, lp0, scores.reshape(-1), bref, S, k)
        assert torch.equal(loss.detach(), l2) and torch.equal(reward, r2)
        assert torch.equal(m, out[1]) and torch.equal(b, out[2])
        assert torch.equal(lp.grad, ops.scst_loss_backward(seq, r2, out, two))
    sample = torch.rand(R, device=DEV)
    for greedy in (torch.rand(B, device=DEV), torch.rand(R, device=DEV)):
        lp = lp0.clone().requires_grad_(True)
        loss, reward, m, b = scst_loss(seq, lp, sample, greedy)
        (3.0 * loss).backward()
        l2, out, r2 = ops.scst_loss_forward(seq, lp0, sample, greedy)
        assert torch.equal(loss.detach(), l2) and torch.equal(reward, r2)
        assert torch.equal(m, out[1]) and torch.equal(b, out[2])
        assert torch.equal(lp.grad, ops.scst_loss_backward(seq, r2, out, 1.5 * two))


def _setup(objective, graph, seed=0, V=500, H=128):
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import make_synthetic, CaptionLoader
    from cst_captioning_amd.cli import build_model
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.train.trainer import Trainer
    S = 5
    ds = make_synthetic('msrvtt', num_videos=48, vocab_size=V, seq_length=12,
                        feat_dims=[64, 32], seed=seed)
    opt = default_opts(vocab_size=V, seq_length=12, feat_dims=[64, 32], train_seq_per_img=S,
                       batch_size=8, rnn_size=H, input_encoding_size=H, drop_prob_lm=0.5,
                       use_rl=1, use_rl_after=0, use_cst=0, use_mixer=1, mixer_from=1,
                       use_eos=1, impl='hip', cuda_graph=graph, learning_rate=1e-3,
                       rl_objective=objective, rl_alpha=2.0, rl_cost_scale=0.5)
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    torch.manual_seed(seed)
    dev = torch.device(DEV)
    model, engine = build_model(opt, dev, 'hip')
    assert engine is not None
    loader = CaptionLoader(ds, 8, S, 'train', dev, seed=seed)
    tr = Trainer(opt, model, loader, None, DistContext(device=dev), engine)
    tr.rl_training = True
    return tr, loader


@pytest.mark.parametrize('objective', ['risk', 'softmax_margin'])
def test_group_step_fused_and_graphed(objective, monkeypatch):
    """The objective through the trainer (modelled on
    test_cst_step_fused_and_graphed): (a) the eager fused step's loss, reward
    and logged means equal GroupCriterion on the tokens it sampled, their
    log-probs and their on-GPU scores; (b) the captured, replayed step gives
    the eager step's samples, rewards, loss and logged means with the seeds
    pinned, and the same weights after 4 updates; no greedy decode is enqueued
    or captured."""
    from cst_captioning_amd.models import GroupCriterion
    from cst_captioning_amd.ops import featpool as fp
    from cst_captioning_amd.train.trainer import Trainer

    def no_greedy(*a, **k):
        raise AssertionError('a group objective decodes no greedy baseline')
    monkeypatch.setattr(Trainer, '_greedy_scores', no_greedy)
    fixed = torch.tensor([2468, 1357], dtype=torch.int32, device=DEV)
    a, la = _setup(objective, graph=0)
    b, lb = _setup(objective, graph=1)
    seen = {}
    rollout = a._decode_rollout

    def spy(data):
        seq, lp, pred = rollout(data)
        seen['seq'], seen['lp'] = seq.detach().clone(), lp.detach().float().clone()
        return seq, lp, pred
    a._decode_rollout = spy
    for tr in (a, b):
        tr.engine._rng = lambda dev: fixed
    old = fp.SEED_SOURCE
    fp.SEED_SOURCE = lambda dev: fixed
    try:
        for it in range(4):
            da, db = la.get_batch(), lb.get_batch()
            oa = a.train_step(da, 0)
            ob = b.train_step(db, 0)
            torch.cuda.synchronize()
            if it == 0:  # (a) the fused loss against the criterion
                S = 5
                assert torch.equal(seen['seq'], oa['seq'])
                vid = da['video_index'].repeat_interleave(S)
                sc = a._ensure_scorer().score(oa['seq'], vid).float().view(-1, S)
                want = GroupCriterion(objective, 2.0, 0.5)(oa['seq'], seen['lp'].double(), sc)
                for k, w in zip(('loss', 'reward', 'm', 'b'), want):
                    torch.testing.assert_close(torch.as_tensor(oa[k]).double(), w.double(),
                                               rtol=1e-5, atol=1e-6)
            assert torch.equal(oa['seq'], ob['seq'])
            torch.testing.assert_close(oa['reward'], ob['reward'], rtol=1e-5, atol=1e-6)
            for k in ('loss', 'm', 'b'):
                torch.testing.assert_close(torch.as_tensor(oa[k]).float(),
                                           torch.as_tensor(ob[k]).float(), rtol=1e-5, atol=1e-6)
    finally:
        fp.SEED_SOURCE = old
    assert b._graph is not None and a._graph is None
    assert getattr(a, '_side_stream', None) is None and getattr(b, '_side_stream', None) is None
    pa = torch.cat([p.detach().reshape(-1) for p in a.model.parameters()])
    pb = torch.cat([p.detach().reshape(-1) for p in b.model.parameters()])
    assert ((pa - pb).norm() / pa.norm()).item() < 1e-4
