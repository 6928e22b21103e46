"""EMA of the parameters on the GPU (``--ema_decay``): the update kernel's EMA
instantiation, the sharded phases on a slice, the swap-and-refresh kernel, the
captured training step and validation with the averaged weights on the fused
engine (csrc/kernels/adam.hip, ops/adam.py, Trainer.ema_weights).

Tolerance against the fp64 recurrence ``e64 += (1 - d) (p - e64)`` over the
kernel's own parameter trajectory (p read back after every step): a step adds
at most about 5 fp32 roundings of magnitude M (the largest ``|p|`` or ``|e|``
seen), every earlier error shrinks by d per step, so
``|e - e64| <= 5 * 2^-24 * M / (1 - d)`` (atol, rtol 0; FMA contraction only
lowers the error)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
# 185 + 1001 + 1849 + 40 = 3075 = 4 * 256 * 3 + 3: three blocks of float4s and
# a tail, tensor boundaries inside float4s
SHAPES = [(37, 5), (1001,), (43, 43), (40,)]
EMPTY_META = torch.empty(0, dtype=torch.int64)


def _ops():
    from cst_captioning_amd import _ext
    assert _ext.available(), 'native extension must be built for GPU tests'
    return _ext.ops()


def ema_bound(M, d):
    return 5 * 2.0 ** -24 * M / (1 - d)


class _RawBucket:
    """Flat buffers of exactly n elements (FlatGradBucket pads to 64)."""
    sharded = False

    def __init__(self, n, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.data = torch.randn(n, generator=g).to(DEV)
        self.grad = torch.zeros(n, device=DEV)

    def zero_grad(self):
        self.grad.zero_()


def _plain_shadows(n):
    """PLAIN segments over the first and third tensor of SHAPES (n = 3075), or
    the whole buffer (n = 3)."""
    if n == 3:
        segs = [(0, 3)]
    else:
        segs = [(0, 185), (1186, 1849)]
    meta = torch.tensor([[off, m, 0, 0, 0, 0, 0, 0] for off, m in segs], dtype=torch.int64)
    empty = torch.empty(0, dtype=torch.bfloat16, device=DEV)
    dsts = []
    for _, m in segs:
        dsts += [torch.zeros(m, dtype=torch.bfloat16, device=DEV), empty]
    return segs, meta, dsts


def _run_update(n, d, seed=0):
    """6 steps: step 2 skipped by the flag, step 4 has an inf gradient.
    Returns (optimizer, bucket, trajectory checks done inside)."""
    from cst_captioning_amd.ops.adam import FlatAdam
    b = _RawBucket(n, seed)
    opt = FlatAdam(b, lr=1e-2, ema_decay=d)
    segs, meta, dsts = _plain_shadows(n)
    opt.set_shadows(meta, dsts)
    g = torch.Generator().manual_seed(seed + 1)
    grads = [torch.randn(n, generator=g).to(DEV) for _ in range(6)]
    grads[4][n // 2] = float('inf')
    yes = torch.ones((), dtype=torch.bool, device=DEV)
    traj, emas = [b.data.clone()], [None if opt.ema is None else opt.ema.clone()]
    for t in range(6):
        b.grad.copy_(grads[t])
        opt.step(yes if t == 2 else None)
        traj.append(b.data.clone())
        emas.append(None if opt.ema is None else opt.ema.clone())
    return opt, b, traj, emas, (segs, dsts)


@pytest.mark.parametrize('n', [3, 4 * 256 * 3 + 3])
def test_update_kernel_ema(n):
    d = 0.9
    assert sum(torch.Size(s).numel() for s in SHAPES) == 4 * 256 * 3 + 3
    opt, b, traj, emas, (segs, dsts) = _run_update(n, d)
    assert opt.step_count == 4 and int(opt.skipped()) == 2
    e64 = traj[0].double()
    M = float(traj[0].abs().max())
    for t in range(6):
        if t in (2, 4):  # skipped: nothing moves, bit for bit
            assert torch.equal(traj[t + 1], traj[t])
            assert torch.equal(emas[t + 1], emas[t]), 'a skipped step touched the EMA'
        else:
            assert not torch.equal(traj[t + 1], traj[t])
            e64 += (1 - d) * (traj[t + 1].double() - e64)
        M = max(M, float(traj[t + 1].abs().max()), float(emas[t + 1].abs().max()))
    err = float((opt.ema.double() - e64).abs().max())
    print('n = %d: max |e - e64| = %.3e, bound %.3e' % (n, err, ema_bound(M, d)))
    assert err <= ema_bound(M, d)
    assert not torch.equal(opt.ema, b.data)
    # no side effect on the update: p, m, v of an optimizer without the EMA
    o0, b0, traj0, _, (_, dsts0) = _run_update(n, 0.0)
    assert o0.ema is None
    assert torch.equal(b0.data, b.data)
    assert torch.equal(o0.exp_avg, opt.exp_avg) and torch.equal(o0.exp_avg_sq, opt.exp_avg_sq)
    # the shadows of the EMA instantiation: bf16 of the parameters, as without it
    for (off, m), dst, dst0 in zip(segs, dsts[::2], dsts0[::2]):
        assert torch.equal(dst, b.data[off:off + m].to(torch.bfloat16))
        assert torch.equal(dst, dst0)
    # deterministic: a second run gives the same EMA, bit for bit
    o2, _, _, _, _ = _run_update(n, d)
    assert torch.equal(o2.ema, opt.ema)


def test_update_kernel_checks_its_ema_arguments():
    ops = _ops()
    from cst_captioning_amd.ops.adam import FlatAdam
    b = _RawBucket(64)
    opt = FlatAdam(b, ema_decay=0.5)

    def call(ema, decay):
        return ops.flat_adam_step(b.data, b.grad, opt.exp_avg, opt.exp_avg_sq, opt._partials,
                                  opt._scal, opt._no_skip, opt._hyper, 0.9, 0.999, 1e-8, 0.25, 1.0,
                                  0, EMPTY_META, [], ema, decay)
    for bad in (1.0, -0.1, float('nan')):
        with pytest.raises(RuntimeError):
            call(opt.ema, bad)
    with pytest.raises(RuntimeError):
        call(opt.ema[:32], 0.5)
    with pytest.raises(RuntimeError):
        call(opt.ema.double(), 0.5)
    with pytest.raises(RuntimeError):
        call(opt.ema.cpu(), 0.5)
    with pytest.raises(RuntimeError):
        ops.refresh_shadows(b.data, EMPTY_META, [], opt.ema[:32])
    with pytest.raises(RuntimeError):
        ops.refresh_shadows(b.data, EMPTY_META, [], b.data)  # overlap
    before = opt.ema.clone()
    call(torch.empty(0, device=DEV), 0.5)  # empty: off
    assert torch.equal(opt.ema, before)


def test_phase_two_on_a_slice():
    """The sharded update's phases on one rank's shard: the EMA slice follows
    the recurrence, the rest of the EMA buffer is untouched."""
    ops = _ops()
    from cst_captioning_amd.ops.adam import FlatAdam
    from cst_captioning_amd.parallel import FlatGradBucket
    d = 0.9
    g = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(*s, generator=g).to(DEV)) for s in SHAPES]
    b = FlatGradBucket(params, world_size=2, update='sharded')
    opt = FlatAdam(b, lr=1e-2, ema_decay=d)
    lo, hi = b.shard_range(1)
    assert hi - lo == 1600 and hi == b.data.numel()
    opt.ema.copy_(torch.randn(b.data.numel(), generator=g).to(DEV))  # (not the fixed point)
    ema0 = opt.ema.clone()
    p, m, v, e = b.data[lo:hi], opt.exp_avg[lo:hi], opt.exp_avg_sq[lo:hi], opt.ema[lo:hi]
    args = (0.9, 0.999, 1e-8, 0.25, 0.5)
    e64 = e.double().clone()
    M = max(float(p.abs().max()), float(e.abs().max()))
    outside_p = b.data[:lo].clone()
    for t in range(3):
        gshard = torch.randn(hi - lo, generator=g).to(DEV)
        ops.flat_adam_step(p, gshard, m, v, opt._partials, opt._scal, opt._no_skip, opt._hyper,
                           *args, 1, EMPTY_META, [])
        ops.flat_adam_step(p, gshard, m, v, opt._partials, opt._scal, opt._no_skip, opt._hyper,
                           *args, 2, EMPTY_META, [], e, d)
        e64 += (1 - d) * (p.double() - e64)
        M = max(M, float(p.abs().max()), float(e.abs().max()))
    assert opt.step_count == 3
    assert torch.equal(opt.ema[:lo], ema0[:lo]) and torch.equal(b.data[:lo], outside_p)
    err = float((e.double() - e64).abs().max())
    print('slice: max |e - e64| = %.3e, bound %.3e' % (err, ema_bound(M, d)))
    assert err <= ema_bound(M, d)
    assert not torch.equal(e, ema0[lo:hi])


# ------------------------------------------------------- swap-and-refresh ---
def _trainer(rnn_type='lstm', ema_decay=0.5, graph=0, rl=True, V=37, H=64, lr=1e-3, val=False,
             seed=0, drop=0.5, **kw):
    from cst_captioning_amd.cli import build_model
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import CaptionLoader, make_synthetic
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.train.trainer import Trainer
    B, S, L = 8, 5, 12
    ds = make_synthetic('msrvtt', num_videos=24, vocab_size=V, seq_length=L, feat_dims=[64, 32],
                        seed=0)
    opt = default_opts(vocab_size=V, seq_length=L, feat_dims=[64, 32], train_seq_per_img=S,
                       test_seq_per_img=S, batch_size=B, test_batch_size=10, rnn_size=H,
                       input_encoding_size=H, drop_prob_lm=drop, rnn_type=rnn_type,
                       use_rl=int(rl), use_rl_after=0, use_cst=0, use_mixer=1, mixer_from=1,
                       use_eos=1, impl='hip', cuda_graph=graph, learning_rate=lr,
                       ema_decay=ema_decay, beam_size=1, **kw)
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    torch.manual_seed(seed)
    dev = torch.device(DEV)
    model, engine = build_model(opt, dev, 'hip')
    assert engine is not None
    loader = CaptionLoader(ds, B, S, 'train', dev, seed=0)
    vl = CaptionLoader(ds, 10, S, 'test', dev) if val else None
    tr = Trainer(opt, model, loader, vl, DistContext(device=dev), engine)
    tr.rl_training = bool(rl)
    return tr, loader


def _clone_dsts(dsts):
    """Fresh destinations with the aliasing of the originals (the packed wx is
    the destination of two segments)."""
    seen, out = {}, []
    for d in dsts:
        if d.numel() == 0:
            out.append(d)
            continue
        if d.data_ptr() not in seen:
            seen[d.data_ptr()] = d.clone()
        out.append(seen[d.data_ptr()])
    return out


@pytest.mark.parametrize('rnn_type', ['lstm', 'gru'])
def test_swap_and_refresh_on_the_engine_shadows(rnn_type):
    """Shadow segments as DecoderEngine.shadow_spec builds them (H = E = 64):
    PLAIN (vocab head, embedding), GATES_IH with the video-column dst2,
    GATES_HH."""
    ops = _ops()
    tr, _ = _trainer(rnn_type)
    opt, b = tr.optimizer, tr.bucket
    meta, dsts = opt._shadow
    assert sorted(set(meta[:, 2].tolist())) == [0, 1, 2]
    ih = [k for k in range(meta.size(0)) if meta[k, 2] == 1][0]
    assert dsts[2 * ih + 1].numel() > 0, 'no video-column shadow'
    g = torch.Generator().manual_seed(5)
    opt.ema.copy_(b.data + 0.05 * torch.randn(b.data.numel(), generator=g).to(DEV))
    p0, e0 = b.data.clone(), opt.ema.clone()
    sh0 = [d.clone() for d in dsts]
    want = _clone_dsts(dsts)
    ops.refresh_shadows(e0, meta, want)  # the existing per-segment kernel
    opt.swap_ema()
    assert torch.equal(b.data, e0) and torch.equal(opt.ema, p0)
    changed = 0
    for got, w, old in zip(dsts, want, sh0):
        assert torch.equal(got, w)
        changed += int(got.numel() > 0 and not torch.equal(got, old))
    assert changed >= 4
    opt.swap_ema()
    assert torch.equal(b.data, p0) and torch.equal(opt.ema, e0)
    for got, old in zip(dsts, sh0):
        assert torch.equal(got, old)


@pytest.mark.parametrize('n', [3, 779])
def test_swap_and_refresh_tail_and_unaligned_segments(n):
    """n % 4 = 3 (a tail), segments at offsets 5, 137 and 521 (none divisible
    by 4), gate segments of a small LSTM (H = E = 8, 4 video columns) whose
    rows of 12 / 8 make float4s straddle rows, the token / video boundary and
    segments; a PLAIN segment over the tail."""
    ops = _ops()
    bf = dict(dtype=torch.bfloat16, device=DEV)
    empty = torch.empty(0, **bf)
    if n == 3:
        meta = torch.tensor([[0, 3, 0, 0, 0, 0, 0, 0]], dtype=torch.int64)
        dsts = [torch.zeros(3, **bf), empty]
    else:
        H = E = 8
        wx, wiv, whh = torch.zeros(4 * H, E + H, **bf), torch.zeros(4 * H, 4, **bf), \
            torch.zeros(4 * H, H, **bf)
        meta = torch.tensor([[5, 130, 0, 0, 0, 0, 0, 0],
                             [137, 4 * H * 12, 1, 12, H, E, 4, 0xE4],
                             [521, 4 * H * H, 2, H, H, E, H, 0xE4],
                             [773, 6, 0, 0, 0, 0, 0, 0]], dtype=torch.int64)
        assert 521 + 4 * H * H == 777 and 137 + 4 * H * 12 == 521
        dsts = [torch.zeros(130, **bf), empty, wx, wiv, wx, whh, torch.zeros(6, **bf), empty]
    g = torch.Generator().manual_seed(n)
    p, q = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    p0, q0 = p.clone(), q.clone()
    want_q, want_p = _clone_dsts(dsts), _clone_dsts(dsts)
    ops.refresh_shadows(q0, meta, want_q)
    ops.refresh_shadows(p0, meta, want_p)
    ops.refresh_shadows(p, meta, dsts, q)
    assert torch.equal(p, q0) and torch.equal(q, p0)
    for got, w in zip(dsts, want_q):
        assert torch.equal(got, w)
    assert any(float(w.float().abs().sum()) > 0 for w in want_q)
    ops.refresh_shadows(p, meta, dsts, q)
    assert torch.equal(p, p0) and torch.equal(q, q0)
    for got, w in zip(dsts, want_p):
        assert torch.equal(got, w)


# ------------------------------------------------------------ the trainer ---
def test_captured_step_keeps_the_ema():
    """SCST through the captured graph: eager warm-up, capture, 4 replays; the
    EMA follows the recurrence over the parameters read after every step."""
    ops = _ops()
    d = 0.9
    ops.reset_device_errors(0)
    tr, loader = _trainer(ema_decay=d, graph=1, V=500, H=128)
    opt, b = tr.optimizer, tr.bucket
    assert torch.equal(opt.ema, b.data)
    e64 = b.data.double().clone()
    M = float(b.data.abs().max())
    prev = b.data.clone()
    for t in range(6):
        tr.train_step(loader.get_batch(), 0)
        p = b.data.clone()
        assert not torch.equal(p, prev), 'step %d changed nothing' % t
        e64 += (1 - d) * (p.double() - e64)
        M = max(M, float(p.abs().max()), float(opt.ema.abs().max()))
        prev = p
        if t == 1:
            assert tr._graph is not None, 'the step was never captured'
    assert opt.step_count == 6 and int(opt.skipped()) == 0
    err = float((opt.ema.double() - e64).abs().max())
    print('captured: max |e - e64| = %.3e, bound %.3e' % (err, ema_bound(M, d)))
    assert err <= ema_bound(M, d)
    assert not torch.equal(opt.ema, b.data)
    assert ops.device_errors(0) == 0


def test_validation_with_the_ema_on_the_fused_engine():
    """validate() inside ema_weights() is validate() of a trainer without the
    EMA whose model was loaded with the averaged weights; leaving the context
    restores the parameters and every shadow bit for bit."""
    # (three XE steps at lr 5e-4: the weights have moved enough for the greedy
    # captions of the live and the averaged model to differ, and the synthetic
    # task has not yet collapsed both to the most frequent token)
    kw = dict(V=500, H=128, lr=5e-4, val=True, rl=False, graph=1, val_scorer='tokens', drop=0.0)
    a, loader = _trainer(ema_decay=0.5, **kw)
    for _ in range(3):  # eager, capture + replay, replay
        a.train_step(loader.get_batch(), 0)
    assert a._graph is not None
    eng = a.engine
    shadows = [eng.wx, eng.whh_q, eng.emb, eng.wlog, eng.wiv]
    p0, e0 = a.bucket.data.clone(), a.optimizer.ema.clone()
    sh0 = [s.clone() for s in shadows]
    assert not torch.equal(p0, e0)
    with a.ema_weights():
        assert torch.equal(a.bucket.data, e0)
        sd = {k: v.detach().clone() for k, v in a.model.state_dict().items()}
        res_ema = a.validate(a.val_loader)
    assert torch.equal(a.bucket.data, p0) and torch.equal(a.optimizer.ema, e0)
    for s, s0 in zip(shadows, sh0):
        assert torch.equal(s, s0)
    b, _ = _trainer(ema_decay=0.0, seed=1, **kw)
    assert b.optimizer.ema is None
    b.model.load_state_dict(sd)
    b.engine.refresh_weights()
    assert torch.equal(b.bucket.data[:b.bucket.numel], e0[:b.bucket.numel])
    res_ref = b.validate(b.val_loader)
    print('EMA scores', res_ema['scores'], 'reference', res_ref['scores'])
    assert torch.equal(torch.as_tensor(res_ema['sequences']), torch.as_tensor(res_ref['sequences']))
    assert res_ema['predictions'] == res_ref['predictions']
    assert res_ema['scores'] == res_ref['scores']
    # outside the context: the live model
    res_live = a.validate(a.val_loader)
    assert res_live['predictions'] != res_ema['predictions']
    # and training goes on from the live weights through the captured graph
    a.train_step(loader.get_batch(), 0)
    assert a.optimizer.step_count == 4
