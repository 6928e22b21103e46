"""EMA of the parameters kept by the Adam pass (``--ema_decay``), CPU side:
FlatAdam's torch path against an fp64 recurrence, the state dict, the flag,
the trainer (validation / best checkpoint on the averaged weights, the
``_last.pth`` sidecar on the live ones, exact resume) and the sharded update
under gloo.

Tolerance against the fp64 recurrence ``e64 += (1 - d) (p - e64)`` over the
optimizer's own parameter trajectory: a step adds at most about 5 fp32
roundings of magnitude M (the largest ``|p|`` or ``|e|`` seen) and every
earlier error shrinks by d per step, so ``|e - e64| <= 5 * 2^-24 * M / (1 - d)``
(atol, rtol 0)."""
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from cst_captioning_amd.cli import build_model, load_splits
from cst_captioning_amd.config import build_parser, parse_opts
from cst_captioning_amd.data import CaptionLoader
from cst_captioning_amd.ops.adam import FlatAdam
from cst_captioning_amd.parallel import DistContext, FlatGradBucket
from cst_captioning_amd.train import checkpoint as ckpt
from cst_captioning_amd.train.trainer import Trainer

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHAPES = [(37, 5), (101,), (8, 8), (3,)]


def _adam(ema_decay, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in SHAPES]
    b = FlatGradBucket(params)
    return b, FlatAdam(b, lr=1e-2, ema_decay=ema_decay)


def _grads(n, steps, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for _ in range(steps)]


def ema_bound(M, d):
    return 5 * 2.0 ** -24 * M / (1 - d)


def test_torch_path_matches_fp64_recurrence_and_skips():
    d, steps = 0.9, 6
    b, opt = _adam(d)
    grads = _grads(b.grad.numel(), steps)
    grads[4][7] = float('nan')  # a NaN gradient: the norm guard skips step 4
    e64 = b.data.double().clone()
    M = float(b.data.abs().max())
    applied = 0
    for t in range(steps):
        before_e, before_p = opt.ema.clone(), b.data.clone()
        b.grad.copy_(grads[t])
        opt.step(torch.tensor(True) if t == 2 else None)  # step 2: skipped by the flag
        if t in (2, 4):
            assert torch.equal(opt.ema, before_e), 'a skipped step touched the EMA'
            assert torch.equal(b.data, before_p)
        else:
            e64 += (1 - d) * (b.data.double() - e64)
            applied += 1
        M = max(M, float(b.data.abs().max()), float(opt.ema.abs().max()))
    assert applied == 4 and opt.step_count == 4 and int(opt.skipped()) == 2
    err = float((opt.ema.double() - e64).abs().max())
    print('max |e - e64| = %.3e, bound %.3e' % (err, ema_bound(M, d)))
    assert err <= ema_bound(M, d)
    assert not torch.equal(opt.ema, b.data)


def test_torch_path_ema_has_no_side_effects_and_swaps_back():
    b0, o0 = _adam(0.0)
    b1, o1 = _adam(0.9)
    assert o0.ema is None and torch.equal(o1.ema, b1.data)
    grads = _grads(b0.grad.numel(), 5)
    for t, g in enumerate(grads):
        for b, o in ((b0, o0), (b1, o1)):
            b.grad.copy_(g)
            o.step(torch.tensor(True) if t == 1 else None)
    assert torch.equal(b0.data, b1.data)
    assert torch.equal(o0.exp_avg, o1.exp_avg)
    assert torch.equal(o0.exp_avg_sq, o1.exp_avg_sq)
    p, e = b1.data.clone(), o1.ema.clone()
    o1.swap_ema()
    assert torch.equal(b1.data, e) and torch.equal(o1.ema, p)
    # the parameters are views of the flat buffer: the model sees the EMA
    assert torch.equal(b1.params[0].detach().reshape(-1), e[:b1.slices[0][1]])
    o1.swap_ema()
    assert torch.equal(b1.data, p) and torch.equal(o1.ema, e)
    with pytest.raises(RuntimeError):
        o0.swap_ema()


def test_state_dict_carries_the_ema_only_when_enabled():
    b0, o0 = _adam(0.0)
    assert 'ema' not in o0.state_dict() and 'ema_decay' not in o0.state_dict()
    b1, o1 = _adam(0.9)
    for g in _grads(b1.grad.numel(), 3):
        b1.grad.copy_(g)
        o1.step()
    s = o1.state_dict()
    assert s['ema_decay'] == 0.9 and torch.equal(s['ema'], o1.ema)
    s = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in s.items()}
    b2, o2 = _adam(0.9, seed=5)
    b2.data.copy_(b1.data)
    o2.load_state_dict(s)
    assert torch.equal(o2.ema, o1.ema) and not torch.equal(o2.ema, b2.data)
    assert torch.equal(o2.exp_avg, o1.exp_avg) and o2.step_count == 3
    # a state written without an EMA: the average starts at the loaded weights
    b3, o3 = _adam(0.9, seed=6)
    b3.data.copy_(b1.data)
    o3.load_state_dict({k: v for k, v in s.items() if k not in ('ema', 'ema_decay')})
    assert torch.equal(o3.ema, b3.data)
    # and an EMA state loads into an optimizer without one
    o0.load_state_dict(s)
    assert o0.ema is None
    with pytest.raises(ValueError):
        FlatAdam(b0, ema_decay=1.0)


@pytest.mark.parametrize('bad', ['-0.1', '1.0', '1.5', 'nan'])
def test_flag_rejects_values_outside_the_unit_interval(bad, capsys):
    with pytest.raises(SystemExit):
        build_parser().parse_args(['--ema_decay=' + bad])
    assert '--ema_decay' in capsys.readouterr().err


def test_flag_parses():
    assert parse_opts([]).ema_decay == 0.0
    assert parse_opts(['--ema_decay', '0']).ema_decay == 0.0
    assert parse_opts(['--ema_decay', '0.999']).ema_decay == 0.999


# ---------------------------------------------------------------- trainer ---
BASE = ['--synthetic', 'msvd', '--synthetic_videos', '24', '--synthetic_vocab', '200',
        '--seq_length', '8', '--rnn_size', '64', '--input_encoding_size', '64',
        '--feat_dims', '16', '8', '--batch_size', '6', '--train_seq_per_img', '3',
        '--test_batch_size', '8', '--test_seq_per_img', '3', '--beam_size', '1',
        '--impl', 'torch', '--loglevel', 'WARNING', '--print_log_interval', '0',
        '--learning_rate', '2e-3', '--drop_prob_lm', '0.1', '--save_checkpoint_from', '1',
        '--eval_metric', 'CIDEr', '--ema_decay', '0.5']


def _trainer(model_file, max_epochs, seed=0):
    opt = parse_opts(BASE + ['--max_epochs', str(max_epochs), '--model_file', model_file])
    torch.manual_seed(seed)
    np.random.seed(seed)
    tr, va, _ = load_splits(opt)
    ctx = DistContext(device=torch.device('cpu'))
    loader = CaptionLoader(tr, opt.batch_size, opt.train_seq_per_img, 'train', 'cpu',
                           seed=opt.seed)
    opt.vocab = loader.get_vocab()
    opt.vocab_size = loader.get_vocab_size()
    opt.seq_length = loader.get_seq_length()
    opt.feat_dims = loader.get_feat_dims()
    opt.history_file = model_file.replace('.pth', '_history.json', 1)
    model, engine = build_model(opt, torch.device('cpu'))
    val = CaptionLoader(va, opt.test_batch_size, opt.test_seq_per_img, 'test', 'cpu')
    return Trainer(opt, model, loader, val, ctx, engine)


def _spy(tr):
    """Record (epoch, live weights, EMA) at every entry of ema_weights() and
    the same pair after it was left."""
    seen, inner = [], tr.ema_weights

    import contextlib

    @contextlib.contextmanager
    def spied():
        rec = {'epoch': tr.infos['epoch'], 'p': tr.bucket.data.clone(),
               'e': tr.optimizer.ema.clone()}
        with inner():
            rec['p_inside'] = tr.bucket.data.clone()
            yield
        rec['p_after'], rec['e_after'] = tr.bucket.data.clone(), tr.optimizer.ema.clone()
        seen.append(rec)

    tr.ema_weights = spied
    return seen


def _model_flat(tr, state):
    """A checkpoint's ``model`` entry laid out like the trainer's flat buffer."""
    flat = torch.zeros_like(tr.bucket.data)
    names = {id(p): k for k, p in tr.model.named_parameters()}
    for p, (off, n) in zip(tr.bucket.params, tr.bucket.slices):
        flat[off:off + n] = state[names[id(p)]].reshape(-1)
    return flat


@pytest.fixture(scope='module')
def full_run(tmp_path_factory):
    """The uninterrupted run: 2 epochs of 4 iterations, validated after each."""
    mf = str(tmp_path_factory.mktemp('ema_full') / 'm.pth')
    tr = _trainer(mf, 2)
    seen = _spy(tr)
    infos = tr.train()
    return tr, seen, infos, mf


def test_trainer_validates_and_saves_the_averaged_weights(full_run):
    tr, seen, infos, mf = full_run
    assert [r['epoch'] for r in seen] == [1, 2]
    for r in seen:
        # inside: the parameters are the EMA; after: everything is back, bit for bit
        assert torch.equal(r['p_inside'], r['e']) and not torch.equal(r['e'], r['p'])
        assert torch.equal(r['p_after'], r['p']) and torch.equal(r['e_after'], r['e'])
    best = [r for r in seen if r['epoch'] == infos['best_epoch']][0]
    saved = _model_flat(tr, ckpt.load_checkpoint(mf)['model'])
    assert torch.equal(saved, best['e']), 'the best checkpoint does not hold the EMA weights'
    assert not torch.equal(saved, best['p'])
    # the sidecar: live weights, the EMA inside the optimizer state
    s = ckpt.load_checkpoint(ckpt.last_path(mf))
    assert torch.equal(_model_flat(tr, s['model']), tr.bucket.data)
    assert torch.equal(_model_flat(tr, s['model']), seen[-1]['p'])
    assert torch.equal(s['optimizer']['ema'], tr.optimizer.ema)
    assert s['optimizer']['ema_decay'] == 0.5
    assert torch.equal(tr.optimizer.ema, seen[-1]['e'])


def test_validate_leaves_the_live_weights_alone(full_run):
    tr = full_run[0]
    p, e = tr.bucket.data.clone(), tr.optimizer.ema.clone()
    with tr.ema_weights():
        tr.validate(tr.val_loader)
    assert torch.equal(tr.bucket.data, p) and torch.equal(tr.optimizer.ema, e)


def test_exact_resume_restores_the_ema(full_run, tmp_path):
    """Interrupted after epoch 1 (sidecar written), rebuilt from another seed
    and resumed: the same live weights and the same EMA as the uninterrupted
    run (the pattern of test_train_integration.py's sidecar test)."""
    ref = full_run[0]
    mf = str(tmp_path / 'm.pth')
    b = _trainer(mf, 1)
    b.train()
    assert b.infos['epoch'] == 1 and os.path.exists(ckpt.last_path(mf))
    assert 'ema' in ckpt.load_checkpoint(ckpt.last_path(mf))['optimizer']
    c = _trainer(mf, 2, seed=99)
    assert not torch.equal(c.bucket.data, b.bucket.data)
    c.train()
    assert c.infos['epoch'] == 2
    assert torch.equal(c.bucket.data, ref.bucket.data)
    assert torch.equal(c.optimizer.ema, ref.optimizer.ema)


def test_warm_start_resets_the_ema(full_run, tmp_path):
    """--start_from a best checkpoint (no sidecar): the average starts at the
    loaded weights."""
    src = full_run[3]
    shutil.copy(src, str(tmp_path / 'warm.pth'))
    tr = _trainer(str(tmp_path / 'new.pth'), 3, seed=7)
    tr.opt.start_from = str(tmp_path / 'warm.pth')
    assert not torch.equal(tr.optimizer.ema, _model_flat(tr, ckpt.load_checkpoint(src)['model']))
    tr.resume()
    assert torch.equal(tr.optimizer.ema, tr.bucket.data)
    assert torch.equal(tr.bucket.data, _model_flat(tr, ckpt.load_checkpoint(src)['model']))


# ------------------------------------------------------------------- gloo ---
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_sharded_update_ema_under_gloo(tmp_path):
    """World size 2, --dp_update sharded, 3 steps: inside ema_weights() every
    rank's full parameter buffer is the EMA of a single-process FlatAdam fed
    the summed gradient (tolerance of test_dist.py's sharded-versus-all-reduce
    parameters: the norm and the sums are accumulated in another order); after
    it each rank's own parameter and EMA shards are bit-equal to before."""
    out = str(tmp_path / 'ema_dist.pt')
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    env['CUDA_VISIBLE_DEVICES'] = ''
    env['HIP_VISIBLE_DEVICES'] = ''
    env['OMP_NUM_THREADS'] = '1'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()),
           os.path.join(HERE, 'ema_dist_worker.py'), out]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = torch.load(out, weights_only=False)
    ranks = res['ranks']
    assert len(ranks) == 2
    # single process: the same initial weights, the summed gradients, 1 / N in the update
    init, n = res['init'], res['numel']
    p = torch.nn.Parameter(init[:n].clone())
    b = FlatGradBucket([p])
    o = FlatAdam(b, lr=res['lr'], grad_clip=res['grad_clip'], ema_decay=res['ema_decay'])
    o.grad_scale = 0.5
    for g in res['grad_sums']:
        b.grad.zero_()
        b.grad[:n].copy_(g[:n])
        o.step()
    assert not torch.equal(o.ema[:n], b.data[:n])
    for k, rk in enumerate(ranks):
        torch.testing.assert_close(rk['inside'][:n], o.ema[:n], rtol=1e-5, atol=1e-6)
        assert torch.equal(rk['inside'], ranks[0]['inside'])
        assert torch.equal(rk['p_shard_after'], rk['p_shard_before'])
        assert torch.equal(rk['e_shard_after'], rk['e_shard_before'])
        torch.testing.assert_close(rk['live_after'][:n], b.data[:n], rtol=1e-5, atol=1e-6)
        assert torch.equal(rk['live_after'], rk['live_before'])
