"""Data parallelism without a cluster (SURVEY.md §4.2 "Distributed"):
torchrun with the gloo backend, world sizes 1, 2 and 4 on the CPU.

  * C1: rank 0's parameters are broadcast (ranks start from different seeds);
  * C2: the all-reduced gradient equals the gradient of the mean of the
    per-shard losses computed in one process;
  * parameters stay bit-identical across ranks after optimizer steps;
  * C4: sharded validation + all-gather reproduces the single-rank result;
  * the bf16-wire reduction (all-to-all + fp32 sum + all-gather) matches the
    reference gradient to bf16 rounding and keeps the ranks in lock-step.
"""
import os
import socket
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, out, wire='fp32', update='allreduce', mode='xe'):
    env = dict(os.environ)
    env['CSTCAP_TEST_MODE'] = mode
    env['CSTCAP_TEST_WIRE'] = wire
    env['CSTCAP_TEST_DPUPDATE'] = update
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    env['CUDA_VISIBLE_DEVICES'] = ''  # CPU ranks (gloo)
    env['HIP_VISIBLE_DEVICES'] = ''  # (set on ROCm hosts, it outranks the CUDA_ name)
    env['OMP_NUM_THREADS'] = '1'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
           '--nproc-per-node', str(world), '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(HERE, 'dist_worker.py'), out]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return torch.load(out, weights_only=False)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp('dist')
    return {w: _run(w, str(d / ('w%d.pt' % w))) for w in (1, 2, 4)}


@pytest.fixture(scope='module')
def runs_bf16(tmp_path_factory):
    d = tmp_path_factory.mktemp('dist_bf16')
    return {w: _run(w, str(d / ('w%d.pt' % w)), 'bf16') for w in (2, 4)}


@pytest.fixture(scope='module')
def runs_sharded(tmp_path_factory):
    d = tmp_path_factory.mktemp('dist_sharded')
    return {w: _run(w, str(d / ('w%d.pt' % w)), update='sharded') for w in (2, 4)}


def _reference_grad(world, with_abs=False):
    """Gradient of mean_k(loss on shard k), one process (and, with_abs, the
    mean of the per-shard gradients' magnitudes)."""
    sys.path.insert(0, HERE)
    import dist_worker as W
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.train.trainer import Trainer
    dev = torch.device('cpu')
    opt, model, engine, _, _ = W.build(0, world, dev)
    grads = mags = None
    for k in range(world):
        _, _, _, loader, _ = W.build(k, world, dev)
        tr = Trainer(opt, model, loader, None, DistContext(device=dev), engine)
        tr.optimizer.zero_grad()
        loss, _ = tr.xe_loss(loader.get_batch())
        loss.backward()
        g = tr.bucket.grad.clone() / world
        grads = g if grads is None else grads + g
        mags = g.abs() if mags is None else mags + g.abs()
    if with_abs:
        return model, grads, mags
    return model, grads


def reference_scst_grad(world, p1, dev):
    """Mean over shards k of the SCST gradient of rank k's second batch at
    the parameters p1, one process, with rank k's sampling seeds
    (dist_worker.fix_seeds) -- what the all-reduce must reproduce."""
    sys.path.insert(0, HERE)
    import dist_worker as W
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.train.trainer import Trainer
    grads = None
    for k in range(world):
        opt, model, engine, loader, _ = W.build(k, world, dev)
        tr = Trainer(opt, model, loader, None, DistContext(device=dev), engine)
        n = min(tr.bucket.data.numel(), p1.numel())
        with torch.no_grad():
            tr.bucket.data[:n].copy_(p1[:n].to(dev))
        if engine is not None:
            engine.refresh_weights()
        W.fix_seeds(tr, k, dev)
        tr.rl_training = True
        loader.get_batch()  # the worker's first (warm-up) batch
        data = loader.get_batch()
        mixer_from, scb = tr._schedules(0)
        torch.manual_seed(999 + k)
        tr._forward_backward(data, mixer_from, scb)
        g = tr.bucket.grad.detach().clone()[:n] / world
        grads = g if grads is None else grads + g
    return grads


@pytest.mark.parametrize('world', [2, 4])
def test_scst_step_allreduce_matches_per_shard_mean(tmp_path, world):
    """The headline recipe under data parallelism: every rank samples its own
    rollout, decodes its greedy baseline and scores both with CIDEr-D on its
    own shard; the all-reduced gradient equals the mean of the per-shard SCST
    gradients (reference train.py:167-218 / utils.py:169-226 per shard), and
    the ranks stay identical after the update."""
    r = _run(world, str(tmp_path / ('scst%d.pt' % world)), mode='scst')
    ref = reference_scst_grad(world, r['p1'], torch.device('cpu'))
    n = ref.numel()
    torch.testing.assert_close(r['grad'][:n], ref, rtol=1e-4, atol=1e-7)
    assert r['same_after_steps']
    assert ref.abs().sum() > 0
    rw = r['rewards']
    assert len(rw) == world and not all(torch.equal(rw[0], x) for x in rw[1:])


def test_broadcast_and_allreduce(runs):
    r2 = runs[2]
    model, ref = _reference_grad(2)
    # C1: rank 0's init (seed 1234) everywhere; the reference model was built
    # with the same seed, so its init matches
    init_ref = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    torch.testing.assert_close(r2['init'], init_ref, rtol=0, atol=0)
    # (the bucket's zero padding depends on the world size)
    torch.testing.assert_close(r2['grad'][:ref.numel()], ref, rtol=1e-5, atol=1e-7)
    assert r2['same_after_steps']


def test_allreduce_world4(runs):
    r4 = runs[4]
    _, ref = _reference_grad(4)
    torch.testing.assert_close(r4['grad'][:ref.numel()], ref, rtol=1e-5, atol=1e-7)
    assert r4['same_after_steps']


def test_nan_on_one_rank_skips_everywhere(runs):
    # the skip flag travels in the gradient bucket's status slot
    assert runs[1]['nan_skip_all'] and runs[2]['nan_skip_all'] and runs[4]['nan_skip_all']


def test_log_scalars_are_rank_means(runs):
    """C3: the log line's loss / reward / m / b are averaged over ranks."""
    for w in (1, 2, 4):
        mean = (w - 1) / 2.0
        assert runs[w]['logged'] == pytest.approx([mean + 1, mean, 2 * mean, -mean])
        # a real step: the logged XE loss is the mean of the per-rank losses
        xl = runs[w]['xe_losses']
        assert len(xl) == w
        assert runs[w]['xe_logged'] == pytest.approx([sum(xl) / w], rel=1e-6)
    assert len(set(runs[4]['xe_losses'])) > 1  # shards differ, so the test has teeth


def test_sharded_validation_matches_single_rank(runs):
    p1, p2 = runs[1]['predictions'], runs[2]['predictions']
    assert len(p1) == 8  # synthetic val split: max(8, 24 // 10) videos
    assert p1 == p2 == runs[4]['predictions']  # same ids, same order, same captions
    # (the XE 'Loss' depends on which seq_per_img captions each rank draws, as in
    # the reference's random caption selection, so only the beam outputs are compared)
    assert runs[1]['world'] == 1 and runs[2]['world'] == 2


@pytest.mark.parametrize('world', [2, 4])
def test_bf16_wire_reduction(runs_bf16, world):
    r = runs_bf16[world]
    _, ref, mag = _reference_grad(world, with_abs=True)
    g = r['grad']
    assert g.numel() % (64 * world) == 0  # the buffer splits into equal chunks
    n = min(ref.numel(), g.numel())
    ref, mag = ref[:n], mag[:n]
    # one bf16 rounding (relative 2^-9) of every rank's input and of the sum
    err = (g[:n] - ref).abs()
    bound = 2 ** -8 * (mag + ref.abs()) + 1e-9
    assert (err <= bound).all(), (err - bound).max()
    assert err.max() > 0  # the wire really is bf16
    assert r['same_after_steps'] and r['nan_skip_all']
    assert r['xe_logged'] == pytest.approx([sum(r['xe_losses']) / world], rel=1e-6)


@pytest.mark.parametrize('world', [2, 4])
def test_sharded_update_matches_allreduce(runs, runs_sharded, world):
    """--dp_update sharded (reduce-scatter -> Adam on the rank's 1/N shard with
    the global clip norm -> all-gather) gives the parameters and the Adam
    moments of the all-reduce path, keeps the ranks identical, and skips
    everywhere when one rank's loss is NaN.  (Not bit-equal: the norm and the
    gradient sums are accumulated in another order.)"""
    a, b = runs[world], runs_sharded[world]
    # (Adam's m / sqrt(v) magnifies last-bit differences of near-zero gradients:
    # atol 1e-6 = 0.1 % of one lr = 1e-3 step)
    torch.testing.assert_close(b['params_after'], a['params_after'], rtol=1e-5, atol=1e-6)
    for x, y in zip(b['moments'], a['moments']):
        torch.testing.assert_close(x, y, rtol=1e-4, atol=1e-10)
    assert b['same_after_steps'] and b['nan_skip_all']
    assert b['steps_done'] == a['steps_done'] and b['skipped'] == a['skipped'] == 1
    assert b['xe_logged'] == pytest.approx([sum(b['xe_losses']) / world], rel=1e-6)
