"""The group objectives (``--rl_objective``), measured on one GPU in one process
by the method of ``scripts/microbench_mbr_mix.py``:

  * the fused forward + backward pair (``csrc/kernels/loss.hip`` group
    objectives, through the bare extension entry points) at ``B=64, S=20,
    T=28`` for each objective, beside ``GroupCriterion`` (PyTorch ops on the
    GPU, eager, forward + autograd backward) on the same inputs: HIP-event
    time per call, windows of ``--reps`` back-to-back calls, the two taking
    turns.  A call includes the binding's argument conversion and the
    allocation of the results, so the figure is an upper bound of the kernels'
    time; the host time to enqueue one call is reported beside it.  The number
    of device launches (kernels and memsets) of one call of each, counted with
    the profiler in a pass of its own, and the largest difference between the
    two gradients;
  * the replayed training step of the flagship model (MSR-VTT shape, batch
    64 x 20 captions, fused engine, captured HIP graph) with ``--rl_objective
    risk`` beside the CST step with the samples' own scores as baseline
    (``--use_cst 1 --scb_baseline 2``) and the SCST step, one trainer per
    recipe: windows of ``--steps`` steps, the recipes taking turns.

Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cst_captioning_amd import _ext
from cst_captioning_amd.cli import build_model
from cst_captioning_amd.config import default_opts
from cst_captioning_amd.data import CaptionLoader, make_synthetic
from cst_captioning_amd.models import GroupCriterion
from cst_captioning_amd.parallel import DistContext
from cst_captioning_amd.train.trainer import Trainer

OBJECTIVES = ('risk', 'softmax_margin', 'multi_margin')
KIND = {'risk': 1, 'softmax_margin': 2, 'multi_margin': 3}


def stats(v, nd=2):
    return [round(float(np.median(v)), nd), round(min(v), nd), round(max(v), nd)]


def launches(fn):
    """Device launches (kernels, memsets, copies) of one call of fn."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return int(sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA))


def kernel_part(dev, reps, rounds, B=64, S=20, T=28):
    torch.manual_seed(0)
    R = B * S
    seq = torch.randint(0, 50, (R, T), device=dev)
    seq[torch.rand(R, T, device=dev) < 0.1] = 0
    lp = -torch.rand(R, T, device=dev) * 5
    scores = torch.randint(0, 12, (B, S), device=dev).float() / 8.0
    flat = scores.reshape(-1).contiguous()
    ops, none, one = _ext.ops(), torch.empty(0, device=dev), torch.ones(1, device=dev)
    crits = {o: GroupCriterion(o) for o in OBJECTIVES}
    lpg = lp.clone().requires_grad_(True)

    def fused(o):
        loss, out, reward, w = ops.cst_loss_forward(seq, lp, flat, none, S, 0, KIND[o], 1.0, 1.0)
        return ops.scst_loss_backward(seq, w, out, one, w)

    def eager(o):
        lpg.grad = None
        crits[o](seq, lpg, scores)[0].backward()
        return lpg.grad

    todo = [(f, o) for o in OBJECTIVES for f in (fused, eager)]
    for f, o in todo:
        for _ in range(5):
            f(o)
    times = {k: [] for k in todo}
    enq = {k: [] for k in todo}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for k in todo:
            f, o = k
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for _ in range(reps):
                f(o)
            enq[k].append((time.perf_counter() - t0) * 1e6 / reps)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    out = {'shape': [B, S, T]}
    for o in OBJECTIVES:
        out[o] = {
            'fused_pair_us': stats(times[(fused, o)]),
            'fused_host_enqueue_us': stats(enq[(fused, o)]),
            'torch_eager_us': stats(times[(eager, o)]),
            'torch_host_enqueue_us': stats(enq[(eager, o)]),
            'grad_max_abs_diff': float((fused(o) - eager(o)).abs().max())}
    return out, fused, eager


def trainer_for(ds, dev, seed, **over):
    B, S = 64, 20
    kw = dict(batch_size=B, train_seq_per_img=S, test_seq_per_img=S, rnn_size=512,
              input_encoding_size=512, drop_prob_lm=0.5, learning_rate=1e-4, grad_clip=0.25,
              eval_metric='CIDEr', max_epochs=10 ** 9, print_log_interval=0, use_rl=1,
              use_rl_after=0, use_cst=0, use_mixer=1, mixer_from=1, use_eos=1, expand_feat=1,
              scb_captions=S, impl='hip', seed=seed, loglevel='WARNING', save_last=0,
              cuda_graph=1)
    kw.update(over)
    opt = default_opts(**kw)
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    opt.vocab_size, opt.seq_length, opt.feat_dims = ds.vocab_size, ds.seq_length, ds.feat_dims
    torch.manual_seed(seed)
    model, engine = build_model(opt, dev, 'hip')
    assert engine is not None
    loader = CaptionLoader(ds, B, S, 'train', dev, seed=seed)
    tr = Trainer(opt, model, loader, None, DistContext(device=dev), engine)
    tr.rl_training = True
    return tr, loader


def step_part(dev, videos, steps, rounds, warmup):
    ds = make_synthetic('msrvtt', num_videos=videos, vocab_size=10509, seed=123)
    recipes = {'risk': dict(rl_objective='risk'),
               'cst_scb2': dict(use_cst=1, scb_baseline=2),
               'scst': dict()}
    trs = {k: trainer_for(ds, dev, 123, **over) for k, over in recipes.items()}
    for tr, loader in trs.values():
        for _ in range(warmup):
            tr.train_step(loader.get_batch(), 0)
        torch.cuda.synchronize()
        assert tr._graph is not None
    times = {k: [] for k in trs}
    for _ in range(rounds):
        for k, (tr, loader) in trs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                out = tr.train_step(loader.get_batch(), 0)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / steps)
            assert bool(torch.isfinite(out['loss']))
    return {'videos': videos, 'batch': [64, 20],
            'step_ms': {k: stats(v, 3) for k, v in times.items()}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=200)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--videos', type=int, default=6513)
    p.add_argument('--steps', type=int, default=100)
    p.add_argument('--warmup', type=int, default=8)
    p.add_argument('--skip_step', action='store_true')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('needs a GPU: the kernels and the training step are measured there')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    out = {'format': 'us / ms per call or step: [median, min, max] of %d alternating windows '
                     '(%d calls; %d steps)' % (a.rounds, a.reps, a.steps)}
    out['kernel'], fused, eager = kernel_part(dev, a.reps, a.rounds)
    print(json.dumps(out['kernel']), file=sys.stderr, flush=True)
    if not a.skip_step:
        out['step'] = step_part(dev, a.videos, a.steps, a.rounds, a.warmup)
        print(json.dumps(out['step']), file=sys.stderr, flush=True)
    for o in OBJECTIVES:  # (the profiler's pass: after everything timed)
        out['kernel'][o]['fused_launches'] = launches(lambda: fused(o))
        out['kernel'][o]['torch_launches'] = launches(lambda: eager(o))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
