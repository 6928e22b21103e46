"""Consensus (MBR) decoding under a mixed utility (``--mbr_mix``), measured on one
GPU in one process by the method of ``scripts/microbench_mbr.py``:

  * the peer-mix kernel (``csrc/kernels/peer_mix.hip``) at ``B=32, G=21, T=29``
    and ``B=64, G=64, T=31`` for the weights (1, 5, 5), (1, 0, 0) and (0, 5, 5),
    beside the peer CIDEr-D kernel (``cider_score(..., group=G)``) as the floor:
    HIP-event time per call of the bare ops on prepared tensors, windows of
    ``--reps`` back-to-back calls, shapes and ops taking turns.  A call is the
    launch plus the binding's argument conversion and the allocation of the
    results, so the figure is an upper bound of the kernel's time; the host time
    to enqueue one call is reported beside it.  The native CPU twin on the same
    inputs (host clock, one run);
  * ``Trainer.validate`` end to end on a synthetic MSR-VTT-shaped split (fused
    engine, ``--val_scorer tokens``, test batch 64, beam 5, ``--decode mbr`` at
    ``N = 20``) without and with ``--mbr_mix CIDEr:1,Bleu_4:5,ROUGE_L:5``:
    ``--runs`` runs each, alternating, after one untimed run of each.

Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from cst_captioning_amd import _ext
from cst_captioning_amd.cli import build_model
from cst_captioning_amd.config import default_opts
from cst_captioning_amd.data import CaptionLoader, make_synthetic
from cst_captioning_amd.ops.mbr import PeerCiderD, PeerMix
from cst_captioning_amd.parallel import DistContext
from cst_captioning_amd.train.trainer import Trainer
from microbench_mbr import SHAPES, VOCAB, pools, stats

WEIGHTS = ((1.0, 5.0, 5.0), (1.0, 0.0, 0.0), (0.0, 5.0, 5.0))
MIX = 'CIDEr:1,Bleu_4:5,ROUGE_L:5'


def wname(w):
    return 'mix_%g_%g_%g' % w


def kernel_part(ds, dev, reps, rounds):
    gpu = PeerCiderD(ds.df, use_eos=1, device=dev, backend='gpu')
    data = {s: torch.from_numpy(pools(ds, *s, seed=1)) for s in SHAPES}
    on_dev = {s: h.to(dev) for s, h in data.items()}
    ops, none = _ext.ops(), torch.zeros(0, dtype=torch.long, device=dev)

    def call(s, op):  # the bare ops: no Python-side checks or copies
        if op == 'cider_peer':
            return ops.cider_score(on_dev[s], none, gpu._tables, gpu.log_ref_len, 1, group=s[1])
        return ops.metric_score('mix', on_dev[s], none, None, 1,
                                cider_tables=gpu._tables if op[0] else None,
                                log_ref_len=gpu.log_ref_len, weights=list(op), group=s[1])

    todo = [(s, op) for s in SHAPES for op in ('cider_peer',) + WEIGHTS]
    for s, op in todo:
        for _ in range(5):
            call(s, op)
    times = {k: [] for k in todo}
    enq = {k: [] for k in todo}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for k in todo:
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for _ in range(reps):
                call(*k)
            enq[k].append((time.perf_counter() - t0) * 1e6 / reps)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    out = {}
    for s in SHAPES:
        B, G, T = s
        o = {'mean_tokens': round(float((data[s] > 0).sum(1).float().mean()), 1),
             'cider_peer': {'op_us': stats(times[(s, 'cider_peer')]),
                            'host_enqueue_us': stats(enq[(s, 'cider_peer')])}}
        for w in WEIGHTS:
            cpu = PeerMix(ds.df, w, use_eos=1, backend='cpu')
            t0 = time.perf_counter()
            twin = cpu.score_both(data[s], G)
            cpu_ms = (time.perf_counter() - t0) * 1e3
            got = call(s, w)
            o[wname(w)] = {
                'op_us': stats(times[(s, w)]), 'host_enqueue_us': stats(enq[(s, w)]),
                'cpu_twin_ms': round(cpu_ms, 2),
                'gpu_vs_twin_max_abs_parts': [float((got[1][:, c].cpu() - twin[1][:, c]).abs().max())
                                              for c in range(3)],
                'out_max': float(twin[0].max())}
        out['B%d_G%d_T%d' % s] = o
    return out


def validate_part(n_videos, runs, dev, N):
    ds = make_synthetic('msrvtt', num_videos=n_videos, vocab_size=VOCAB, seed=123)
    B, S = 64, 20
    opt = default_opts(batch_size=B, train_seq_per_img=S, test_batch_size=B, test_seq_per_img=S,
                       rnn_size=512, input_encoding_size=512, drop_prob_lm=0.5, beam_size=5,
                       impl='hip', seed=123, loglevel='WARNING', save_last=0, max_epochs=1,
                       print_log_interval=0, val_scorer='tokens', decode='mbr', mbr_samples=N)
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    opt.vocab_size, opt.seq_length, opt.feat_dims = ds.vocab_size, ds.seq_length, ds.feat_dims
    torch.manual_seed(123)
    model, engine = build_model(opt, dev, 'hip')
    assert engine is not None
    train = CaptionLoader(ds, B, S, 'train', dev, seed=123)
    val = CaptionLoader(ds, B, S, 'test', dev)
    tr = Trainer(opt, model, train, val, DistContext(device=dev), engine)
    scorers = {'mbr_cider': tr.mbr_scorer}
    opt.mbr_mix = MIX
    scorers['mbr_mix'] = tr._build_mbr_scorer()
    assert isinstance(scorers['mbr_mix'], PeerMix) and scorers['mbr_mix'].backend == 'gpu'

    def validate(mode):
        tr.mbr_scorer = scorers[mode]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tr.validate(val)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    res = {'videos': n_videos, 'batches': -(-n_videos // B), 'mbr_samples': N, 'beam_size': 5,
           'mbr_mix': MIX}
    warm = {m: validate(m) for m in scorers}  # untimed
    for m in scorers:
        res['mean_mbr_score_' + m] = round(float(np.mean(
            [p['mbr_score'] for p in warm[m][1]['predictions']])), 4)
    times = {m: [] for m in scorers}
    for _ in range(runs):
        for m in scorers:
            times[m].append(validate(m)[0])
    res['validate_ms'] = {m: stats(v) for m, v in times.items()}
    res['extra_ms'] = round(float(np.median(times['mbr_mix']) - np.median(times['mbr_cider'])), 2)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--videos', type=int, default=497)
    p.add_argument('--runs', type=int, default=5)
    p.add_argument('--reps', type=int, default=200)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--samples', type=int, default=20)
    p.add_argument('--skip_validate', action='store_true')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('needs a GPU: the kernel and the decode are measured there')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    ds = make_synthetic('msrvtt', num_videos=64, vocab_size=VOCAB, seed=123, feat_dims=[8])
    out = {'format': 'op_us / host_enqueue_us: us per call [median, min, max] of %d windows x %d '
                     'calls; validate_ms: ms [median, min, max] of %d alternating runs'
                     % (a.rounds, a.reps, a.runs),
           'kernel': kernel_part(ds, dev, a.reps, a.rounds)}
    if not a.skip_validate:
        out['validate'] = validate_part(a.videos, a.runs, dev, a.samples)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
