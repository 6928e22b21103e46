"""Consensus (MBR) decoding, measured on one GPU in one process:

  * the peer CIDEr-D kernel (``csrc/kernels/cider_pairwise.hip``) at
    ``B=32, G=21, T=29`` (one MSR-VTT test batch at ``--mbr_samples 20``) and at
    ``B=64, G=64, T=31`` (an LDS limit): HIP-event time per call of the bare op
    (``cider_score(..., group=G)`` on prepared tensors), windows of ``--reps``
    back-to-back calls, the shapes taking turns.  A call is the launch plus the
    binding's argument conversion and the allocation of the result, so the
    figure is an upper bound of the kernel's time; the host time to enqueue one
    call is reported beside it (where it is the smaller of the two, the device
    and not the host paces the window).  The native CPU twin and the
    Python oracle on the same inputs (host clock; the oracle on the first
    ``--oracle_pools`` pools, scaled to the batch);
  * ``Trainer.validate`` end to end on a synthetic MSR-VTT-shaped split (V =
    10,509, fused engine, ``--val_scorer tokens``, test batch 64, beam 5) with
    ``--decode standard`` and ``--decode mbr`` at ``N = 20``: ``--runs`` runs
    each, alternating, after one untimed run of each; and the parts of the mbr
    decode over the same batches: the beam decode, the N-row sampled decode, the
    peer scoring with selection.

The model is randomly initialised, so the captions are long (few early EOS): a
worst case for the scorer.  Prints one JSON line.
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
from cst_captioning_amd.ops.mbr import PeerCiderD
from cst_captioning_amd.parallel import DistContext
from cst_captioning_amd.train.trainer import Trainer

VOCAB = 10509
SHAPES = ((32, 21, 29), (64, 64, 31))


def stats(v, nd=2):
    return [round(float(np.median(v)), nd), round(min(v), nd), round(max(v), nd)]


def pools(ds, B, G, T, seed):
    """Pools like a decoder's: rows of one pool are label rows of one video with
    a few substitutions, cut to T tokens."""
    rng = np.random.RandomState(seed)
    out = np.zeros((B * G, T), dtype=np.int64)
    for b in range(B):
        g = ds.gts_of(b % len(ds.label_start_ix))
        for j in range(G):
            row = np.asarray(g[rng.randint(len(g))][1:T + 1], dtype=np.int64).copy()
            k = rng.randint(0, 3)
            live = np.flatnonzero(row > 0)
            if k and len(live):
                row[rng.choice(live, k)] = rng.randint(3, VOCAB, size=k)
            out[b * G + j, :len(row)] = row
    return out


def kernel_part(ds, dev, reps, rounds, oracle_pools):
    gpu = PeerCiderD(ds.df, use_eos=1, device=dev, backend='gpu')
    cpu = PeerCiderD(ds.df, use_eos=1, backend='cpu')
    ref = PeerCiderD(ds.df, use_eos=1, backend='cpu-ref')
    data = {s: torch.from_numpy(pools(ds, *s, seed=1)) for s in SHAPES}
    on_dev = {s: h.to(dev) for s, h in data.items()}
    ops, none = _ext.ops(), torch.zeros(0, dtype=torch.long, device=dev)

    def call(s):  # the bare op: no Python-side checks or copies
        return ops.cider_score(on_dev[s], none, gpu._tables, gpu.log_ref_len, 1, group=s[1])

    for s in SHAPES:
        for _ in range(5):
            call(s)
    times = {s: [] for s in SHAPES}
    enq = {s: [] for s in SHAPES}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for s in SHAPES:
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for _ in range(reps):
                call(s)
            enq[s].append((time.perf_counter() - t0) * 1e6 / reps)
            e1.record()
            torch.cuda.synchronize()
            times[s].append(e0.elapsed_time(e1) * 1e3 / reps)
    out = {}
    for s in SHAPES:
        B, G, T = s
        got = gpu.score(on_dev[s], G).cpu().numpy()
        t0 = time.perf_counter()
        twin = cpu.score(data[s], G).numpy()
        cpu_ms = (time.perf_counter() - t0) * 1e3
        nb = min(B, oracle_pools)
        t0 = time.perf_counter()
        want = ref.score_reference(data[s][:nb * G], G)
        ora_ms = (time.perf_counter() - t0) * 1e3 * B / nb
        out['B%d_G%d_T%d' % s] = {
            'op_us': stats(times[s]), 'host_enqueue_us': stats(enq[s]), 'cpu_twin_ms': round(cpu_ms, 2),
            'python_oracle_ms_scaled_from_%d_pools' % nb: round(ora_ms, 1),
            'mean_tokens': round(float((data[s] > 0).sum(1).float().mean()), 1),
            'gpu_vs_twin_max_abs': float(np.abs(got - twin).max()),
            'gpu_vs_oracle_max_abs': float(np.abs(got[:nb * G] - want).max()),
            'score_max': float(twin.max())}
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
    scorer = tr.mbr_scorer

    def validate(mode):
        tr.mbr_scorer = scorer if mode == 'mbr' else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tr.validate(val)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    nb = -(-n_videos // B)
    res = {'videos': n_videos, 'batches': nb, 'mbr_samples': N, 'beam_size': 5}
    warm = {m: validate(m) for m in ('standard', 'mbr')}  # untimed
    res['scores_standard'] = warm['standard'][1]['scores']
    res['scores_mbr'] = warm['mbr'][1]['scores']
    res['mean_mbr_score'] = round(float(np.mean([p['mbr_score']
                                                 for p in warm['mbr'][1]['predictions']])), 4)
    times = {'standard': [], 'mbr': []}
    for _ in range(runs):
        for m in ('standard', 'mbr'):
            times[m].append(validate(m)[0])
    res['validate_ms'] = {m: stats(v) for m, v in times.items()}
    res['extra_ms'] = round(float(np.median(times['mbr']) - np.median(times['standard'])), 2)

    # the parts of the mbr decode over the same batches
    model.eval()
    feats = [val.get_batch_at(ii)['feats'] for ii in range(nb)]
    parts = {'beam_decode': [], 'sampled_decode': [], 'peer_score_select': []}
    prev = model.seq_per_img
    with torch.no_grad():
        model.set_seq_per_img(N)
        pool = [model.sample(f, {'sample_max': 0, 'expand_feat': 1, 'beam_size': 1})[0]
                for f in feats]
        pool = [torch.cat([p.view(-1, N, p.size(1)), p.view(-1, N, p.size(1))[:, :1]], 1)
                .reshape(-1, p.size(1)).contiguous() for p in pool]  # (G = N + 1 rows per video)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(nb):
                fn(i)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(runs):
            model.set_seq_per_img(prev)
            parts['beam_decode'].append(timed(lambda i: model.sample(feats[i], {'beam_size': 5})))
            model.set_seq_per_img(N)
            parts['sampled_decode'].append(timed(lambda i: model.sample(
                feats[i], {'sample_max': 0, 'expand_feat': 1, 'beam_size': 1})))
            parts['peer_score_select'].append(timed(lambda i: scorer.select(pool[i], N + 1)))
        model.set_seq_per_img(prev)
    model.train()
    res['parts_ms'] = {k: stats(v) for k, v in parts.items()}
    res['pool_width'] = int(pool[0].size(1))
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--videos', type=int, default=497)
    p.add_argument('--runs', type=int, default=5)
    p.add_argument('--reps', type=int, default=200)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--samples', type=int, default=20)
    p.add_argument('--oracle_pools', type=int, default=4)
    p.add_argument('--skip_validate', action='store_true')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('needs a GPU: the kernel and the decode are measured there')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    ds = make_synthetic('msrvtt', num_videos=64, vocab_size=VOCAB, seed=123, feat_dims=[8])
    out = {'format': 'op_us / host_enqueue_us: us per call [median, min, max] of %d windows x %d calls; '
                     'validate_ms / parts_ms: ms [median, min, max] of %d alternating runs'
                     % (a.rounds, a.reps, a.runs),
           'kernel': kernel_part(ds, dev, a.reps, a.rounds, a.oracle_pools)}
    if not a.skip_validate:
        out['validate'] = validate_part(a.videos, a.runs, dev, a.samples)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
