"""Truncated sampling of the consensus pool, measured on one GPU in one process
at the headline shape (H = E = 512, V = 10,509, seq_length 30; a pool of 32
videos x 20 samples = 640 rows):

  * ``decode``: the sampled pool decode (``DecoderEngine.sample`` with
    ``sample_max 0, expand_feat 1``) with ``top_k = 0`` -- the two-launch
    sampler, the path of a call without the keys -- and with ``--top_k`` /
    ``--top_p`` -- the three-launch loop of ``beam_search.cpp`` sample_topk --:
    host clock around ``--reps`` decodes ending in a synchronise, ``--rounds``
    windows per arm, the arms taking turns; per decode and per step (28 steps);
  * ``validate``: ``Trainer.validate`` with ``--decode mbr`` (greedy row 0, 20
    samples, ``--val_scorer tokens``, test batch 32) per batch for both arms,
    alternating;
  * ``--part profile``: nothing timed: a few decodes of each arm, for a kernel
    trace taken around the process (per-launch times).

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cst_captioning_amd.cli import build_model
from cst_captioning_amd.config import default_opts
from cst_captioning_amd.data import CaptionLoader, make_synthetic
from cst_captioning_amd.parallel import DistContext
from cst_captioning_amd.train.trainer import Trainer

VOCAB, B, N = 10509, 32, 20


def stats(v, nd=3):
    return [round(float(np.median(v)), nd), round(float(min(v)), nd), round(float(max(v)), nd)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--part', default='all', choices=['all', 'decode', 'validate', 'profile'])
    p.add_argument('--top_k', type=int, default=5)
    p.add_argument('--top_p', type=float, default=0.9)
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--videos', type=int, default=256)
    p.add_argument('--runs', type=int, default=5)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('needs a GPU: the decode is measured there')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    ds = make_synthetic('msrvtt', num_videos=a.videos, vocab_size=VOCAB, seed=123)
    opt = default_opts(batch_size=B, train_seq_per_img=N, test_batch_size=B, test_seq_per_img=N,
                       rnn_size=512, input_encoding_size=512, drop_prob_lm=0.5, beam_size=1,
                       impl='hip', seed=123, loglevel='WARNING', save_last=0, max_epochs=1,
                       print_log_interval=0, val_scorer='tokens', decode='mbr', mbr_samples=N)
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    opt.vocab_size, opt.seq_length, opt.feat_dims = ds.vocab_size, ds.seq_length, ds.feat_dims
    torch.manual_seed(123)
    model, engine = build_model(opt, dev, 'hip')
    assert engine is not None
    train = CaptionLoader(ds, B, N, 'train', dev, seed=123)
    val = CaptionLoader(ds, B, N, 'test', dev)
    tr = Trainer(opt, model, train, val, DistContext(device=dev), engine)
    model.eval()
    model.set_seq_per_img(N)
    feats = val.get_batch_at(0)['feats']
    arms = {'top_k0': {'sample_max': 0, 'expand_feat': 1, 'beam_size': 1},
            'top_k%d_p%.2f' % (a.top_k, a.top_p): {'sample_max': 0, 'expand_feat': 1, 'beam_size': 1,
                                                 'top_k': a.top_k, 'top_p': a.top_p}}
    steps = ds.seq_length - 2
    out = {'shape': {'H': 512, 'V': VOCAB, 'seq_length': ds.seq_length, 'rows': B * N,
                     'steps': steps},
           'format': 'ms [median, min, max]'}

    def decode(o, reps):
        with torch.no_grad():
            for _ in range(reps):
                r = model.sample(feats, o)
        return r

    for o in arms.values():  # warm-up: code objects, allocator
        decode(o, 3)
    torch.cuda.synchronize()
    if a.part == 'profile':
        for o in arms.values():
            decode(o, 5)
        torch.cuda.synchronize()
        print(json.dumps({'profile': 'done', 'decodes_per_arm': 8}))
        return
    if a.part in ('all', 'decode'):
        times = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, o in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                decode(o, a.reps)
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3 / a.reps)
        out['decode_ms'] = {k: stats(v) for k, v in times.items()}
        out['decode_us_per_step'] = {k: round(float(np.median(v)) * 1e3 / steps, 2)
                                     for k, v in times.items()}
        seq = {k: decode(o, 1)[0] for k, o in arms.items()}
        out['mean_caption_length'] = {k: round(float((s > 0).sum(1).float().mean()), 2)
                                      for k, s in seq.items()}
    if a.part in ('all', 'validate'):
        nb = -(-a.videos // B)

        def validate(k):
            tr.opt.mbr_top_k, tr.opt.mbr_top_p = (0, 1.0) if k == 'top_k0' else (a.top_k, a.top_p)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = tr.validate(val)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / nb, res

        warm = {k: validate(k) for k in arms}  # untimed
        out['validate_scores'] = {k: warm[k][1]['scores'] for k in arms}
        times = {k: [] for k in arms}
        for _ in range(a.runs):
            for k in arms:
                times[k].append(validate(k)[0])
        out['validate_ms_per_batch'] = {k: stats(v) for k, v in times.items()}
        out['validate_batches'] = nb
    print(json.dumps(out))


if __name__ == '__main__':
    main()
