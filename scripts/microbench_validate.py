"""``Trainer.validate`` end to end with ``--val_scorer strings`` and ``tokens``
on a synthetic MSR-VTT-shaped split (V = 10,509, 20 references per video, beam
5, fused engine, test batch 64), at 497 videos (the MSR-VTT validation size)
and 2,990 (its test size).

  * wall time of ``validate`` per scorer: ``--runs`` runs each (default 5),
    alternating in one process, after one untimed run of each (which builds the
    token scorer's tables and warms the decode graphs); host clock between
    device synchronisations;
  * the beam decode alone over the same batches (its share of ``tokens``);
  * HIP-event time per launch of ``bleu_stats_kernel``, ``meteor_stats_kernel``,
    the unclipped CIDEr kernel and ``rouge_l_kernel`` on the decoded captions;
  * the one-off table build of the token scorer.

The model is randomly initialised, so the decoded captions are long (few early
EOS): a worst case for both scorers.  Prints one JSON line.
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
from cst_captioning_amd.parallel import DistContext
from cst_captioning_amd.train.trainer import Trainer

VOCAB = 10509


def stats(v):
    return [round(float(np.median(v)), 2), round(min(v), 2), round(max(v), 2)]


def kernel_times(scorer, seqs, vi, reps=100, rounds=5):
    """us per launch [median, min, max] of `rounds` windows of `reps` launches,
    the kernels taking turns."""
    ops = _ext.ops()
    hyps = scorer.canon_t[seqs]
    mt, ct = scorer._metric_tables, scorer._cider_tables
    fns = {'bleu_stats_kernel': lambda: ops.bleu_stats(hyps, vi, mt),
           'meteor_stats_kernel': lambda: ops.meteor_stats(hyps, vi, mt, scorer.stems_t),
           'cider_unclipped_kernel': lambda: ops.cider_score(hyps, vi, ct, scorer.log_ref_len, 0,
                                                             False),
           'rouge_l_kernel': lambda: ops.metric_score('ROUGE_L', hyps, vi, mt, 0)}
    for fn in fns.values():
        for _ in range(5):
            fn()
    out = {k: [] for k in fns}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    return {k: stats(v) for k, v in out.items()}


def run_size(n_videos, runs, dev):
    ds = make_synthetic('msrvtt', num_videos=n_videos, vocab_size=VOCAB, seed=123)
    B, S = 64, 20
    opt = default_opts(batch_size=B, train_seq_per_img=S, test_batch_size=B, test_seq_per_img=S,
                       rnn_size=512, input_encoding_size=512, drop_prob_lm=0.5, beam_size=5,
                       impl='hip', seed=123, loglevel='WARNING', save_last=0, max_epochs=1,
                       print_log_interval=0, val_scorer='strings')
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    opt.vocab_size, opt.seq_length, opt.feat_dims = ds.vocab_size, ds.seq_length, ds.feat_dims
    torch.manual_seed(123)
    model, engine = build_model(opt, dev, 'hip')
    assert engine is not None
    train = CaptionLoader(ds, B, S, 'train', dev, seed=123)
    val = CaptionLoader(ds, B, S, 'test', dev)
    tr = Trainer(opt, model, train, val, DistContext(device=dev), engine)

    def validate(mode):
        opt.val_scorer = mode
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tr.validate(val)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    res = {'videos': n_videos, 'batches': -(-n_videos // B)}
    t0 = time.perf_counter()
    scorer = tr.corpus_scorer(val)
    res['token_scorer_build_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    warm = {m: validate(m) for m in ('strings', 'tokens')}  # untimed
    res['scores_strings'] = warm['strings'][1]['scores']
    res['scores_tokens'] = warm['tokens'][1]['scores']
    res['predictions_equal'] = warm['strings'][1]['predictions'] == warm['tokens'][1]['predictions']
    times = {'strings': [], 'tokens': []}
    for _ in range(runs):
        for m in ('strings', 'tokens'):
            times[m].append(validate(m)[0])
    res['validate_ms'] = {m: stats(v) for m, v in times.items()}
    res['ratio_strings_over_tokens'] = round(float(np.median(times['strings']) /
                                                   np.median(times['tokens'])), 2)
    # the beam decode alone over the same batches
    model.eval()
    dec = []
    with torch.no_grad():
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for ii in range(res['batches']):
                model.sample(val.get_batch_at(ii)['feats'], {'beam_size': 5})
            torch.cuda.synchronize()
            dec.append((time.perf_counter() - t0) * 1e3)
    model.train()
    res['beam_decode_ms'] = stats(dec)
    res['decode_share_of_tokens'] = round(float(np.median(dec) / np.median(times['tokens'])), 3)
    out = warm['tokens'][1]
    seqs = torch.from_numpy(out['sequences']).to(dev)
    vi = torch.from_numpy(out['video_index']).to(dev)
    res['mean_caption_tokens'] = round(float((torch.cumprod((seqs > 0).long(), 1)).sum(1)
                                             .float().mean()), 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scorer.score(seqs, vi)
    res['token_score_call_ms'] = round((time.perf_counter() - t0) * 1e3, 2)
    res['kernel_us'] = kernel_times(scorer, seqs, vi)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--videos', type=int, nargs='+', default=[497, 2990])
    p.add_argument('--runs', type=int, default=5)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('needs a GPU: nothing here is measured on the CPU')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    out = {'format': 'ms [median, min, max] of %d alternating runs; kernel_us: us per launch '
                     '[median, min, max] of 5 windows x 100 launches' % a.runs,
           'sizes': [run_size(n, a.runs, dev) for n in a.videos]}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
