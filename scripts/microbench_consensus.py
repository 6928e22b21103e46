"""GT consensus scores of one synthetic MSR-VTT-shaped training split (V = 10,509,
20 captions per video, seq_per_img 20, leave-one-out) by both routes, in one
process:

  * ``strings``: wall time of ``prepro.evalscores.compute_consensus_scores`` (the
    Python scorers on the caption strings, one slot at a time), per metric.  It
    is pure host work, and slow: ``--strings_videos`` limits it to the first
    videos of the split (0 skips it), ``--strings_metrics`` to some metrics;
  * ``tokens``: ``ops.consensus.ConsensusScorer`` on the GPU -- the table build
    per metric family (host builder + upload, once per scorer) and the wall
    time of ``scores()`` with the tables built, host clock between device
    synchronisations, ``--runs`` runs after one untimed run;
  * HIP-event time per launch of the four kernels with ``exclude`` over all
    ``videos x 20`` hypotheses, the kernels taking turns (windows of ``--reps``
    launches), and the same launches without ``exclude``;
  * ``backend='cpu'`` (the native twins), one run.

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

from cst_captioning_amd.data import make_synthetic
from cst_captioning_amd.ops.consensus import METRICS, ConsensusScorer, consensus_slots
from cst_captioning_amd.prepro.evalscores import compute_consensus_scores

VOCAB, S = 10509, 20
FAMILY = {'Bleu_4': 'sent', 'ROUGE_L': 'sent', 'METEOR': 'meteor', 'CIDEr': 'cider'}


def stats(v):
    return [round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)]


def wall_ms(fn, sync):
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_times(scorer, ds, reps, rounds=5):
    """us per launch [median, min, max] of `rounds` windows of `reps` launches."""
    dev = scorer.device
    rows, vid, ex = (torch.from_numpy(a).to(dev) for a in
                     consensus_slots(ds.label_start_ix, ds.label_end_ix, S, True))
    fns = {}
    for m in METRICS:
        fns[m + '/exclude'] = lambda m=m: scorer.score_slots(m, rows, vid, ex)
        fns[m + '/all_refs'] = lambda m=m: scorer.score_slots(m, rows, vid, None)
    for fn in fns.values():
        for _ in range(3):
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--videos', type=int, default=6513)
    p.add_argument('--strings_videos', type=int, default=6513,
                   help='videos of the strings route (0: skip it)')
    p.add_argument('--strings_metrics', nargs='+', default=list(METRICS))
    p.add_argument('--runs', type=int, default=5)
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--use_eos', type=int, default=1)
    p.add_argument('--strings_only', action='store_true',
                   help='only the strings route (host work: needs no GPU)')
    a = p.parse_args()
    if not a.strings_only and not torch.cuda.is_available():
        sys.exit('needs a GPU: the token route is measured there')
    t0 = time.perf_counter()
    ds = make_synthetic('msrvtt', num_videos=a.videos, vocab_size=VOCAB, seed=123,
                        feat_dims=[8])
    res = {'videos': a.videos, 'seq_per_img': S, 'hypotheses': a.videos * S,
           'label_width': int(ds.labels.shape[1]), 'use_eos': a.use_eos,
           'make_synthetic_s': round(time.perf_counter() - t0, 1)}

    if not a.strings_only:
        tokens_route(a, ds, res)
    # -- strings -----------------------------------------------------------------------
    if a.strings_videos > 0:
        ids = sorted(ds.gt_refs)[:a.strings_videos]
        refs = {v: ds.gt_refs[v] for v in ids}
        res['strings_videos'] = len(ids)
        res['strings_ms'] = {}
        res['strings_mean'] = {}
        for m in a.strings_metrics:
            ms, out = wall_ms(lambda: compute_consensus_scores(refs, S, True, tokenize=False,
                                                               metrics=(m,)), False)
            res['strings_ms'][m] = round(ms, 1)
            res['strings_mean'][m] = round(float(out[m].mean()), 5)
            print('strings %s: %.1f s' % (m, ms / 1e3), file=sys.stderr, flush=True)
    print(json.dumps(res))


def tokens_route(a, ds, res):
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    # -- tokens, GPU: table build per family, then scores() ----------------------
    torch.zeros(1, device=dev)  # (context creation is not the scorer's)
    scorer = ConsensusScorer(ds, use_eos=a.use_eos, device=dev, backend='gpu')
    build = {}
    for m in ('Bleu_4', 'METEOR', 'CIDEr'):  # (ROUGE_L shares the Bleu_4 tables)
        build[FAMILY[m]] = round(wall_ms(lambda: scorer.build_tables((m,)), True)[0], 1)
    res['tokens_table_build_ms'] = build
    _, tok = wall_ms(lambda: scorer.scores(S), True)  # untimed: first launches
    runs = [wall_ms(lambda: scorer.scores(S), True)[0] for _ in range(a.runs)]
    res['tokens_scores_ms'] = stats(runs)
    res['tokens_scores_per_metric_ms'] = {
        m: stats([wall_ms(lambda: scorer.scores(S, (m,)), True)[0] for _ in range(a.runs)])
        for m in METRICS}
    res['kernel_us'] = kernel_times(scorer, ds, a.reps)
    res['tokens_mean'] = {m: round(float(tok[m].mean()), 5) for m in METRICS}

    # -- tokens, native CPU twins ----------------------------------------------------
    cpu = ConsensusScorer(ds, use_eos=a.use_eos, backend='cpu')
    res['cpu_table_build_ms'] = round(wall_ms(lambda: cpu.build_tables(), False)[0], 1)
    ms, tok_cpu = wall_ms(lambda: cpu.scores(S), False)
    res['cpu_scores_ms'] = round(ms, 1)
    res['gpu_vs_cpu_max_abs_diff'] = {m: float(np.abs(tok[m] - tok_cpu[m]).max())
                                      for m in METRICS}


if __name__ == '__main__':
    main()
