"""Mixed-metric reward (--reward_mix) at the headline shape (synthetic MSR-VTT,
6,513 videos x 20 captions, V = 10,509; 1,344 hypotheses = 1,280 samples + 64
greedy rows, T = 30, use_eos = 1, weights CIDEr:1, Bleu_4:5, ROUGE_L:5): fused
against composed, taking turns in one process.

  (a) fused:    reward_mix_kernel, one launch (ops/reward_mix.py reward_mix_score);
  (b) composed: the three existing scorers' .score (cider_d_kernel,
                bleu4_kernel, rouge_l_kernel) plus the blend
                w_c * c + w_b * b + w_r * r in torch ops.

HIP-event windows of 200 back-to-back calls, 5 windows per arm, for hypotheses
of random tokens (a random-init rollout: no early EOS) and of ground-truth
captions (short, many matches); median [min, max].  Both arms are checked
against the oracle on a slice before anything is timed.  The rule: the fused
kernel stays only if its median is below the composition's by more than the
larger of the two arms' max - min spread ('fused_wins').

With --steps N > 0 also, for information: the captured SCST training step with
--reward_mix CIDEr:1,Bleu_4:5,ROUGE_L:5 against --eval_metric CIDEr, trainers
alternating in one process.

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

from cst_captioning_amd.data import CaptionLoader, make_synthetic
from cst_captioning_amd.ops.cider_d import CiderDScorer
from cst_captioning_amd.ops.reward_mix import MixedRewardScorer
from cst_captioning_amd.ops.sent_metrics import SentenceMetricScorer

N, T, VIDEOS, VOCAB = 1344, 30, 6513, 10509
SPEC, WEIGHTS = 'CIDEr:1,Bleu_4:5,ROUGE_L:5', (1.0, 5.0, 5.0)


def timed_interleaved(fns, reps=200, rounds=5):
    """us per call of each fn: `rounds` windows of `reps` back-to-back calls
    per fn, the fns taking turns; returns {name: [median, min, max]}."""
    for fn in fns.values():
        for _ in range(10):
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
    return {k: [round(float(np.median(v)), 2), round(min(v), 2), round(max(v), 2)]
            for k, v in out.items()}


def step_times(ds, dev, steps, rounds=3):
    from cst_captioning_amd.cli import build_model
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.train.trainer import Trainer
    S, B = 20, 64
    trainers = {}
    for name, mix in (('eval_metric_CIDEr', ''), ('reward_mix', SPEC)):
        opt = default_opts(batch_size=B, train_seq_per_img=S, test_seq_per_img=S, rnn_size=512,
                           input_encoding_size=512, drop_prob_lm=0.5, learning_rate=1e-4,
                           grad_clip=0.25, eval_metric='CIDEr', reward_mix=mix,
                           max_epochs=10 ** 9, print_log_interval=0, use_rl=1, use_rl_after=0,
                           use_cst=0, use_mixer=1, mixer_from=1, use_eos=1, expand_feat=1,
                           impl='hip', seed=123, loglevel='WARNING', save_last=0, cuda_graph=1)
        opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
        opt.vocab_size, opt.seq_length, opt.feat_dims = ds.vocab_size, ds.seq_length, ds.feat_dims
        torch.manual_seed(123)
        model, engine = build_model(opt, dev, 'hip')
        loader = CaptionLoader(ds, B, S, 'train', dev, seed=123)
        tr = Trainer(opt, model, loader, None, DistContext(device=dev), engine)
        tr.rl_training = True
        for _ in range(5):
            tr.train_step(loader.get_batch(), 0)
        torch.cuda.synchronize()
        assert tr._graph is not None and tr.scorer.backend == 'gpu'
        assert isinstance(tr.scorer, MixedRewardScorer) == bool(mix)
        trainers[name] = (tr, loader)
    out = {k: [] for k in trainers}
    for _ in range(rounds):
        for k, (tr, loader) in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train_step(loader.get_batch(), 0)
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3 / steps)
    return {k: [round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)]
            for k, v in out.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--steps', type=int, default=0,
                   help='also time this many captured SCST steps per trainer and round')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('needs a GPU: nothing here is measured on the CPU')
    dev = torch.device('cuda')
    ds = make_synthetic('msrvtt', num_videos=VIDEOS, vocab_size=VOCAB, seed=123)
    mix = MixedRewardScorer(ds, WEIGHTS, use_eos=1, device=dev)
    assert mix.backend == 'gpu'
    cider = CiderDScorer(ds, use_eos=1, device=dev)
    bleu = SentenceMetricScorer(ds, 'Bleu_4', use_eos=1, device=dev)
    rouge = SentenceMetricScorer(ds, 'ROUGE_L', use_eos=1, device=dev)
    w_c, w_b, w_r = WEIGHTS

    def composed(h, v):
        return w_c * cider.score(h, v) + w_b * bleu.score(h, v) + w_r * rouge.score(h, v)

    g = torch.Generator(device='cpu').manual_seed(0)
    vid = torch.randint(0, VIDEOS, (N,), generator=g)
    rnd = torch.randint(3, VOCAB, (N, T), generator=g)
    rnd[:, T - 1] = 0
    labels = torch.from_numpy(ds.labels).long()
    # a reference of the video (not always the first), its leading BOS dropped
    pick = torch.from_numpy(ds.label_start_ix[vid.numpy()]).long() + \
        torch.randint(0, 20, (N,), generator=g)
    gt = torch.zeros(N, T, dtype=torch.long)
    rows = labels[pick][:, 1:T + 1]
    gt[:, :rows.shape[1]] = rows
    vid, rnd, gt = vid.to(dev), rnd.to(dev), gt.to(dev)
    res = {'N': N, 'T': T, 'refs_per_video': 20, 'vocab': VOCAB, 'use_eos': 1, 'weights': WEIGHTS,
           'format': 'us per call [median, min, max] of 5 windows x 200 calls'}
    # correctness before timing (the Python oracles on a slice)
    for h, tag in ((rnd, 'random'), (gt, 'gt')):
        want = mix.score_reference(h[:64], vid[:64])
        for fn, name in ((mix.score, 'fused'), (composed, 'composed')):
            got = fn(h[:64], vid[:64]).cpu().numpy()
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-4, err_msg=name + ' ' + tag)
        full, parts = mix.score_both(h, vid)
        res['%s_mean_reward' % tag] = float(full.mean())
        res['%s_mean_parts' % tag] = [round(float(x), 5) for x in parts.mean(0)]
        res['%s_max_abs_fused_minus_composed' % tag] = float((full - composed(h, vid)).abs().max())
        res['%s_max_abs_cider_column_minus_cider_d_kernel' % tag] = \
            float((parts[:, 0] - cider.score(h, vid)).abs().max())
    for h, tag in ((rnd, 'random'), (gt, 'gt')):
        t = timed_interleaved({'fused': lambda: mix.score(h, vid),
                               'composed': lambda: composed(h, vid)})
        spread = max(v[2] - v[1] for v in t.values())
        for k, v in t.items():
            res['%s_%s_us' % (k, tag)] = v
        res['fused_wins_%s' % tag] = bool(t['composed'][0] - t['fused'][0] > spread)
    if a.steps > 0:
        res['scst_step_ms'] = step_times(ds, dev, a.steps)
        res['scst_step_format'] = ('ms per captured step [median, min, max] of 3 rounds x %d '
                                   'steps, host clock + synchronise' % a.steps)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
