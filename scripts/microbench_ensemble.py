"""Ensemble decoding measured on one GPU in one process at the headline shape
(H = E = 512, V = 10,509, seq_length 30, 64 videos):

  * ``kernel``: ``ensemble_topk_kernel`` alone through its test route at R = 320
    rows (64 videos x beam 5), K = 5, M in {1, 2, 4} members, and for M = 1
    ``beam_topk_kernel`` on the same input: device events around ``--reps``
    back-to-back launches, ``--rounds`` windows per arm, the arms taking turns.
    The route allocates its two outputs per call, so this is launch-to-launch
    time of the route; the kernels' own times come from a kernel trace taken
    around ``--part profile``.  Beside each: the bytes it must read
    (``R * M * ldl * 4``) and the GB/s that makes;
  * ``decode``: videos/s of the beam-5 ensemble decode for M in {1, 2, 4}, and
    of the single model's beam-5 (the fused two-launch path) and beam-9 (the
    dense general path, graph replay and the plain loop), host clock around
    ``--reps`` decodes ending in a synchronise;
  * ``--part profile``: nothing timed: 55 launches of each kernel arm, for a
    kernel trace taken around the process.

Prints one JSON line."""
import argparse
import json
import math
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
from cst_captioning_amd.models.decoder_engine import EnsembleEngine
from cst_captioning_amd.models.ensemble import EnsembleCaptionModel

VOCAB, B, K, R = 10509, 64, 5, 320
MS = (1, 2, 4)


def stats(v, nd=3):
    return [round(float(np.median(v)), nd), round(float(min(v)), nd), round(float(max(v)), nd)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--part', default='all', choices=['all', 'kernel', 'decode', 'profile'])
    p.add_argument('--reps', type=int, default=200)
    p.add_argument('--decode_reps', type=int, default=10)
    p.add_argument('--rounds', type=int, default=7)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('needs a GPU: the kernel and the decode are measured there')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    C = _ext.ops()
    ldl = (VOCAB + 7) // 8 * 8
    g = torch.Generator().manual_seed(0)
    z = [(torch.randn(R, ldl, generator=g) * 3).to(dev) for _ in range(max(MS))]
    lse = [torch.logsumexp(x[:, :VOCAB], 1).contiguous() for x in z]
    e = torch.empty(0, device=dev)

    def launch(M, baseline=False):
        return C.vocab_select(e, e, e, e, 1, 1.0, 0, ens_logits=z[:M], ens_lse=lse[:M],
                              ens_logw=[math.log(1.0 / M)] * M, ens_V=VOCAB, ens_K=K,
                              ens_baseline=baseline)

    arms = {'ensemble_m%d' % M: (lambda M=M: launch(M)) for M in MS}
    arms['beam_topk_m1'] = lambda: launch(1, True)
    out = {'shape': {'H': 512, 'V': VOCAB, 'ldl': ldl, 'R': R, 'K': K, 'videos': B},
           'format': '[median, min, max]'}
    a0, b0 = launch(1), launch(1, True)
    out['m1_equals_beam_topk'] = bool(torch.equal(a0[0], b0[0]) and torch.equal(a0[1], b0[1]))
    for f in arms.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    if a.part == 'profile':  # (the kernel arms only: one shape per kernel name in the trace)
        for f in list(arms.values()) * 50:
            f()
        torch.cuda.synchronize()
        print(json.dumps({'profile': 'done', 'launches_per_arm': 55}))
        return
    if a.part in ('all', 'kernel'):
        times = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, f in arms.items():
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                ev0.record()
                for _ in range(a.reps):
                    f()
                ev1.record()
                torch.cuda.synchronize()
                times[k].append(ev0.elapsed_time(ev1) * 1e3 / a.reps)
        out['route_us_per_launch'] = {k: stats(v, 2) for k, v in times.items()}
        out['bytes_read'] = {'ensemble_m%d' % M: R * M * ldl * 4 for M in MS}
        out['bytes_read']['beam_topk_m1'] = R * ldl * 4
        out['route_GBps'] = {k: round(out['bytes_read'][k] / (np.median(v) * 1e-6) / 1e9, 1)
                             for k, v in times.items()}
    # the decode: max(MS) independently initialised members of the headline shape
    ds = make_synthetic('msrvtt', num_videos=B, vocab_size=VOCAB, seed=123)
    members, engines = [], []
    for i in range(max(MS)):
        opt = default_opts(batch_size=B, train_seq_per_img=20, test_batch_size=B,
                           test_seq_per_img=20, rnn_size=512, input_encoding_size=512,
                           drop_prob_lm=0.5, beam_size=K, impl='hip', seed=123,
                           loglevel='WARNING')
        opt.vocab = {j: w for j, w in enumerate(ds.vocab)}
        opt.vocab_size, opt.seq_length, opt.feat_dims = ds.vocab_size, ds.seq_length, ds.feat_dims
        torch.manual_seed(123 + i)
        m, eng = build_model(opt, dev, 'hip')
        assert eng is not None
        with torch.no_grad():
            m.logit.weight.mul_(3.0)
        eng.refresh_weights()
        members.append(m.eval())
        engines.append(eng)
    feats = CaptionLoader(ds, B, 20, 'test', dev).get_batch_at(0)['feats']
    m0, e0 = members[0], engines[0]

    def ens_decode(M):
        ens = EnsembleCaptionModel(members[:M])
        EnsembleEngine(ens, engines[:M])
        return lambda: ens.sample_beam(feats, {'beam_size': K})

    def plain_loop(Kb):  # the single model's native loop without the graph replay
        def f():
            vg, blog, att, s0 = e0._decode_operands(m0, feats)
            return C.beam_search(e0.wx, e0.ptab, e0.whh, e0.wlog, blog, vg, Kb, m0.seq_length, 1,
                                 att, e0.cell, s0, e0.upper_operands())
        return f

    darms = {'ensemble_m%d_beam5' % M: ens_decode(M) for M in MS}
    darms['single_beam5_fused_graph'] = lambda: e0.sample_beam(m0, feats, {'beam_size': 5})
    darms['single_beam5_fused_loop'] = plain_loop(5)
    darms['single_beam9_dense_graph'] = lambda: e0.sample_beam(m0, feats, {'beam_size': 9})
    darms['single_beam9_dense_loop'] = plain_loop(9)
    with torch.no_grad():
        for f in darms.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        if a.part in ('all', 'decode'):
            times = {k: [] for k in darms}
            for _ in range(a.rounds):
                for k, f in darms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.decode_reps):
                        f()
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t0) * 1e3 / a.decode_reps)
            out['decode_ms'] = {k: stats(v) for k, v in times.items()}
            out['decode_videos_per_s'] = {k: round(B / (np.median(v) * 1e-3), 1)
                                          for k, v in times.items()}
            s1 = darms['ensemble_m1_beam5']()[0]
            s5 = darms['single_beam5_fused_loop']()[0]
            out['m1_rows_equal_to_single_beam5'] = round(float((s1 == s5).all(1).float().mean()), 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
