"""Inputs and oracle values shared by tests/test_sent_metrics.py (CPU) and
tests/test_gpu_sent_metrics.py: the smallest datasets at which the sentence
BLEU-4 / ROUGE-L scorers can go wrong, and the fp64 oracle scores of
``eval/metrics.py`` on them (computed once per process, never modified).

Main case: four videos with 1, 3, 20 and 70 references (70: the reference loop
past one wavefront), reference lengths uniform in 1..30, V = 50 (matches and
LCS ambiguity are common); per video 60 hypotheses (a quarter random, length
0..30, BOS allowed inside; the rest a random reference mutated per token: 10 %
delete, 10 % substitute, 5 % insert) plus hand-written rows.  Tiny case: T = 64
hypotheses, 64-token references, token ids up to 65,534 (the packing limit).
"""
import functools

import numpy as np

from cst_captioning_amd.eval.metrics import Bleu, Rouge
from cst_captioning_amd.utils.text import array_to_str

L, V, T = 30, 50, 32
N_REFS = (1, 3, 20, 70)
# oracle.astype(float32) is the target: integer counts / LCS are exact, the fp64
# formula is rounded once to fp32, and the device's pow / exp may differ from
# the host's in the last fp64 bits -> two fp32 ulps
RTOL, ATOL = 2.0 ** -22, 1e-30


class TableDataset:
    """The part of VideoCaptionDataset the reward scorers read."""

    def __init__(self, labels, counts):
        self.labels = np.ascontiguousarray(labels, dtype=np.int64)
        ends = np.cumsum(counts)
        self.label_start_ix = (ends - np.asarray(counts)).astype(np.int64)
        self.label_end_ix = ends.astype(np.int64)
        self.num_videos = len(counts)
        self.df = None

    def gts_of(self, v):
        return self.labels[self.label_start_ix[v]:self.label_end_ix[v]]


def _row(tokens, width):
    out = np.zeros(width, dtype=np.int64)
    out[:len(tokens)] = tokens
    return out


def _mutate(rng, ref):
    out = []
    for t in ref:
        u = rng.rand()
        if u < 0.10:
            continue
        if u < 0.20:
            t = rng.randint(2, V)
        out.append(int(t))
        if rng.rand() < 0.05:
            out.append(int(rng.randint(2, V)))
    return out[:T]


@functools.lru_cache(maxsize=None)
def main_case():
    """(dataset, hyps (N, T) int64, vid (N,) int64, names of the hand rows)."""
    rng = np.random.RandomState(7)
    refs = []  # per video: list of token lists
    for n in N_REFS:
        refs.append([list(rng.randint(2, V, size=rng.randint(1, L + 1))) for _ in range(n)])
    # label rows: BOS, the tokens, EOS padding
    labels = np.stack([_row([1] + r, L + 2) for vr in refs for r in vr])
    ds = TableDataset(labels, N_REFS)
    hyps, vid = [], []
    for v, vr in enumerate(refs):
        for i in range(60):
            if i % 4 == 0:
                h = list(rng.randint(2, V, size=rng.randint(0, L + 1)))
                if len(h) > 2 and rng.rand() < 0.5:
                    h[rng.randint(0, len(h))] = 1  # BOS inside: dropped
            else:
                h = _mutate(rng, vr[rng.randint(0, len(vr))])
            hyps.append(_row(h, T))
            vid.append(v)
    hand = {}

    def add(name, v, tokens):
        hand[name] = len(hyps)
        hyps.append(_row(tokens, T))
        vid.append(v)
    add('all_eos', 2, [])
    add('no_eos', 2, list(rng.randint(2, V, size=T)))
    add('copy_of_reference', 3, refs[3][5][:T])
    long_ref = max(refs[2], key=len)
    add('one_token_repeated', 2, [long_ref[0]] * T)  # clipping
    for n in (1, 2, 3):  # orders with guess_k = 0
        add('length_%d' % n, 3, refs[3][11][:n] if len(refs[3][11]) >= n else [5] * n)
    # a length exactly between two reference lengths of the 3-reference video,
    # no third length closer: closest-length tie, the shorter one wins
    lens = sorted(len(r) for r in refs[1])
    tie = [(a, b) for a in lens for b in lens
           if a < b and (a + b) % 2 == 0
           and all(abs(c - (a + b) // 2) >= (b - a) // 2 for c in lens)]
    assert tie, 'generator seed gives no closest-length tie: %r' % (lens,)
    a, b = tie[0]
    src = [r for r in refs[1] if len(r) == b][0]
    add('closest_length_tie', 1, src[:(a + b) // 2])
    mid = list(refs[2][3][:8]) + [1] + list(refs[2][3][8:12])
    add('bos_in_the_middle', 2, mid)
    return ds, np.stack(hyps), np.asarray(vid, dtype=np.int64), hand


@functools.lru_cache(maxsize=None)
def tiny_case():
    """T = 64, 64-token references without EOS, token ids up to 65,534."""
    rng = np.random.RandomState(11)
    r0 = rng.randint(65000, 65535, size=64)
    r0[:3] = (65534, 65534, 65533)
    r1 = rng.randint(2, 65535, size=64)
    ds = TableDataset(np.stack([r0, r1]), (2,))
    hyps = [r0.copy(), r1.copy()]
    h = r0.copy()
    h[10:20] = rng.randint(65000, 65535, size=10)
    hyps.append(h)
    hyps.append(np.roll(r1, 5))
    hyps.append(np.full(64, 65534))
    hyps.append(_row(list(r0[:40]), 64))
    hyps.append(rng.randint(2, 65535, size=64))
    return ds, np.stack(hyps).astype(np.int64), np.zeros(len(hyps), dtype=np.int64), {}


def direct_oracle(ds, hyps, vid, metric, use_eos):
    """fp64 scores of eval/metrics.py, called directly."""
    ref_strs = {int(v): [array_to_str(r, use_eos) for r in ds.gts_of(int(v))]
                for v in np.unique(vid)}
    res = {i: [array_to_str(h, use_eos)] for i, h in enumerate(hyps)}
    gts = {i: ref_strs[int(v)] for i, v in enumerate(vid)}
    if metric == 'Bleu_4':
        s = np.asarray(Bleu(4).compute_score(gts, res)[1][-1], dtype=np.float64)
    else:
        s = np.asarray(Rouge().compute_score(gts, res)[1], dtype=np.float64)
    assert s.shape == (len(hyps),)
    return s


@functools.lru_cache(maxsize=None)
def oracle(case, metric, use_eos):
    """The oracle on a case above, computed once (read-only array)."""
    ds, hyps, vid, _ = {'main': main_case, 'tiny': tiny_case}[case]()
    s = direct_oracle(ds, hyps, vid, metric, use_eos)
    s.setflags(write=False)
    return s


def check(got, case, metric, use_eos):
    """Every hypothesis against the oracle; exact zeros stay exact."""
    want = oracle(case, metric, use_eos).astype(np.float32)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    assert np.array_equal(got == 0, want == 0)


def check_not_vacuous(use_eos):
    b, r = oracle('main', 'Bleu_4', use_eos), oracle('main', 'ROUGE_L', use_eos)
    assert (b > 1e-3).mean() >= 0.5, (b > 1e-3).mean()
    assert (r > 0).mean() >= 0.9, (r > 0).mean()
    _, _, _, hand = main_case()
    # the all-EOS row is the empty sentence (exact 0), or with use_eos the
    # one-token sentence "0", which every reference ends with
    assert (b[hand['all_eos']] == 0) == (r[hand['all_eos']] == 0) == (not use_eos)
