"""Inputs and oracle values shared by tests/test_consensus.py (CPU) and
tests/test_gpu_consensus.py: the smallest label stores at which leave-one-out
scoring can go wrong, and the Python oracles' scores on them (computed once per
process, never modified).

Hand-made store (captions of at most 12 tokens, S = 5 slots):
  v0  4 captions (ncap < S: slots cycle).  Caption 0 is the only holder of the
      maximum count of the unigram "plays" (3; the others have 1 and 2), so
      leaving it out must clip at ng_cnt2 = 2;
  v1  two captions tied for the maximum count of "dog" (ng_arg = -1);
  v2  the same caption twice: leaving one out still scores BLEU 1;
  v3  one caption: nothing is left out;
  v4  caption 0 (5 tokens) is its own closest reference length; without it the
      closest is 3, not 9;
  v5  stem-only matches between captions ("runs" / "running", "dog" / "dogs",
      a duplicate vocabulary word): the best METEOR and ROUGE reference of every
      caption is the caption itself, which is left out;
  v6  7 captions (ncap > S).
With ``big``: v7 with 70 random captions (the reference loops past one
wavefront, exclusions >= 64).
"""
import functools

import numpy as np

from cst_captioning_amd.data.dataset import VideoCaptionDataset
from cst_captioning_amd.prepro.ciderdf import df_from_token_refs

S = 5
WIDTH = 14  # BOS + at most 12 tokens + EOS
WORDS = ['a', 'man', 'plays', 'playing', 'guitar', 'dog', 'dogs', 'runs', 'running', 'the',
         'cat', 'walks', 'walked', 'on', 'grass', 'fast', 'dog']  # (last: a duplicate word)
VOCAB = ['<end>', '<start>', '<unk>'] + WORDS
W = {w: 3 + i for i, w in reversed(list(enumerate(WORDS)))}  # (first id of a word)
DUP_DOG = 3 + len(WORDS) - 1

HAND = [
    ['a man plays plays plays guitar', 'a man plays guitar', 'a man plays plays guitar',
     'the dog runs'],
    ['dog dog runs', 'dog dog walks', 'a cat'],
    ['a man walks on the grass', 'a man walks on the grass', 'the cat runs fast'],
    ['a dog runs'],
    ['a man plays the guitar', 'a man plays',
     'the man playing the guitar on the grass fast'],
    ['a dog runs fast', 'a dog running fast', 'the dogs runs', 'a man walked on grass',
     'a man walks on the grass', 'a DUP runs fast'],
    ['the cat walks', 'a cat walked on the grass', 'the cat runs on grass fast', 'cat',
     'a man walks the dog', 'the dog walks a man', 'dogs running fast on the grass'],
]


def _row(tokens):
    out = np.zeros(WIDTH, dtype=np.int64)
    out[0] = 1
    out[1:1 + len(tokens)] = tokens
    return out


def make_dataset(caps_per_video):
    """VideoCaptionDataset (no features) of per-video lists of token-id lists,
    with the CIDEr-D df table of its own captions (no BOS, + EOS)."""
    labels = np.stack([_row(c) for v in caps_per_video for c in v])
    counts = np.array([len(v) for v in caps_per_video])
    ends = np.cumsum(counts)
    df, n = df_from_token_refs([[list(c) + [0] for c in v] for v in caps_per_video])
    keys = np.fromiter(df.keys(), dtype=np.uint64, count=len(df))
    vals = np.fromiter(df.values(), dtype=np.float32, count=len(df))
    return VideoCaptionDataset(VOCAB, [str(i) for i in range(len(counts))], [], labels,
                               ends - counts, ends, df=(keys, vals, n))


@functools.lru_cache(maxsize=None)
def hand_dataset(big=False):
    caps = [[[DUP_DOG if w == 'DUP' else W[w] for w in c.split()] for c in v] for v in HAND]
    if big:
        rng = np.random.RandomState(5)
        caps.append([list(rng.randint(3, len(VOCAB), size=rng.randint(1, 13)))
                     for _ in range(70)])
    return make_dataset(caps)


@functools.lru_cache(maxsize=None)
def synthetic_dataset():
    from cst_captioning_amd.data import make_synthetic
    return make_synthetic('msvd', num_videos=24, vocab_size=60, seq_length=12, feat_dims=[4],
                          seed=4, mean_len=6.0)


def dataset(name):
    return {'hand': lambda: hand_dataset(False), 'big': lambda: hand_dataset(True),
            'synthetic': synthetic_dataset}[name]()


@functools.lru_cache(maxsize=None)
def reference(name, use_eos, seq_per_img=S):
    """``{metric: (Nv, S) float64}`` of the Python oracles (backend 'cpu-ref'),
    leave-one-out; read-only."""
    from cst_captioning_amd.ops.consensus import ConsensusScorer
    out = ConsensusScorer(dataset(name), use_eos=use_eos, backend='cpu-ref').scores(seq_per_img)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_meteor_stats(name, seq_per_img=S):
    """(N, 6) int64 statistics of the Python Meteor's best alignment per slot
    (n_exact, n_stem, len_h, len_r, chunks, n_pairs), leave-one-out."""
    from cst_captioning_amd.eval.metrics import Meteor
    from cst_captioning_amd.ops.consensus import consensus_slots
    from cst_captioning_amd.utils.text import sequence_tokens
    ds = dataset(name)
    words = [str(w) for w in ds.vocab]
    met = Meteor()
    met.java = False
    rows, vid, ex = consensus_slots(ds.label_start_ix, ds.label_end_ix, seq_per_img, True)
    out = []
    for r, v, e in zip(rows, vid, ex):
        refs = [[words[t] for t in sequence_tokens(g, 0)] for g in ds.gts_of(int(v))]
        if len(refs) > 1:
            refs = refs[:e] + refs[e + 1:]
        hyp = [words[t] for t in sequence_tokens(ds.labels[r], 0)]
        m, lh, lr, chunks, npairs = max((met._stats(hyp, x) for x in refs), key=met._score)
        n_stem = int(round((npairs * met.w_exact - m) / (met.w_exact - met.w_stem)))
        out.append([npairs - n_stem, n_stem, lh, lr, chunks, npairs])
    out = np.array(out, dtype=np.int64)
    out.setflags(write=False)
    return out
