"""Shared cases of the token-space validation scorer tests
(``test_corpus_metrics.py``, ``test_gpu_corpus_metrics.py``).

A hand-written English vocabulary (40 words after the three specials, 19
distinct stems under the project's stemmer), splits of 1, 13 and 24 videos with
1 to 70 references of 1 to 64 tokens, and one hypothesis per video.  The first
thirteen videos are hand-made edge cases (see ``_special``); the others are
random, half of the hypotheses a reference with 30 % of its words replaced.
The oracle results (``backend='cpu-ref'``) are computed once per split and
shared; callers must not modify them.
"""
import functools

import numpy as np

from cst_captioning_amd.data.dataset import VideoCaptionDataset
from cst_captioning_amd.prepro.vocab import SPECIALS

WORDS = ('a the man men woman women run running runs ran walk walking walked walks dog dogs is '
         'are play playing plays played cook cooking cooks cooked talk talking talks talked car '
         'cars drive driving drives song songs sing singing sings').split()
VOCAB = list(SPECIALS) + WORDS
ID = {w: i for i, w in enumerate(VOCAB)}
T = 64           # hypothesis width
L = 66           # label row: BOS + up to 64 tokens + EOS
SIZES = (1, 13, 24)
BOS = 1


def ids(sentence):
    return [ID[w] for w in sentence.split()]


def _rand_sentence(rng, n, exclude=()):
    pool = [ID[w] for w in WORDS if w not in exclude]
    return [int(pool[k]) for k in rng.randint(len(pool), size=n)]


def _perturb(rng, ref):
    out = list(ref)
    for k in range(len(out)):
        if rng.rand() < 0.3:
            out[k] = int(rng.randint(len(SPECIALS), len(VOCAB)))
    return out


def _special(rng):
    """[(references, hypothesis)] of the hand-made videos.  A hypothesis is a
    token list (EOS padding is added) and may hold BOS."""
    song = ID['song']
    long_ref = _rand_sentence(rng, 63, exclude=('song', 'songs')) + [song]
    cases = [
        # a single reference, and its exact copy
        ([ids('a man is running')], ids('a man is running')),
        # more than 64 references; the empty hypothesis
        ([_rand_sentence(rng, int(rng.randint(1, 13))) for _ in range(70)], []),
        # references of length 1 and 64; a hypothesis of length 1
        ([ids('dog'), _rand_sentence(rng, 64), ids('the dog runs')], ids('dogs')),
        # 64 tokens without EOS; the pair (0, 63) makes the next wanted position 64
        ([long_ref, _rand_sentence(rng, 40)],
         [song] + [long_ref[k] for k in rng.randint(63, size=63)]),
        # BOS in the middle of the hypothesis
        ([ids('a man is running'), ids('the man runs')], ids('a man') + [BOS] + ids('is running')),
        # a repeated word that outnumbers its copies in the references
        ([ids('the dog runs'), ids('the dog is running the car')], ids('the the the the dog')),
        # crossing alignments
        ([ids('a man walks the dog')], ids('the dog walks a man')),
        # equidistant candidates, exact stage: after (0, 1), 'dog' wants 2 and finds
        # 0 and 4.  The smaller j wins: (1, 0), then 'are' (2, 5) is a third chunk.
        # With j = 4, (1, 4) (2, 5) would be adjacent: two chunks.
        ([ids('dog a man the dog are')], ids('a dog are')),
        # stem stage only: runs/running, dog/dogs, cooks/cooked
        ([ids('men running dogs cooked'), ids('women talk')], ids('man runs dog cooks talking')),
        # exact and stem stages mixed, two chunks
        ([ids('the woman is singing a song'), ids('a woman sings songs')],
         ids('a woman is sings the song')),
        # references of every other length class
        ([_rand_sentence(rng, n) for n in (2, 3, 5, 17, 31, 33, 63)], _rand_sentence(rng, 30)),
        ([_rand_sentence(rng, n) for n in (4, 8, 16, 32)], None),
        # equidistant candidates, stem stage: the exact stage pairs (0, 1) and
        # (2, 5); then 'dog' wants 2 and finds the stems of 'dogs' at 0 and 4.
        # (1, 0): three chunks; with j = 4 it would be two.
        ([ids('dogs a man the dogs are')], ids('a dog are')),
    ]
    return cases


def _random_video(rng):
    refs = [_rand_sentence(rng, int(rng.randint(1, 16))) for _ in range(int(rng.randint(1, 8)))]
    return refs, None


@functools.lru_cache(maxsize=None)
def make_case(nv, seed=0):
    """(dataset, seqs (nv, 64) int64, video_index (nv,) int64) of an ``nv``-video
    split.  Row i of ``seqs`` is the hypothesis of video ``video_index[i]``."""
    rng = np.random.RandomState(1000 + seed)
    videos = _special(rng)[:nv]
    while len(videos) < nv:
        videos.append(_random_video(rng))
    rows, start, end, hyps = [], [], [], []
    for k, (refs, hyp) in enumerate(videos):
        start.append(len(rows))
        for r in refs:
            assert 1 <= len(r) <= 64
            rows.append([BOS] + list(r) + [0] * (L - 1 - len(r)))
        end.append(len(rows))
        if hyp is None:  # half: a reference with 30 % of its words replaced
            hyp = _perturb(rng, refs[int(rng.randint(len(refs)))]) if k % 2 == 0 \
                else _rand_sentence(rng, int(rng.randint(1, 16)))
        assert len(hyp) <= T
        hyps.append(list(hyp) + [0] * (T - len(hyp)))
    ds = VideoCaptionDataset(VOCAB, [str(i) for i in range(nv)],
                             [np.zeros((nv, 1, 4), np.float32)], np.array(rows, np.int64),
                             np.array(start), np.array(end))
    perm = rng.permutation(nv).astype(np.int64)
    seqs = np.array(hyps, np.int64)[perm]
    seqs.setflags(write=False)
    perm.setflags(write=False)
    return ds, seqs, perm


@functools.lru_cache(maxsize=None)
def reference(nv, seed=0):
    """The oracle's result for ``make_case(nv, seed)`` (computed once)."""
    from cst_captioning_amd.ops.corpus_metrics import CorpusScorer
    ds, seqs, vi = make_case(nv, seed)
    return CorpusScorer(ds, 'cpu', 'cpu-ref').score(seqs, vi)


@functools.lru_cache(maxsize=None)
def meteor_near_ties(nv, seed=0):
    """Per hypothesis: does the oracle's runner-up reference have different
    statistics and a score within 1e-9 relative of the best one's?"""
    from cst_captioning_amd.eval.metrics import Meteor
    from cst_captioning_amd.utils.text import sequence_tokens
    ds, seqs, vi = make_case(nv, seed)
    met = Meteor()
    met.java = False
    out = []
    for row, v in zip(seqs, vi):
        hyp = [VOCAB[t] for t in sequence_tokens(row, 0)]
        stats = [met._stats(hyp, [VOCAB[t] for t in sequence_tokens(r, 0)])
                 for r in ds.gts_of(int(v))]
        best = max(stats, key=met._score)
        sb = met._score(best)
        # (all references scoring exactly 0 is no exception: the first one wins in
        # every backend, so those segments are compared like the others)
        out.append(sb > 0 and any(st != best and abs(met._score(st) - sb) <= 1e-9 * sb
                                  for st in stats))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def changed_by_opposite_tie_break(nv, seed=0):
    """Per hypothesis: do the oracle's best-reference statistics change when an
    equidistant candidate pair is decided for the LARGER j, i.e. with the key
    ``(|j - want|, -j)`` in place of ``Meteor._align``'s ``(|j - want|, j)``?
    Where they do, the case pins the tie-break of the backends."""
    from cst_captioning_amd.eval.metrics import Meteor
    from cst_captioning_amd.eval.stem import stem
    from cst_captioning_amd.utils.text import sequence_tokens

    class LargerJ(Meteor):
        def _align(self, h, r):  # Meteor._align but for the sign of j in the key
            used = [False] * len(r)
            pairs = []
            for stage, key in ((self.w_exact, lambda w: w), (self.w_stem, stem)):
                for i, w in enumerate(h):
                    if any(p[0] == i for p in pairs):
                        continue
                    kw = key(w)
                    cands = [j for j in range(len(r)) if not used[j] and key(r[j]) == kw]
                    if not cands:
                        continue
                    prev = max((p for p in pairs if p[0] < i), default=None)
                    want = prev[1] + 1 if prev else 0
                    j = min(cands, key=lambda j: (abs(j - want), -j))
                    used[j] = True
                    pairs.append((i, j, stage))
            return sorted(pairs)

    ds, seqs, vi = make_case(nv, seed)
    out = []
    for row, v in zip(seqs, vi):
        hyp = [VOCAB[t] for t in sequence_tokens(row, 0)]
        refs = [[VOCAB[t] for t in sequence_tokens(r, 0)] for r in ds.gts_of(int(v))]
        best = []
        for met in (Meteor(), LargerJ()):
            met.java = False
            best.append(max((met._stats(hyp, r) for r in refs), key=met._score))
        out.append(best[0] != best[1])
    return np.array(out)


def check_against_oracle(got, nv, seed=0):
    """The bounds of the scorer against the oracle, for a table-based backend's
    result ``got`` on ``make_case(nv, seed)``."""
    ref = reference(nv, seed)
    gs, rs = got['segments'], ref['segments']
    # BLEU: integer statistics exactly, corpus values to 1e-12 relative
    assert np.array_equal(gs['bleu_stats'], rs['bleu_stats'])
    for k in range(1, 5):
        g, r = got['scores']['Bleu_%d' % k], ref['scores']['Bleu_%d' % k]
        assert abs(g - r) <= 1e-12 * abs(r), (k, g, r)
    # METEOR: scores to 1e-9 relative; the six integers wherever the oracle's
    # choice of the best reference is not a near-tie between different statistics
    ties = meteor_near_ties(nv, seed)
    assert ties.mean() <= 0.05, ties.mean()
    np.testing.assert_allclose(gs['METEOR'], rs['METEOR'], rtol=1e-9, atol=0)
    assert np.array_equal(gs['meteor_stats'][~ties], rs['meteor_stats'][~ties])
    g, r = got['scores']['METEOR'], ref['scores']['METEOR']
    assert abs(g - r) <= 1e-9 * abs(r), (g, r)
    # ROUGE-L: two fp32 ulps at 1.0
    assert abs(got['scores']['ROUGE_L'] - ref['scores']['ROUGE_L']) <= 2.4e-7
    # CIDEr: the bound of test_cider_kernel_matches_oracle
    tol = 1e-4 * max(1.0, float(rs['CIDEr'].max()))
    assert np.abs(gs['CIDEr'] - rs['CIDEr']).max() <= tol
    assert abs(got['scores']['CIDEr'] - ref['scores']['CIDEr']) <= tol
