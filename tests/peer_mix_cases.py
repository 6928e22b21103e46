"""Shared inputs and oracles of the peer-mix (``--mbr_mix``) tests: the pools of
``mbr_cases`` plus a hand-made pool on which ROUGE-L and CIDEr-D choose
differently, the fp64 oracle columns (CIDEr-D, BLEU-4, ROUGE-L of every row
against the other rows of its pool; computed once per process, read-only) and
the checks both test files apply.

Tolerances are those of the single-metric tests: ``mbr_cases.tolerance`` for
the CIDEr-D column, ``sent_metric_cases.RTOL / ATOL`` (two fp32 ulps of the
fp64 oracle rounded to fp32, exact zeros exact) for BLEU-4 / ROUGE-L.
"""
import functools

import numpy as np

import mbr_cases as mc
from sent_metric_cases import ATOL, RTOL

WEIGHTS = (1.0, 5.0, 5.0)

# Rows 0 and 1 share the subsequence 10 11 12 13 (LCS 4) but no bigram; rows 0, 2
# and 3 share the bigram 14 15.  ROUGE-L (beta 1.2 favours recall): row 1 has
# P = 4/8, R = 4/6 -> 0.586, row 0 has P = 4/6, R = 4/8 -> 0.557, rows 2 and 3
# have P = R = 2/6 -> 0.333: row 1.  CIDEr-D: row 1 matches unigrams of row 0 only,
# row 0 matches every peer and two of them on a bigram: row 0.
HAND_ROWS = [[10, 11, 12, 13, 14, 15],
             [10, 20, 11, 21, 12, 22, 13, 23],
             [14, 15, 30, 31, 32, 33],
             [14, 15, 40, 41, 42, 43]]
HAND_BEST = {'CIDEr': 0, 'ROUGE_L': 1}
HAND = mc.Case('hand_rouge_vs_cider', mc._rows(HAND_ROWS, 16), 4, 0, None)


@functools.lru_cache(maxsize=None)
def cases():
    return mc.cases() + (HAND,)


def case_ids():
    return [c.name for c in cases()]


def limit_pools(G, T, seed):
    """Two pools at an LDS limit, full-width rows without EOS among them (the
    pools of ``test_gpu_mbr._limit_pools``)."""
    hyps = mc._random_pools(seed, 2, G, T, 60)
    hyps[0] = np.arange(3, 3 + T)  # full width, no EOS, all distinct
    hyps[1] = 5                     # full width, one token: tf = T
    return hyps


def oracle_parts(hyps, G, use_eos, cider=True):
    """(N, 3) fp64: the Python oracles, row i against the other rows of its
    pool as references (column 0 left 0 with ``cider=False``)."""
    from cst_captioning_amd.eval.metrics import Bleu, Rouge
    from cst_captioning_amd.utils.text import array_to_str
    hyps = np.asarray(hyps)
    strs = [array_to_str(r, use_eos) for r in hyps]
    res = {i: [s] for i, s in enumerate(strs)}
    gts = {}
    for p0 in range(0, len(strs), G):
        pool = strs[p0:p0 + G]
        for i in range(G):
            gts[p0 + i] = pool[:i] + pool[i + 1:]
    out = np.zeros((len(strs), 3))
    if cider:
        out[:, 0] = mc.oracle_scores(hyps, G, use_eos)
    out[:, 1] = np.asarray(Bleu(4).compute_score(gts, res)[1][-1], dtype=np.float64)
    out[:, 2] = np.asarray(Rouge().compute_score(gts, res)[1], dtype=np.float64)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_of(index):
    c = cases()[index]
    ref = oracle_parts(c.hyps, c.G, c.use_eos)
    ref.setflags(write=False)
    return ref


def oracle(case):
    """The oracle columns of a shared case (cached, read-only)."""
    return _oracle_of(case_ids().index(case.name))


def blend(parts, weights=WEIGHTS):
    return np.asarray(parts, dtype=np.float64) @ np.asarray(weights, dtype=np.float64)


def check_parts(parts, ref, weights=WEIGHTS):
    """(N, 3) float32 columns against the oracle columns; a zero-weight column
    is exactly 0."""
    parts = np.asarray(parts)
    assert parts.dtype == np.float32 and parts.shape == ref.shape
    for col in (1, 2):
        if not weights[col]:
            assert not parts[:, col].any()
            continue
        want = ref[:, col].astype(np.float32)
        np.testing.assert_allclose(parts[:, col], want, rtol=RTOL, atol=ATOL)
        assert np.array_equal(parts[:, col] == 0, want == 0)
    if weights[0]:
        assert np.abs(parts[:, 0] - ref[:, 0]).max() < mc.tolerance(ref[:, 0])
    else:
        assert not parts[:, 0].any()


def table_columns(score, hyps, G, use_eos, device='cpu'):
    """The second reference: BLEU-4 / ROUGE-L of the table scorers (``score`` =
    the extension's ``metric_score`` or ``metric_score_cpu``) on
    ``metric_build_tables`` of the pool rows themselves, row i with its own
    reference left out.  Returns {metric: (N,) float32 numpy}."""
    import torch
    from cst_captioning_amd import _ext
    N = len(hyps)
    lab = torch.from_numpy(np.ascontiguousarray(hyps))
    st = torch.arange(0, N, G)
    t = _ext.ops().metric_build_tables(lab, st, st + G, use_eos)
    t = {k: v.to(device) for k, v in t.items()}
    i = torch.arange(N)
    return {m: score(m, lab.to(device), (i // G).to(device), t, use_eos,
                     exclude=(i % G).to(device)).cpu().numpy()
            for m in ('Bleu_4', 'ROUGE_L')}
