"""Inputs and oracle values shared by tests/test_reward_mix.py (CPU) and
tests/test_gpu_reward_mix.py: the cases of tests/sent_metric_cases.py (imported,
not modified) with a CIDEr-D document-frequency table built from the case's own
references, and the fp64 oracle scores of the three metrics on them (computed
once per process, never modified).

Main case: 4 videos with 1 / 3 / 20 / 70 references, 249 hypotheses, T = 32:
the reference loop past one wavefront, clipping, closest-length ties, BOS
inside, empty rows.  Tiny case: T = 64, ids up to 65,534 (BLEU / ROUGE only:
CIDEr-D takes at most 63 tokens).
"""
import copy
import functools

import numpy as np

import sent_metric_cases as sm
from cst_captioning_amd.prepro.ciderdf import df_from_token_refs
from cst_captioning_amd.utils.text import sequence_tokens

WEIGHTS = (1.0, 5.0, 5.0)  # CIDEr, Bleu_4, ROUGE_L
COLS = ('CIDEr', 'Bleu_4', 'ROUGE_L')


@functools.lru_cache(maxsize=None)
def main_case():
    """(dataset with df, hyps (N, T) int64, vid (N,) int64, hand rows): the
    dataset is a copy, sent_metric_cases' own keeps ``df = None``."""
    ds0, hyps, vid, hand = sm.main_case()
    ds = copy.copy(ds0)
    refs = [[list(sequence_tokens(r, 1)) for r in ds.gts_of(v)] for v in range(ds.num_videos)]
    df, n = df_from_token_refs(refs)  # (no BOS, + EOS: as prepro/ciderdf.py index_refs)
    keys = np.fromiter(df.keys(), dtype=np.uint64, count=len(df))
    vals = np.fromiter(df.values(), dtype=np.float32, count=len(df))
    ds.df = (keys, vals, n)
    return ds, hyps, vid, hand


def tiny_case():
    return sm.tiny_case()


@functools.lru_cache(maxsize=None)
def oracle_parts(use_eos):
    """(N, 3) float64: CIDEr-D (x10, the case's df), BLEU-4, ROUGE-L of the
    Python oracles on the main case; read-only."""
    import torch
    from cst_captioning_amd.ops.cider_d import CiderDScorer
    ds, hyps, vid, _ = main_case()
    c = CiderDScorer(ds, use_eos, 'cpu', 'cpu-ref').score_reference(torch.from_numpy(hyps),
                                                                    torch.from_numpy(vid))
    out = np.stack([np.asarray(c, dtype=np.float64), sm.oracle('main', 'Bleu_4', use_eos),
                    sm.oracle('main', 'ROUGE_L', use_eos)], axis=1)
    out.setflags(write=False)
    return out


def oracle_blend(use_eos, weights=WEIGHTS):
    return oracle_parts(use_eos) @ np.asarray(weights, dtype=np.float64)


def check_parts(got, use_eos, weights=WEIGHTS, rows=None):
    """(n, 3) fp32 parts against the oracle, each column at its own scorer's
    tolerance: CIDEr-D the bound of test_gpu_kernels.py::
    test_cider_kernel_matches_oracle, BLEU / ROUGE sent_metric_cases.RTOL / ATOL
    with exact zeros; a zero-weight column is exactly 0."""
    got = np.asarray(got)
    want = oracle_parts(use_eos)
    if rows is not None:
        want = want[rows]
    assert got.dtype == np.float32 and got.shape == want.shape
    for col in range(3):
        if not weights[col]:
            assert not got[:, col].any(), COLS[col]
            continue
        g, w = got[:, col], want[:, col]
        if col == 0:
            assert np.abs(g - w).max() < 1e-4 * max(1.0, w.max()), COLS[col]
        else:
            w32 = w.astype(np.float32)
            np.testing.assert_allclose(g, w32, rtol=sm.RTOL, atol=sm.ATOL, err_msg=COLS[col])
            assert np.array_equal(g == 0, w32 == 0), COLS[col]


def check_not_vacuous(use_eos):
    """Conditions that keep the tests from being vacuous (not tolerances): at
    least half of the rows have all three metrics positive, and the (1, 5, 5)
    mix orders at least 10 % of the pairs differently from CIDEr-D alone."""
    p = oracle_parts(use_eos)
    all3 = (p[:, 0] > 0) & (p[:, 1] > 1e-3) & (p[:, 2] > 0)
    assert all3.mean() >= 0.5, all3.mean()
    mix = oracle_blend(use_eos)
    i, j = np.triu_indices(len(mix), 1)
    dc, dm = p[i, 0] - p[j, 0], mix[i] - mix[j]
    discordant = (dc * dm < 0).mean()
    assert discordant >= 0.10, discordant
    return all3.mean(), discordant
