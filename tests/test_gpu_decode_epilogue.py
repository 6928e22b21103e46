"""The decode launch's epilogue (csrc/kernels/vocab.hip vocab_tr_block) at the
smallest shapes that reach every branch, through ``decode_step_test``:
H = 64, R = 70 (one full 64-row tile and a ragged one), V = 301 (three
128-column tiles, the last ragged, V % 4 != 0 for the scalar bias tail, padded
columns).

  * the inverse-CDF draw's index map (count of positions below the threshold
    -> vocabulary index, select tree -> logit): a spike holds all of a row's
    mass in fp32, so the sampled token is the spike whatever the seed;
  * the target lookup is skipped where the step's combine does not read it
    (launchers.h vocab_step_reads_target): a sampling / greedy step with
    labels gives bit-equal tokens, log-probs, LSE and exp store to the step
    without labels;
  * and kept where it is read: teacher forcing, scheduled sampling, g_xe,
    against fp32 PyTorch at test_gpu_decode_step.py's tolerances;
  * a row whose hidden state is NaN gets no sampling candidate in any tile's
    partial (race key -inf).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
E0 = torch.empty(0)
R, V, H = 70, 301, 64
N_VT = (V + 127) // 128
NONE_IDX = 0x7fffffff


def _ops():
    from cst_captioning_amd import _ext
    return _ext.ops()


def _inputs(seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    hd = torch.randn(R, H, device=DEV, generator=g).bfloat16()
    W = (torch.randn(V, H, device=DEV, generator=g) * 0.1).bfloat16()
    b = torch.randn(V, device=DEV, generator=g) * 0.5
    tgt = torch.randint(0, V, (R,), device=DEV, generator=g)
    return hd, W, b, tgt


def _step(hd, W, b, tgt, mode, save=0, eoff=E0, seed=(11, 22), step=3, ss_prob=0.0, want_xe=True):
    rng = torch.tensor(list(seed), dtype=torch.int32, device=DEV)
    out = _ops().decode_step_test(hd, E0, W, b, E0, E0, 1, tgt, eoff, save, mode, step, rng,
                                  E0, E0, 0.0, 0, 0, E0, ss_prob, want_xe)
    torch.cuda.synchronize()
    return out


def _partials(out):
    """VocabPartial (vocab_common.h) fields {m, s, zval, zlogit, zidx, xidx,
    xtgt, pad} of every (tile, row): (floats, the same words as int32)."""
    p = out[12].view(N_VT, R, 8)
    return p, p.view(torch.int32)


def _ref(hd, W, b):
    x = hd.float() @ W.float().t() + b
    return x, torch.logsumexp(x, 1)


# row r's spike sits at column off + r: offsets 0 / 70 / 140 / 210 cover every
# place of the two full tiles and the ragged tile's first 24, 231 the rest
@pytest.mark.parametrize('off', [0, 70, 140, 210, 231])
def test_draw_index_map(off):
    # hd[r] = the +-1 code of r's 7 bits, W[off + r] = 32 x that code: logit
    # 224 at the row's own column, <= 160 at every other row's (the codes
    # differ in a bit), the bias (|b| < 4) elsewhere: the spike outweighs the
    # rest of the row by e^60 and more, beyond fp32's 2^-24 next to 1 and
    # beyond the race's Gumbel range (-2.9 .. 17.4)
    rows = torch.arange(R, device=DEV)
    code = ((rows[:, None] >> torch.arange(7, device=DEV)) & 1).float() * 2 - 1
    hd = torch.zeros(R, H, device=DEV)
    hd[:, :7] = code
    W = torch.zeros(V, H, device=DEV)
    W[off + rows, :7] = 32 * code
    b = torch.randn(V, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)) * 0.5
    for seed in [(1, 2), (1234, 99), (7, 31337)]:
        out = _step(hd.bfloat16(), W.bfloat16(), b, E0, 1, seed=seed)
        tok, gsel = out[1], out[2]
        assert int(tok.min()) >= 0 and int(tok.max()) < V
        assert torch.equal(tok, off + rows), seed
        # the chosen logit is the spike's: log-prob 0 (a wrong pick gives <= -60)
        torch.testing.assert_close(gsel, torch.zeros_like(gsel), rtol=1e-5, atol=2e-4)


@pytest.mark.parametrize('mode', [1, 2])  # sampling, greedy
def test_target_skipped_where_unread(mode):
    hd, W, b, tgt = _inputs(seed=2)
    _, lse_ref = _ref(hd, W, b)
    eoff = lse_ref + 0.5
    skip = _step(hd, W, b, tgt, mode, save=2, eoff=eoff, want_xe=False)  # labels given, xt unread
    none = _step(hd, W, b, E0, mode, save=2, eoff=eoff)                   # no labels
    kept = _step(hd, W, b, tgt, mode, save=2, eoff=eoff, want_xe=True)    # g_xe reads xt
    for o in (skip, kept):
        for k in (0, 1, 2):  # lse, tokens, g_sel
            assert torch.equal(o[k], none[k]), k
        assert torch.equal(o[4].view(torch.int16), none[4].view(torch.int16))  # exp store
    pf_skip, pi_skip = _partials(skip)
    pf_none, pi_none = _partials(none)
    pf_kept, _ = _partials(kept)
    assert torch.equal(pi_skip, pi_none)  # no target: xtgt = -inf in every partial
    assert torch.isinf(pf_skip[..., 6]).all() and (pf_skip[..., 6] < 0).all()
    assert (torch.isfinite(pf_kept[..., 6]).sum(0) == 1).all()  # one tile holds the row's target


def test_target_kept_where_read():
    hd, W, b, tgt = _inputs(seed=3)
    x, lse_ref = _ref(hd, W, b)
    lp = torch.log_softmax(x, 1)
    lp_tgt = lp.gather(1, tgt[:, None]).squeeze(1)
    # teacher forcing, no g_xe: g_sel is the target's log-prob
    o = _step(hd, W, b, tgt, 0, want_xe=False)
    assert torch.equal(o[1], tgt)
    torch.testing.assert_close(o[0], lse_ref, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(o[2], lp_tgt, rtol=1e-5, atol=2e-4)
    # scheduled sampling, no g_xe: either side of the coin
    o = _step(hd, W, b, tgt, 3, ss_prob=0.5, want_xe=False)
    tok = o[1]
    assert int((tok == tgt).sum()) >= 10  # rows that took the ground truth (P(< 10 of 70) ~ 1e-10)
    assert int((tok != tgt).sum()) >= 10
    torch.testing.assert_close(o[2], lp.gather(1, tok[:, None]).squeeze(1), rtol=1e-5, atol=2e-4)
    # a sampling step whose g_xe is asked for
    o = _step(hd, W, b, tgt, 1, want_xe=True)
    torch.testing.assert_close(o[3], lp_tgt, rtol=1e-5, atol=2e-4)
    torch.testing.assert_close(o[2], lp.gather(1, o[1][:, None]).squeeze(1), rtol=1e-5, atol=2e-4)


def test_non_finite_row_has_no_candidate():
    hd, W, b, _ = _inputs(seed=5)
    bad = 37
    hd[bad] = float('nan')
    out = _step(hd, W, b, E0, 1)
    pf, pi = _partials(out)
    assert torch.isinf(pf[:, bad, 2]).all() and (pf[:, bad, 2] < 0).all()  # race key -inf
    assert (pi[:, bad, 4] == NONE_IDX).all()
    ok = torch.arange(R, device=DEV) != bad
    assert torch.isfinite(pf[:, ok, 2]).all()  # every other row: a candidate in each tile
    assert int(pi[:, ok, 4].min()) >= 0 and int(pi[:, ok, 4].max()) < V
