"""The references, bounds and emulations of ``lstm_bwd_cases.py`` proved
against each other on the CPU: an fp32 emulation of the kernels' arithmetic
meets every bound the GPU tests assert (``test_gpu_lstm_bwd.py``), and every
mutation of it -- the faults the reverse recurrence invites -- does not."""
import pytest
import torch

import lstm_bwd_cases as lc

CELLS = pytest.mark.parametrize('cell', lc.CELLS, ids=[lc.CELL_NAMES[c] for c in lc.CELLS])
CHAINS = [(15, 128, 4), (8, 128, 3), (130, 128, 4)]


@CELLS
@pytest.mark.parametrize('drop_p', [0.0, 0.5])
@pytest.mark.parametrize('R,H,KD', [(65, 64, 256), (130, 128, 512), (63, 64, 320)])
def test_step_emulation_meets_the_bound(cell, drop_p, R, H, KD):
    for kw in ({}, {'has_next': False}, {'has_cprev': False}, {'has_scale': True, 'onehot': 'both'},
               {'onehot': 'same'}, {'onehot': 'a'}, {'onehot': 'b'}):
        c = lc.step_case(cell, R, H, KD, drop_p, **kw)
        d, cy = lc.step_emulate(c)
        ref_d, ref_cy = lc.step_ref(c)
        E_d, E_cy = lc.step_bound(c)
        rd, rc = lc.ratio(d, ref_d, E_d), lc.ratio(cy, ref_cy, E_cy)
        print('step emulation %s R=%d H=%d KD=%d p=%g %s: dG %.3f carry %.3f'
              % (lc.CELL_NAMES[cell], R, H, KD, drop_p, kw, rd, rc))
        assert rd <= 1.0 and rc <= 1.0
        assert float(ref_d.abs().max()) > 0


@CELLS
@pytest.mark.parametrize('fold', [False, True])
@pytest.mark.parametrize('R,H,T', CHAINS)
def test_chain_emulation_meets_the_bound(cell, fold, R, H, T):
    """max err / bound <= 1 at every step of the chain, and for dc_out"""
    c = lc.chain_case(cell, R, H, T, 0.5, fold)
    dG, cy = lc.chain_emulate(c)
    ref, ref_cy = lc.chain_ref(c)
    E, E_cy = lc.chain_bound(c)
    per_step = [lc.ratio(dG[t], ref[t], E[t]) for t in range(T)]
    rc = lc.ratio(cy, ref_cy, E_cy)
    print('chain emulation %s R=%d H=%d T=%d fold=%d: per step %s dc_out %.3f'
          % (lc.CELL_NAMES[cell], R, H, T, fold, ['%.3f' % x for x in per_step], rc))
    assert max(per_step) <= 1.0 and rc <= 1.0


@CELLS
def test_every_mutation_is_rejected(cell):
    """each mutation of the emulation leaves the chain bound by a factor > 4 on
    at least one element of some dG_t or of dc_out"""
    c = lc.chain_case(cell, 15, 128, 4, 0.5, True)
    ref, ref_cy = lc.chain_ref(c)
    E, E_cy = lc.chain_bound(c)
    muts = lc.mutations_of(cell)
    assert set(muts) <= set(lc.MUTATIONS) and len(muts) >= 8
    for m in muts:
        dG, cy = lc.chain_emulate(c, m)
        q = ((dG.double() - ref).abs() / E)[ref != 0]
        worst = max(float(q.max()), lc.ratio(cy, ref_cy, E_cy))
        share = float((q > 1).double().mean())
        print('%s %s: worst err/bound %.1f, %.0f%% of the elements outside'
              % (lc.CELL_NAMES[cell], m, worst, 100 * share))
        assert worst > 4.0, m


@CELLS
def test_step_mutations_are_rejected(cell):
    """the same on the single-step bound (what the step kernel's tests assert)"""
    c = lc.step_case(cell, 65, 128, 512, 0.5, 7, True, True, True, 'both')
    ref_d, ref_cy = lc.step_ref(c)
    E_d, E_cy = lc.step_bound(c)
    for m in lc.mutations_of(cell):
        if m == 'stale_dg_next':  # (a chain fault)
            continue
        d, cy = lc.step_emulate(c, m)
        worst = max(lc.ratio(d, ref_d, E_d), lc.ratio(cy, ref_cy, E_cy))
        print('%s %s: worst err/bound %.1f' % (lc.CELL_NAMES[cell], m, worst))
        assert worst > 4.0, m


@CELLS
def test_cases_hold_what_they_claim(cell):
    c = lc.chain_case(cell, 130, 128, 4, 0.5, True)
    assert c.whhT.dtype == lc.BF and c.whhT.shape == (128, 512) and c.whhT.is_contiguous()
    assert c.gates.dtype == lc.BF and c.gates.shape == (4, 130, 512) and c.gates.stride() == (130 * 512, 512, 1)
    assert c.dh.dtype == torch.float32 and c.dh.stride() == (130 * 128, 128, 1)
    assert c.c_all.dtype == torch.float32 and c.c_all.stride() == (130 * 128, 128, 1)
    assert float(c.c_all.abs().max()) <= 8.0
    sat = c.c_all[..., ::7]
    assert bool((sat.abs() >= 4.0).all()) and bool((c.c_all[..., 0].abs() == 8.0).all())
    assert bool(((1.0 - torch.tanh(sat.double()) ** 2) < 2e-3).all())  # saturated units
    assert bool((c.c_all[..., 1::7].abs() <= 3.5).all())
    s = c.gates.float().view(4, 130, 128, 4)
    if cell == lc.LSTM:
        assert bool(((s[..., [0, 1, 3]] >= 0) & (s[..., [0, 1, 3]] <= 1)).all())
        assert bool((s[..., 2].abs() <= 1).all()) and bool((s[..., 2] < 0).any())
    elif cell == lc.GRU:
        assert bool(((s[..., :2] >= 0) & (s[..., :2] <= 1)).all())
        assert bool((s[..., 2].abs() <= 1).all()) and float(s[..., 3].abs().max()) > 1.0
    else:
        assert bool((s[..., 0].abs() <= 1).all()) and bool((s[..., 1:] == 0).all())
    # dropped and kept elements in every 64-row x 64-unit tile of every step
    for t in range(c.T):
        k = lc.keep_mask(c.seed, t, 130, 128, 0.5)
        for r0 in range(0, 130, 64):
            for u0 in range(0, 128, 64):
                tile = k[r0:r0 + 64, u0:u0 + 64]
                assert bool(tile.any()) and not bool(tile.all())
    # tokens -1 carry the weight 0; no token selects the large row 0 of W
    for w, y in ((c.oh.a, c.oh.ys), (c.oh.b, c.oh.yx)):
        assert y.dtype == torch.int32 and w.shape == y.shape == (4, 130)
        assert int((y == -1).sum()) >= 4 and bool((w[y == -1] == 0).all())
        assert bool((y != 0).all()) and int(y.max()) < lc.OH_V and bool((w[y >= 0] != 0).all())
    assert bool((c.oh.W[0].float() == lc.OH_BIG).all()) and float(c.oh.W[1:].float().abs().max()) < 1.0
    # step cases: the tail columns of dg_next / whhT take part in the GEMM
    sc = lc.step_case(cell, 63, 64, 320)
    assert sc.dg_next.shape == (63, 320) and sc.whhT.shape == (64, 320)
    assert float(sc.dg_next[:, 256:].float().abs().max()) > 0
    same = lc.step_case(cell, 65, 64, 256, onehot='same')
    assert torch.equal(same.oh.ys, same.oh.yx)
    assert lc.step_case(cell, 65, 64, 256, onehot='a').oh.b is None
    assert lc.step_case(cell, 65, 64, 256, onehot='b').oh.a is None


def test_keep_mask_share_and_keys():
    R, H = 130, 128
    n = R * H
    for p in (0.25, 0.5):
        for step in (0, 7, 65539):
            k = lc.keep_mask(lc.SEED, step, R, H, p)
            share = float(k.double().mean())
            assert abs(share - (1 - p)) <= 3 * (p * (1 - p) / n) ** 0.5, (p, step, share)
    # steps t, t + 1 and 65536 + t (the drop key of a lower layer) draw different masks
    for t in (0, 3):
        a, b, c = (lc.keep_mask(lc.SEED, s, R, H, 0.5) for s in (t, t + 1, 65536 + t))
        for x, y in ((a, b), (a, c), (b, c)):
            d = float((x != y).double().mean())
            assert abs(d - 0.5) <= 3 * (0.25 / n) ** 0.5
    assert not torch.equal(lc.keep_mask(lc.SEED, 0, R, H, 0.5), lc.keep_mask(lc.SEED + 1, 0, R, H, 0.5))


def test_attention_epilogue_reference():
    """dal_ref against a plain loop, pad frames zero, the admitted vdiv"""
    assert lc.smallest_vdiv(8, 128) == 7 and lc.smallest_vdiv(12, 128) == 16
    assert lc.att_epi_ok(20, 12, 128) and not lc.att_epi_ok(6, 8, 128)
    R, H, vdiv, C = 70, 128, 7, 8
    gv = lc.gate_table(R, H, vdiv, C)
    assert gv.shape == (10, H, 8, 4)
    gv12 = lc.gate_table(R, H, 20, 12)
    assert gv12.shape == (4, H, 16, 4) and bool((gv12[:, :, 12:] == 0).all())
    d, _ = lc.step_emulate(lc.step_case(lc.LSTM, R, H))
    ref, bound = lc.dal_ref(d, gv, vdiv), lc.dal_bound(d, gv, vdiv)
    assert ref.shape == (2, R, 8)
    for (ut, r, c) in ((0, 0, 0), (1, 69, 7), (1, 13, 3)):
        x = sum(float(d[r, 4 * u + g]) * float(gv[r // vdiv, u, c, g])
                for u in range(64 * ut, 64 * ut + 64) for g in range(4))
        assert abs(x - float(ref[ut, r, c])) <= 1e-12 * max(1.0, abs(x))
    assert bool((bound > 0).all())
