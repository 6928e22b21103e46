"""The backward's gradient-assembly kernels one by one (``vocab_grad.hip``,
``embed_grad.hip``) against the fp64 references of ``grad_kernel_cases.py``,
at tiny shapes built around the kernels' edges: per-element bounds from the
reference, bit equality where the kernel owes it."""
import pytest
import torch

import grad_kernel_cases as gc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF = torch.bfloat16


def _ops():
    from cst_captioning_amd import _ext
    assert _ext.available(), 'native extension must be built for GPU tests'
    return _ext.ops()


def _none(dtype=torch.float32):
    return torch.empty(0, dtype=dtype, device=DEV)


def _dirty(shape, dtype):
    """Leave a NaN-filled block of this size in the caching allocator, so the
    kernel's output is not handed freshly zeroed memory."""
    t = torch.full(shape, float('nan'), dtype=dtype, device=DEV)
    torch.cuda.synchronize()
    del t


def _fold(c, guard=False, forward_x=False, X=None, fix_total=None, zero_weights=False):
    """vgrad_fold on a case: (E' cpu, outputs on the cpu)"""
    E = c.E.to(DEV)
    dg_sel = c.dg_sel.to(DEV)
    dg_xe = c.dg_xe
    if dg_xe.numel():  # keep the row stride of the allocation (pad NaN)
        store = torch.as_strided(dg_xe, (dg_xe.size(0), dg_xe.stride(0)), (dg_xe.stride(0), 1))
        dg_xe = store.to(DEV)[:, :c.n]
        assert dg_xe.stride(0) == c.n + 2
    else:
        dg_xe = dg_xe.to(DEV)
    if zero_weights:
        dg_sel, dg_xe = torch.zeros_like(dg_sel), torch.zeros_like(dg_xe)
    g = (c.hd.to(DEV), c.wlog.to(DEV), c.blog.to(DEV), fix_total) if guard else \
        (_none(BF), _none(BF), _none(), _none(torch.int32))
    _dirty((c.n * c.R,), torch.float32)
    out = _ops().vgrad_fold(E, c.lse.to(DEV), c.y_sel.to(DEV), dg_sel, c.labels.to(DEV), dg_xe,
                            c.V, c.zero_off, *g, forward_x, X if X is not None else _none())
    torch.cuda.synchronize()
    return E.cpu(), [o.cpu() for o in out]


def _check_fold_rows(c, E2, alpha, rows, unit_s=None, tag=''):
    """the fold's contract on the given rows (bool (n, R))"""
    ref, _ = gc.alpha_ref(c, unit_s)
    al = alpha.view(c.n, c.R)
    torch.testing.assert_close(al[rows].double(), ref[rows], rtol=1e-5, atol=0)
    ratio = gc.fold_ratio(c, alpha, E2, unit_s=unit_s, rows=rows)
    print('%s fold err/bound %.3f' % (tag, ratio))
    assert ratio <= 1.0


def _check_untouched(c, E2, rows):
    same = gc.bits(E2) == gc.bits(c.E)
    keep = torch.ones(c.n, c.R, c.ldl, dtype=torch.bool)
    keep[:, :, :c.V] = ~gc.folded_columns(c)
    assert bool(same[rows][keep[rows]].all()), 'an entry outside the folded columns changed'
    assert bool((E2[:, :, c.V:].float() == gc.PAD).all()), 'pad columns written'


@pytest.mark.parametrize('R', [37, 300])
@pytest.mark.parametrize('zero_off', [0, 1])
@pytest.mark.parametrize('has_xe', [True, False])
def test_fold_matches_dense_ds(R, zero_off, has_xe):
    """alpha and diag(alpha) E' against the dense fp64 dS; every other entry
    of E, the pad columns and the rows without gradient bit-identical."""
    c = gc.fold_case(R, zero_off, has_xe)
    E2, (alpha, fix) = _fold(c)
    every = torch.ones(c.n, c.R, dtype=torch.bool)
    _check_fold_rows(c, E2, alpha, every, tag='R=%d zero_off=%d xe=%d' % (R, zero_off, has_xe))
    _check_untouched(c, E2, every)
    a, b, _, _ = gc.row_weights(c)
    _, fl = gc.alpha_ref(c)
    dead = ((a + b == 0) & ~fl).view(-1)
    assert int(dead.sum()) > 0 and bool((alpha[dead] == 0).all())  # written, as zero
    assert torch.equal(gc.bits(E2.view(-1, c.ldl)[dead]), gc.bits(c.E.view(-1, c.ldl)[dead]))
    assert int(fix.abs().sum()) == 0  # no guard asked for


@pytest.mark.parametrize('has_xe', [True, False])
def test_fold_forward_x_outputs(has_xe):
    c = gc.fold_case(37, 0, has_xe)
    E2, (alpha, fix, oh_a, oh_ys, oh_b, oh_yx) = _fold(c, forward_x=True)
    a, b, ys, yx = gc.row_weights(c)
    assert torch.equal(oh_a, a.view(-1)) and torch.equal(oh_ys.long(), ys.view(-1))
    assert torch.equal(oh_b, b.view(-1)) and torch.equal(oh_yx.long(), yx.view(-1))
    assert bool((oh_ys.view(c.n, c.R)[c.dg_sel.size(1):] == -1).all())
    if not has_xe:
        assert bool((oh_yx == -1).all())
    E1, (alpha1, _) = _fold(c)  # E is folded all the same
    assert torch.equal(gc.bits(E2), gc.bits(E1)) and torch.equal(alpha, alpha1)


@pytest.mark.parametrize('zero_off', [0, 1])
def test_range_guard_rows_recomputed(zero_off):
    c = gc.guard_case(zero_off)
    NR, V = c.n * c.R, c.V
    fix_total = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    Xs = torch.full((NR, c.H), 7.0, device=DEV)
    E2, (alpha, fix, _, _, _, _, X) = _fold(c, guard=True, forward_x=True, X=Xs, fix_total=fix_total)
    want = c.listed.view(-1).nonzero().view(-1)
    k = int(fix[0])
    assert k == want.numel() and k > 0
    assert torch.equal(fix[1:1 + k].long().sort().values, want)
    assert int(fix_total) == 5 + k
    listed, unlisted = c.listed, ~c.listed
    rowsE = E2[:, :, :V].float()
    assert bool(torch.isfinite(rowsE[listed]).all())
    # recomputed rows: exp(x - own LSE); one bf16 rounding (2^-9) + the fp32
    # logit error (< 2^-10 here), doubled; entries under the smallest normal
    # bf16 (2^-126) may flush to zero
    plain = ~gc.folded_columns(c)
    err = (rowsE.double() - c.exact).abs()
    lim = 2.0 ** -7 * c.exact + 2.0 ** -126
    sel = listed.unsqueeze(2) & plain
    print('guard zero_off=%d exp err/bound %.3f' % (zero_off, float((err / lim)[sel].max())))
    assert bool((err <= lim)[sel].all())
    _check_fold_rows(c, E2, alpha, listed, unit_s=listed, tag='guard listed')
    _check_fold_rows(c, E2, alpha, unlisted, unit_s=listed, tag='guard unlisted')
    _check_untouched(c, E2, unlisted)
    # X: untouched where not listed; listed rows = (unfolded exact E) W.  The
    # unfolded rows are those of a run with all weights zero (alpha = 0: no fold)
    assert bool((X[unlisted.view(-1)] == 7.0).all())
    E0, (alpha0, fix0, _, _, _, _, X0) = _fold(c, guard=True, forward_x=True, fix_total=fix_total,
                                                zero_weights=True)
    assert int(fix_total) == 5 + 2 * k and int(fix0[0]) == k
    assert bool((alpha0 == 0).all())
    lrows = listed.view(-1)
    assert torch.equal(X[lrows], X0[lrows])  # X comes from the row before its fold
    Eu = E0.view(NR, c.ldl)[lrows][:, :V].double()
    W = c.wlog.double()
    refX = Eu @ W
    absX = Eu @ W.abs()
    # fp32 sum of V products: V 2^-24 = 1.2e-5 of sum |terms| at worst
    assert bool(((X[lrows].double() - refX).abs() <= 1e-5 * absX).all())
    same = gc.bits(E0.view(NR, c.ldl)[lrows][:, :V]) == gc.bits(E2.view(NR, c.ldl)[lrows][:, :V])
    assert bool(same[plain.view(NR, V)[lrows]].all())


@pytest.mark.parametrize('H', [8, 64, 520])
@pytest.mark.parametrize('pad', [0, 16, 64, 512])
@pytest.mark.parametrize('NR', [1, 5, 130])
def test_scaled_rows_bitwise(H, pad, NR):
    g = torch.Generator().manual_seed(H + pad + NR)
    alpha = torch.randn(NR, generator=g)
    alpha[0] = 0.0 if NR > 1 else alpha[0]
    hd = torch.randn(NR, H, generator=g).to(BF)
    dhd = torch.randn(NR, H, generator=g)
    ldhs = H + pad
    for with_dhd in (False, True):
        d = dhd.to(DEV) if with_dhd else _none()
        _dirty((NR, ldhs), BF)
        hs = _ops().vgrad_rows(alpha.to(DEV), hd.to(DEV), ldhs, d).cpu()
        assert hs.shape == (NR, ldhs) and hs.dtype == BF
        want = (alpha.unsqueeze(1) * hd.float()).to(BF)
        assert torch.equal(gc.bits(hs[:, :H]), gc.bits(want))
        if pad:
            hi = alpha.to(BF)
            lo = (alpha - hi.float()).to(BF)
            assert torch.equal(gc.bits(hs[:, H]), gc.bits(hi))
            assert torch.equal(gc.bits(hs[:, H + 1]), gc.bits(lo))
            assert bool((gc.bits(hs[:, H + 2:]) == 0).all())
        if with_dhd:
            assert torch.equal(d.cpu().view(torch.int32),
                               (alpha.unsqueeze(1) * dhd).view(torch.int32))


@pytest.mark.parametrize('V,ldl,NR', gc.COLSUM_SHAPES)
def test_bias_column_sums(V, ldl, NR):
    E, alpha, ref, bound = gc.colsum_case(V, ldl, NR)
    Ed, ad = E.to(DEV), alpha.to(DEV)
    _dirty((V,), torch.float32)
    db = _ops().vgrad_colsum(Ed, ad, V)
    db2 = _ops().vgrad_colsum(Ed, ad, V)
    assert db.shape == (V,) and db.dtype == torch.float32
    assert torch.equal(db.view(torch.int32), db2.view(torch.int32))
    got = db.cpu()
    assert bool(torch.isfinite(got).all())  # the NaN pad columns reach no output
    err = (got.double() - ref).abs()
    print('colsum (%d, %d, %d) err/bound %.3f' % (V, ldl, NR, float((err / bound).max())))
    assert bool((err <= bound).all())


@pytest.mark.parametrize('n,Bv,vdiv', gc.VGATE_SHAPES)
@pytest.mark.parametrize('G4', [8, 264])
def test_video_gate_sums(n, Bv, vdiv, G4):
    dG, ref, bound = gc.vgate_case(n, Bv, vdiv, G4)
    _dirty((Bv, G4), torch.float32)
    out = _ops().video_gate_grad(dG.to(DEV), vdiv, G4).cpu()
    assert out.shape == (Bv, G4) and out.dtype == torch.float32
    assert bool(torch.isfinite(out).all())
    err = (out.double() - ref).abs()
    print('vgate (%d, %d, %d, %d) err/bound %.3f' % (n, Bv, vdiv, G4, float((err / bound).max())))
    assert bool((err <= bound).all())


@pytest.mark.parametrize('V', [300, 2500, 65536])
@pytest.mark.parametrize('N', [1, 255, 257, 1500])
def test_token_sort_drops_ids_outside_the_vocabulary(V, N):
    toks = gc.sort_case(V, N)
    stok, srow = _ops().token_sort(toks.to(DEV), V)
    gc.check_sorted(toks.numpy(), V, stok.cpu().numpy(), srow.cpu().numpy())


@pytest.mark.parametrize('N', [64, 257])
def test_token_sort_all_zero_tokens(N):
    toks = torch.zeros(N, dtype=torch.long)
    stok, srow = _ops().token_sort(toks.to(DEV), 300)
    gc.check_sorted(toks.numpy(), 300, stok.cpu().numpy(), srow.cpu().numpy())
    assert bool((stok == 0).all())


def test_token_group_sum_nothing_valid():
    toks = torch.tensor(gc.invalid_ids(300) * 20, dtype=torch.long)
    S = _ops().token_group_sum(torch.full((100, 8), float('nan'), dtype=BF, device=DEV),
                               toks.to(DEV), 300)
    assert bool((gc.bits(S.cpu()) == 0).all())


GROUP_CASES = [(name, C, 40) for name in sorted(gc.LAYOUTS) for C in (8, 264, 2048, 2056, 4096)]
GROUP_CASES.append(('full', 8, 65536))


@pytest.mark.parametrize('name,C,V', GROUP_CASES)
@pytest.mark.parametrize('ld_pad', [0, 40])
def test_token_group_sums_bit_exact(name, C, V, ld_pad):
    """S equals bf16(float32(exact sum)) bit for bit, zero rows for the tokens
    without entries included, in two row orders, with ids outside [0, V) (NaN
    rows) mixed in and -- ld_pad -- as a column slice of a wider NaN-padded
    tensor; the bare layout as well where its size is the point (n64)."""
    ops = _ops()
    runs = [(True, 1), (True, 2)] + ([(False, 3)] if name != 'full' else [])
    for with_invalid, seed in runs:
        x, toks, ref = gc.group_case(name, C, V, with_invalid, seed)
        wide = torch.full((x.size(0), C + ld_pad), float('nan'), dtype=BF)
        wide[:, :C] = x
        xd = wide.to(DEV)[:, :C]
        assert xd.stride(0) == C + ld_pad
        _dirty((V, C), BF)
        S = ops.token_group_sum(xd, toks.to(DEV), V).cpu()
        assert S.shape == (V, C) and S.dtype == BF
        bad = gc.bits(S) != gc.bits(ref)
        assert not bool(bad.any()), (with_invalid, seed, bad.nonzero()[:8].tolist())
