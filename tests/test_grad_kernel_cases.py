"""The references and bounds of ``grad_kernel_cases.py`` proved against each
other on the CPU: a correct kernel can meet every bound the GPU tests assert
(``test_gpu_grad_kernels.py``), and a wrong one cannot."""
import numpy as np
import pytest
import torch

import grad_kernel_cases as gc

FOLD_CASES = [(37, 0), (37, 1), (300, 0), (300, 1)]


@pytest.mark.parametrize('R,zero_off', FOLD_CASES)
def test_fold_case_holds_every_row_kind(R, zero_off):
    c = gc.fold_case(R, zero_off)
    a, b, ys, yx = gc.row_weights(c)
    T_sel = c.dg_sel.size(1)
    assert T_sel < c.n and c.labels.size(1) > c.n + 1 and c.dg_xe.stride(0) > c.n
    assert not c.dg_xe.is_contiguous()
    k = c.kind[:T_sel]
    A, B, YS, YX = a[:T_sel], b[:T_sel], ys[:T_sel], yx[:T_sel]
    want = {
        'ordinary': (A != 0) & (B != 0) & (A + B != 0) & (YS != YX),
        'cancel_two_tokens': (A != 0) & (A + B == 0) & (YS != YX),
        'cancel_same_token': (A != 0) & (A + B == 0) & (YS == YX),
        'a_zero': (A == 0) & (B != 0),
        'b_zero': (A != 0) & (B == 0),
        'both_zero': (A == 0) & (B == 0),
        'same_token': (A != 0) & (B != 0) & (A + B != 0) & (YS == YX),
        'near_cancel_two_tokens': (A + B != 0) & ((A + B).abs() < 2.0 ** -11 * A.abs()) & (YS != YX),
    }
    for i, name in enumerate(gc.KINDS):
        rows = k == i
        assert int(rows.sum()) >= 2 and bool(want[name][rows].all()), name
    assert bool((ys[T_sel:] == -1).all()) and bool((a[T_sel:] == 0).all())
    # LSE moves (zero_off: the LSEs) stay where the fast exp is accurate
    d = c.lse if zero_off else c.lse[1:] - c.lse[:-1]
    assert float(d.abs().max()) <= 10.0
    assert bool((c.E[:, :, c.V:].float() == gc.PAD).all())


@pytest.mark.parametrize('R,zero_off', FOLD_CASES)
def test_fold_emulation_meets_the_bound(R, zero_off):
    """alpha (rtol 1e-5) and diag(alpha) E' (per-element bound) of the fold
    emulated in the kernel's arithmetic, against the fp64 oracle."""
    c = gc.fold_case(R, zero_off)
    al, E2 = gc.fold_emulate(c)
    ref, fl = gc.alpha_ref(c)
    assert int(fl.sum()) >= 2 * 2  # both cancelling kinds on two tokens are floored
    torch.testing.assert_close(al.double(), ref, rtol=1e-5, atol=0)
    a, b, _, _ = gc.row_weights(c)
    dead = (a + b == 0) & ~fl
    assert int(dead.sum()) > 0 and bool((al[dead] == 0).all())
    assert torch.equal(gc.bits(E2[dead]), gc.bits(c.E[dead]))  # rows without gradient untouched
    changed = gc.bits(E2[:, :, :c.V]) != gc.bits(c.E[:, :, :c.V])
    assert int(changed.sum()) > 0 and not bool((changed & ~gc.folded_columns(c)).any())
    for rows in (fl, ~fl):
        ratio = gc.fold_ratio(c, al, E2, rows=rows)
        print('fold emulation R=%d zero_off=%d floored=%s err/bound %.3f'
              % (R, zero_off, bool(rows is fl), ratio))
        assert ratio <= 1.0  # and so <= 2 of the un-doubled 2^-8 bound


@pytest.mark.parametrize('mutation', ['one_column_off', 'missing', 'wrong_sign'])
def test_fold_bound_rejects_a_wrong_onehot_term(mutation):
    c = gc.fold_case(37, 0)
    al, E2 = gc.fold_emulate(c)
    a, b, ys, yx = gc.row_weights(c)
    t, r = 0, int((c.kind[0] == gc.KINDS.index('ordinary')).nonzero()[0])
    col = int(ys[t, r])
    delta = float(a[t, r] / al[t, r])
    E3 = E2.clone()
    if mutation == 'one_column_off':
        E3[t, r, col] = c.E[t, r, col]
        E3[t, r, (col + 1) % c.V] += delta
    elif mutation == 'missing':
        E3[t, r, col] = c.E[t, r, col]
    else:
        E3[t, r, col] = c.E[t, r, col] - delta
    assert gc.fold_ratio(c, al, E3) > 100.0


class SimpleCopy:
    def __init__(self, c):
        self.__dict__.update(c.__dict__)


@pytest.mark.parametrize('zero_off', [0, 1])
def test_guard_case_overflows_and_underflows(zero_off):
    c = gc.guard_case(zero_off)
    n_listed = int(c.listed.sum())
    jump = torch.arange(c.R) % 3 == 0
    if zero_off:
        assert bool(c.listed[0].any()) and n_listed == 2 * int(jump.sum())
    else:
        assert not bool(c.listed[0].any()) and n_listed == 3 * int(jump.sum())
    d = c.lse if zero_off else c.lse[1:] - c.lse[:-1]
    big = d.abs() > 30
    assert float(d[big].abs().min()) > 70 and float(d[~big].abs().max()) <= 10  # no borderline row
    stored = c.E[:, :, :c.V].float()
    assert bool(torch.isinf(stored[c.listed]).any())
    if not zero_off:  # rows whose whole mass underflowed
        assert bool((stored[c.listed].sum(1) == 0).any())
    assert bool(torch.isfinite(stored[~c.listed]).all())
    # the stored rows that stay are an ordinary fold case
    al, E2 = gc.fold_emulate(c)
    assert gc.fold_ratio(c, al, E2, rows=~c.listed) <= 1.0
    # an exactly recomputed row (s = 1) meets the same bound
    E3 = c.E.clone()
    E3[:, :, :c.V] = torch.where(c.listed.unsqueeze(2), c.exact.float().to(gc.BF), E3[:, :, :c.V])
    c2 = SimpleCopy(c)
    c2.E = E3
    al4, E4 = gc.fold_emulate(c2, unit_s=c.listed)
    al_ref, _ = gc.alpha_ref(c, unit_s=c.listed)
    torch.testing.assert_close(al4.double(), al_ref, rtol=1e-5, atol=0)
    assert gc.fold_ratio(c, al4, E4, unit_s=c.listed, rows=c.listed) <= 1.0


def test_layouts_hold_the_ownership_edges():
    total = {name: sum(n for _, n in lay) for name, lay in gc.LAYOUTS.items()}
    assert [total[k] for k in ('n1', 'n63', 'n64', 'n65')] == [1, 63, 64, 65]
    assert 1400 < total['full'] < 1600 and total['full'] % 8 != 0
    for lay in gc.LAYOUTS.values():
        toks = [t for t, _ in lay]
        assert toks == sorted(set(toks))
    s = gc.layout_spans('full')
    CH, LONG = gc.GS_CHUNK, gc.GS_LONG
    assert s[3][1] == CH and s[5][0] == CH             # a group ends on a boundary, the next starts there
    assert s[5][1] - s[5][0] == LONG and s[5][0] % CH == 0   # exactly GS_LONG from a boundary
    assert s[6][1] - s[6][0] == LONG + 1                # the shortest long group
    lo, hi = s[9]
    assert hi - lo == 130 and lo % CH != 0 and hi // CH - lo // CH == 2  # crosses two boundaries
    assert s[11] == (10 * CH - 1, 10 * CH) and s[12] == (10 * CH, 10 * CH + 1)
    assert 650 < s[20][1] - s[20][0] < 750
    used = set(s)
    assert {1, 2, 4, 7, 8, 13, 19, 22, 29, 31} & used == set()   # empty tokens between and after


@pytest.mark.parametrize('name', sorted(gc.LAYOUTS))
def test_exact_group_sums_do_not_depend_on_the_order(name):
    x, toks = gc.group_rows(name), gc.layout_tokens(name)
    V = 40
    xd = x.double()
    assert torch.equal(torch.trunc(xd * 2.0 ** 56) * 2.0 ** -56, xd)  # the truncation drops nothing
    ref = gc.group_ref(name, gc.X_COLS, V)
    sums = torch.zeros(V, gc.X_COLS, dtype=torch.float64).index_add_(0, toks, xd)
    assert float(sums.abs().max()) < 0.125 and float(sums.abs().max()) > 0
    for seed in (1, 2):
        xp, tp, _ = gc.group_case(name, gc.X_COLS, V, True, seed)
        assert bool(torch.isnan(xp.float()).any())  # the invalid ids' rows
        assert torch.equal(gc.bits(gc.exact_group_sum(xp, tp, V)), gc.bits(ref))
    # a sequential fp64 sum in yet another order, by hand, for one token
    tok, cnt = gc.LAYOUTS[name][-1]
    rows = xd[toks == tok]
    acc = torch.zeros(gc.X_COLS, dtype=torch.float64)
    for i in reversed(range(cnt)):
        acc += rows[i]
    assert torch.equal(gc.bits(acc.float().to(gc.BF)), gc.bits(ref[tok]))
    empty = sorted(set(range(V)) - {t for t, _ in gc.LAYOUTS[name]})
    assert bool((gc.bits(ref[empty]) == 0).all())


@pytest.mark.parametrize('V', [300, 2500, 65536])
@pytest.mark.parametrize('N', [1, 255, 257, 1500])
def test_sort_case_and_its_checker(V, N):
    toks = gc.sort_case(V, N).numpy()
    valid = (toks >= 0) & (toks < V)
    if N >= 255:
        assert abs((~valid).sum() - N // 10) <= 25
        for bad in gc.invalid_ids(V):
            assert (toks == bad).any()
    if N >= 257:
        assert not valid[64:84].any() and valid[84:128].any()
        assert (toks[100:140] == 0).sum() >= 30
    order = np.argsort(np.where(valid, toks, np.iinfo(np.int64).max), kind='stable')
    stok = np.where(valid, toks, -7)[order].astype(np.int32)
    gc.check_sorted(toks, V, stok, order.astype(np.int32))
    if N >= 255:  # an id kept by its low 32 bits is caught
        alias = np.flatnonzero(toks == 2 ** 32 + 5)[0]
        nv = int(valid.sum())
        srow2 = np.concatenate([order[:nv], [alias]]).astype(np.int32)
        stok2 = np.concatenate([stok[:nv], [5]]).astype(np.int32)
        o2 = np.argsort(stok2, kind='stable')
        toks2 = toks.copy()
        with pytest.raises(AssertionError):
            gc.check_sorted(toks2, V, stok2[o2][:nv], srow2[o2][:nv])


@pytest.mark.parametrize('V,ldl,NR', gc.COLSUM_SHAPES)
def test_colsum_bound_admits_an_fp32_sum(V, ldl, NR):
    E, alpha, ref, bound = gc.colsum_case(V, ldl, NR)
    assert bool(torch.isnan(E[:, V:].float()).all()) and E.shape == (NR, ldl)
    got = (alpha.unsqueeze(1) * E[:, :V].float()).sum(0)
    assert bool(((got.double() - ref).abs() <= bound).all())
    # one row dropped, or the ragged chunk's last column lost, is far outside
    drop = ref - alpha[NR - 1].double() * E[NR - 1, :V].double()
    if 1 < NR < 2000:  # (beyond that one row is inside the rounding of the sum)
        assert bool(((drop - ref).abs() > bound).any())


@pytest.mark.parametrize('n,Bv,vdiv', gc.VGATE_SHAPES)
@pytest.mark.parametrize('G4', [8, 264])
def test_vgate_bound_admits_an_fp32_sum(n, Bv, vdiv, G4):
    dG, ref, bound = gc.vgate_case(n, Bv, vdiv, G4)
    x = dG[:, :, :G4].float().view(n, Bv, vdiv, G4)
    got = x.sum((0, 2))
    assert bool(((got.double() - ref).abs() <= bound).all())
    assert bool(torch.isnan(dG[:, :, G4:].float()).all())
