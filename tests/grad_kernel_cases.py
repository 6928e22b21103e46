"""Shared cases and fp64 references of the gradient-assembly kernel tests
(``csrc/kernels/vocab_grad.hip``, ``csrc/kernels/embed_grad.hip``): built once
per process on the CPU, never modified.  ``test_grad_kernel_cases.py`` proves
the references and the stated bounds against each other without a GPU;
``test_gpu_grad_kernels.py`` holds the kernels to them.

Vocab head.  Row (t, r) carries a weight ``a`` on its chosen token ``ys`` and a
weight ``b`` on its target token ``yx``; the dense gradient of the logits is
    dS = a onehot(ys) + b onehot(yx) - (a + b) softmax(x).
The kernels never form it: the rollout stored ``E = bf16(exp(x - c))`` (``c``
the previous step's LSE; its own at step 0; 0 with ``zero_off``), and
``vgrad_onehot`` writes ``alpha = -(a + b) exp(c - lse)`` and folds the one-hot
terms into the row's own entries of E, so that ``dS = diag(alpha) E'``.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

BF = torch.bfloat16
PAD = 768.0            # sentinel of the pad columns V..ldl of an exp store
EXP_SAFE_LSE_JUMP = 60.0
FLOOR = 2.0 ** -10     # |alpha| >= FLOOR (|a| + |b|) s on rows whose weights cancel on two tokens

# what a row of a fold case exercises (assigned round-robin over the flat rows)
KINDS = ('ordinary', 'cancel_two_tokens', 'cancel_same_token', 'a_zero', 'b_zero', 'both_zero',
         'same_token', 'near_cancel_two_tokens')


def bits(t):
    """bf16 tensor -> its 16-bit patterns (int16), for bit comparisons"""
    assert t.dtype == BF
    return t.contiguous().view(torch.int16)


# ---- vocab head: weights, stores, oracle, emulation, bound ---------------------

def _weights(n, R, V, T_sel, g, has_sel=True, has_xe=True):
    """y_sel / dg_sel (R, T_sel), labels (R, n + 3), dg_xe (R, n) inside an
    (R, n + 2) allocation, and the kind of every row (n, R)."""
    L = n + 3
    y_sel = torch.randint(0, V, (R, T_sel), generator=g)
    labels = torch.randint(0, V, (R, L), generator=g)
    dg_sel = torch.randn(R, T_sel, generator=g)
    dg_store = torch.full((R, n + 2), float('nan'))
    dg_store[:, :n] = torch.randn(R, n, generator=g)
    dg_xe = dg_store[:, :n]  # row stride n + 2
    kind = torch.empty(n, R, dtype=torch.long)
    for t in range(n):
        for r in range(R):
            k = (t * R + r) % len(KINDS)
            kind[t, r] = k
            name = KINDS[k]
            sel = t < T_sel
            if sel and labels[r, t + 1] == y_sel[r, t]:  # the builder decides which rows coincide
                labels[r, t + 1] = (int(y_sel[r, t]) + 1 + int(torch.randint(0, V - 1, (1,), generator=g))) % V
            if name in ('cancel_two_tokens', 'cancel_same_token') and sel:
                dg_xe[r, t] = -dg_sel[r, t]
            if name == 'near_cancel_two_tokens' and sel:
                dg_xe[r, t] = -dg_sel[r, t] * (1.0 + 2.0 ** -12)
            if name in ('cancel_same_token', 'same_token') and sel:
                labels[r, t + 1] = y_sel[r, t]
            if name in ('a_zero', 'both_zero') and sel:
                dg_sel[r, t] = 0.0
            if name in ('b_zero', 'both_zero'):
                dg_xe[r, t] = 0.0
    empty_l, empty_f = torch.empty(0, dtype=torch.long), torch.empty(0)
    if not has_sel:
        y_sel, dg_sel = empty_l, empty_f
    if not has_xe:
        labels, dg_xe = empty_l, empty_f
    return y_sel, dg_sel, labels, dg_xe, kind


def row_weights(c):
    """(a, b, ys, yx), each (n, R): the weights and tokens of every row as the
    backward defines them (token -1: no such term); a, b fp32."""
    n, R = c.n, c.R
    a, b = torch.zeros(n, R), torch.zeros(n, R)
    ys = torch.full((n, R), -1, dtype=torch.long)
    yx = torch.full((n, R), -1, dtype=torch.long)
    if c.dg_sel.numel():
        T = c.dg_sel.size(1)
        a[:T] = c.dg_sel.t()
        ys[:T] = c.y_sel.t()
    if c.dg_xe.numel():
        b[:] = c.dg_xe[:, :n].t()
        yx[:] = c.labels[:, 1:n + 1].t()
    return a, b, ys, yx


def store_offsets(lse, zero_off):
    """c (n, R) fp64: the offset the forward subtracted before the exp"""
    lse = lse.double()
    return torch.zeros_like(lse) if zero_off else torch.cat([lse[:1], lse[:-1]], 0)


def exp_store(x64, lse, zero_off, ldl):
    """E (n, R, ldl) bf16 = exp(x - c), pad columns PAD"""
    n, R, V = x64.shape
    E = torch.full((n, R, ldl), PAD, dtype=BF)
    E[:, :, :V] = torch.exp(x64 - store_offsets(lse, zero_off).unsqueeze(2)).float().to(BF)
    return E


@functools.lru_cache(maxsize=None)
def fold_case(R, zero_off, has_xe=True, n=3, V=203, ldl=256, seed=0):
    """Rows of every kind in KINDS in the same tensors; T_sel = n - 1 < n;
    per-step LSE moves (and, with zero_off, the LSEs themselves) within +-10."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * R + zero_off)
    shift = torch.rand(n, R, 1, generator=g, dtype=torch.float64) * 8 - 4
    x64 = torch.randn(n, R, V, generator=g, dtype=torch.float64) + shift - math.log(V)
    lse = torch.logsumexp(x64, 2).float()
    y_sel, dg_sel, labels, dg_xe, kind = _weights(n, R, V, n - 1, g, has_xe=has_xe)
    c = SimpleNamespace(n=n, R=R, V=V, ldl=ldl, zero_off=zero_off, x64=x64, lse=lse,
                        E=exp_store(x64, lse, zero_off, ldl), y_sel=y_sel, dg_sel=dg_sel,
                        labels=labels, dg_xe=dg_xe, kind=kind)
    return c


def dense_ds(c):
    """(dS, p) fp64 (n, R, V) from the fp64 logits"""
    a, b, ys, yx = (t.double() if t.is_floating_point() else t for t in row_weights(c))
    p = torch.softmax(c.x64, 2)
    dS = -(a + b).unsqueeze(2) * p
    for w, y in ((a, ys), (b, yx)):
        has = (y >= 0).unsqueeze(2)
        dS.scatter_add_(2, y.clamp(min=0).unsqueeze(2), torch.where(has, w.unsqueeze(2), 0.0))
    return dS, p


def _floored(a, b, ys, yx, al, s):
    """rows where the kernel keeps |alpha| at FLOOR (|a| + |b|) s"""
    two = (a != 0) & (b != 0) & (ys >= 0) & (yx >= 0) & (ys != yx)
    return two & (al.abs() < FLOOR * (a.abs() + b.abs()) * s)


def alpha_ref(c, unit_s=None):
    """(alpha fp64 (n, R), floored bool (n, R)) from the fp32 inputs, in fp64;
    unit_s (bool (n, R)): rows whose E carries its own LSE as offset (s = 1)"""
    a, b, ys, yx = row_weights(c)
    a, b = a.double(), b.double()
    s = torch.exp(store_offsets(c.lse, c.zero_off) - c.lse.double())
    if unit_s is not None:
        s = torch.where(unit_s, torch.ones_like(s), s)
    al = -(a.float() + b.float()).double() * s  # the sum a + b is one fp32 rounding of the inputs
    fl = _floored(a, b, ys, yx, al, s)
    floor_al = FLOOR * (a.abs() + b.abs()) * s
    al = torch.where(fl, torch.where(al < 0, -floor_al, floor_al), al)
    return al, fl


def fold_emulate(c, unit_s=None):
    """(alpha fp32 (n, R), E' bf16 (n, R, ldl)): the fold with the kernel's
    arithmetic in plain torch -- fp32 s and alpha, the floor, one bf16
    round-to-nearest-even per folded entry of the stored bf16 E.  unit_s: rows
    with s = 1 (as alpha_ref)."""
    a, b, ys, yx = row_weights(c)
    lse = c.lse
    off = torch.zeros_like(lse) if c.zero_off else torch.cat([lse[:1], lse[:-1]], 0)
    s = torch.exp(off - lse)
    if unit_s is not None:
        s = torch.where(unit_s, torch.ones_like(s), s)
    al = -(a + b) * s
    fl = _floored(a, b, ys, yx, al, s)
    floor_al = torch.tensor(FLOOR, dtype=torch.float32) * (a.abs() + b.abs()) * s
    al = torch.where(fl, torch.where(al < 0, -floor_al, floor_al), al)
    E = c.E.clone()
    live = al != 0
    inv = torch.where(live, 1.0 / torch.where(live, al, torch.ones_like(al)), torch.zeros_like(al))
    us, ux = live & (a != 0) & (ys >= 0), live & (b != 0) & (yx >= 0)
    same = us & ux & (ys == yx)

    def add(mask, y, w):
        t, r = mask.nonzero(as_tuple=True)
        col = y[t, r]
        E[t, r, col] = (E[t, r, col].float() + w[t, r] * inv[t, r]).to(BF)

    add(same, ys, a + b)
    add(us & ~same, ys, a)
    add(ux & ~same, yx, b)
    return al, E


def fold_bound(c, p, floored):
    """per-element bound (n, R, V) fp64 on |alpha E' - dS|.
    E is rounded to bf16 once when stored and once when folded (2^-9 each):
    2^-8 of the entry's terms, with a factor 2 of margin = 2^-7; 1e-6 (|a| +
    |b|) covers the fp32 exp / reciprocal.  A floored row's softmax part is
    alpha_floor E instead of -(a + b) s E: off by the documented 2^-10 (|a| +
    |b|), spread by p and the one-hot entries -- and alpha_floor E carries the
    same two roundings, so on those rows the rounding term counts |alpha| / s
    = 2^-10 (|a| + |b|) where that exceeds |a + b| (on a peaked row, p ~ 1,
    the rounding of the floored part alone is 2^-19 (|a| + |b|) > 1e-6 (|a| +
    |b|): the emulation reaches 1.0003 of the bound without it)."""
    wa, wb, ys, yx = row_weights(c)
    a, b = wa.double().abs(), wb.double().abs()
    ab = (wa.double() + wb.double()).abs()
    eff = torch.where(floored, torch.maximum(ab, FLOOR * (a + b)), ab)
    oh_a = torch.zeros_like(p)
    oh_b = torch.zeros_like(p)
    oh_a.scatter_(2, ys.clamp(min=0).unsqueeze(2), (ys >= 0).double().unsqueeze(2))
    oh_b.scatter_(2, yx.clamp(min=0).unsqueeze(2), (yx >= 0).double().unsqueeze(2))
    bound = 2.0 ** -7 * (a.unsqueeze(2) * oh_a + b.unsqueeze(2) * oh_b + eff.unsqueeze(2) * p)
    bound = bound + 1e-6 * (a + b).unsqueeze(2)
    extra = FLOOR * (a + b).unsqueeze(2) * (p + oh_a + oh_b)
    return bound + torch.where(floored.unsqueeze(2), extra, torch.zeros_like(extra))


def folded_columns(c):
    """bool (n, R, V): the one or two entries of each row a fold may rewrite"""
    a, b, ys, yx = row_weights(c)
    m = torch.zeros(c.n, c.R, c.V, dtype=torch.bool)
    for w, y in ((a, ys), (b, yx)):
        one = torch.zeros_like(m)
        one.scatter_(2, y.clamp(min=0).unsqueeze(2), ((w != 0) & (y >= 0)).unsqueeze(2))
        m |= one
    return m


def fold_ratio(c, alpha, E_folded, unit_s=None, rows=None):
    """max over the elements (of the given rows) of |alpha E' - dS| / bound"""
    dS, p = dense_ds(c)
    _, fl = alpha_ref(c, unit_s)
    got = alpha.double().view(c.n, c.R, 1) * E_folded[:, :, :c.V].double()
    err, bound = (got - dS).abs(), fold_bound(c, p, fl)
    # (a row without weights has bound 0 and must be reproduced as exact zeros)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    if rows is not None:
        ratio = ratio[rows]
    return float(ratio.max())


# ---- range guard ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def guard_case(zero_off, n=4, R=24, H=128, V=203, ldl=256, seed=0):
    """Every third row's vocab input is scaled x60 on alternate steps, so its
    LSE moves by about +-100 between steps (stored E overflows to inf or loses
    the row to underflow); zero_off: steps 0 and 2, so |lse| > 60 at step 0."""
    g = torch.Generator().manual_seed(77 + zero_off + seed)
    wlog = (torch.rand(V, H, generator=g) * 0.2 - 0.1).to(BF)
    blog = torch.randn(V, generator=g) * 0.1
    scale = torch.ones(n, R, 1)
    jump = torch.arange(R) % 3 == 0
    scale[(0 if zero_off else 1)::2, jump] = 60.0
    hd = (torch.randn(n, R, H, generator=g) * scale).to(BF)
    x64 = hd.double() @ wlog.double().t() + blog.double()
    lse = torch.logsumexp(x64, 2).float()
    y_sel, dg_sel, labels, dg_xe, kind = _weights(n, R, V, n - 1, g)
    c = SimpleNamespace(n=n, R=R, V=V, H=H, ldl=ldl, zero_off=zero_off, x64=x64, lse=lse,
                        E=exp_store(x64, lse, zero_off, ldl), y_sel=y_sel, dg_sel=dg_sel,
                        labels=labels, dg_xe=dg_xe, kind=kind, hd=hd.view(n * R, H), wlog=wlog,
                        blog=blog)
    d = lse if zero_off else torch.cat([torch.zeros(1, R), lse[1:] - lse[:-1]], 0)  # fp32, as the kernel
    c.listed = d.abs() > EXP_SAFE_LSE_JUMP  # (n, R)
    c.exact = torch.exp(x64 - lse.double().unsqueeze(2))  # E of a listed row (own LSE as offset)
    return c


# ---- per-token sums --------------------------------------------------------------

def invalid_ids(V):
    """ids outside [0, V); the last two alias tokens 5 and 0 in their low 32 bits"""
    return [-1, V, V + 7, 2 ** 32 + 5, -2 ** 40]


# (token, entries), tokens ascending: the sorted layout is the concatenation
LAYOUTS = {
    'n1': [(7, 1)],
    'n63': [(1, 63)],
    'n64': [(1, 64)],
    'n65': [(1, 65)],
    'full': [(0, 50), (3, 14),   # [0, 50), [50, 64): ends exactly on a chunk boundary
             (5, 192),           # [64, 256): starts there, exactly GS_LONG, two whole chunks inside
             (6, 193),           # [256, 449): long
             (9, 130),           # [449, 579): starts mid-chunk, crosses 512 and 576
             (10, 60),           # [579, 639)
             (11, 1), (12, 1),   # 639 and 640: single rows either side of a boundary
             (20, 701),          # [641, 1342): long, ten whole chunks inside
             (21, 100), (30, 65)],  # [1342, 1442), [1442, 1507)
}
GS_CHUNK, GS_LONG = 64, 192


def layout_spans(name):
    """{token: (start, end)} in the sorted order"""
    out, pos = {}, 0
    for tok, cnt in LAYOUTS[name]:
        out[tok] = (pos, pos + cnt)
        pos += cnt
    return out


def layout_tokens(name):
    return torch.cat([torch.full((cnt,), tok, dtype=torch.long) for tok, cnt in LAYOUTS[name]])


X_COLS = 4096


@functools.lru_cache(maxsize=None)
def group_rows(name):
    """gradient-sized bf16 rows (entries of the layout, X_COLS), in token order"""
    g = torch.Generator().manual_seed(31 + len(name) + sum(c for _, c in LAYOUTS[name]))
    N = sum(c for _, c in LAYOUTS[name])
    return (torch.randn(N, X_COLS, generator=g) * 1e-4).to(BF)


def exact_group_sum(x, toks, V):
    """S (V, C) bf16 = bf16(float32(sum_fp64 of the rows of each token)), ids
    outside [0, V) left out.  The fp64 sums are exact for gradient-sized bf16
    rows (every addend a multiple of 2^-56, |sum| < 0.125), so this is the value
    whatever the order of the rows."""
    ok = (toks >= 0) & (toks < V)
    ref = torch.zeros(V, x.size(1), dtype=torch.float64)
    ref.index_add_(0, toks[ok], x[ok].double())
    return ref.float().to(BF)


def group_case(name, C, V, with_invalid, perm_seed):
    """(x (N, C) bf16, toks (N) int64, S_ref (V, C) bf16): the layout's rows in
    a random order, the invalid ids mixed in with NaN rows"""
    toks = layout_tokens(name)
    x = group_rows(name)[:, :C]
    if with_invalid:
        bad = torch.tensor(invalid_ids(V), dtype=torch.long)
        toks = torch.cat([toks, bad])
        x = torch.cat([x, torch.full((bad.numel(), C), float('nan'), dtype=BF)])
    g = torch.Generator().manual_seed(perm_seed)
    perm = torch.randperm(toks.numel(), generator=g)
    return x[perm].contiguous(), toks[perm].contiguous(), group_ref(name, C, V)


@functools.lru_cache(maxsize=None)
def group_ref(name, C, V):
    return exact_group_sum(group_rows(name)[:, :C], layout_tokens(name), V)


# ---- token sort ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sort_case(V, N, seed=0):
    """ids in [0, V) with repeats (a run of token 0, a run of one wave's first
    token), a tenth of them replaced by ids outside [0, V), and -- from N = 257
    on -- a wave whose first 20 lanes are all invalid"""
    g = torch.Generator().manual_seed(5 + seed + V + N)
    toks = torch.randint(0, V, (N,), generator=g)
    if N >= 257:
        toks[100:140] = 0
        toks[192:230] = toks[192]
    bad = torch.tensor(invalid_ids(V), dtype=torch.long)
    if N >= 10:
        where = torch.randperm(N, generator=g)[:N // 10]
        toks[where] = bad[torch.arange(where.numel()) % bad.numel()]
    if N >= 257:
        toks[64:84] = bad[torch.arange(20) % bad.numel()]
    return toks


def check_sorted(toks, V, stok, srow):
    """the sort's contract over its first n_valid entries (the rest of stok /
    srow is unspecified); numpy arrays"""
    valid = np.flatnonzero((toks >= 0) & (toks < V))
    nv = valid.size
    st, sr = stok[:nv], srow[:nv]
    assert (np.diff(st) >= 0).all(), 'not grouped by token'
    assert np.array_equal(np.sort(sr), valid), 'not a permutation of the valid positions'
    assert np.array_equal(toks[sr], st), 'a row under another token'


# ---- column / row sums -----------------------------------------------------------------

# (V, ldl, NR): a ragged last chunk (V % 8 = 3); a second column block of one
# chunk; two row blocks, the second of 5 rows; 34 partial rows (the reduce
# kernel's unrolled loop and its tail); a ragged chunk next to the following
# partial row's first columns (9 partial rows)
COLSUM_SHAPES = ((1299, 1344, 129), (2056, 2056, 1), (72, 128, 1029), (72, 128, 33 * 1024 + 1),
                 (75, 128, 8 * 1024 + 1))


@functools.lru_cache(maxsize=None)
def colsum_case(V, ldl, NR):
    """(E (NR, ldl) bf16 with NaN pad columns, alpha (NR), db fp64 (V), bound (V))"""
    g = torch.Generator().manual_seed(V + NR)
    E = torch.full((NR, ldl), float('nan'), dtype=BF)
    E[:, :V] = torch.rand(NR, V, generator=g).to(BF)
    alpha = torch.randn(NR, generator=g)
    prod = alpha.double().unsqueeze(1) * E[:, :V].double()
    # fp32 sum of NR rounded products, plus the adds of the partial rows
    bound = (NR + 40) * 2.0 ** -24 * prod.abs().sum(0)
    return E, alpha, prod.sum(0), bound


VGATE_SHAPES = ((3, 3, 5), (3, 2, 11), (1, 4, 1))  # (n, Bv, vdiv)


@functools.lru_cache(maxsize=None)
def vgate_case(n, Bv, vdiv, G4):
    """(dG (n, R, G4 + 24) bf16 with NaN pad columns, ref fp64 (Bv, G4), bound)"""
    g = torch.Generator().manual_seed(n * 100 + Bv * 10 + vdiv + G4)
    R = Bv * vdiv
    dG = torch.full((n, R, G4 + 24), float('nan'), dtype=BF)
    dG[:, :, :G4] = torch.randn(n, R, G4, generator=g).to(BF)
    x = dG[:, :, :G4].double().view(n, Bv, vdiv, G4)
    rows = n * vdiv
    return dG, x.sum((0, 2)), (rows + 8) * 2.0 ** -24 * x.abs().sum((0, 2))
