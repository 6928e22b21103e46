"""Shared cases, fp64 references, derived bounds and fp32 emulations of the
reverse-recurrence kernel tests (``csrc/kernels/lstm.hip``
``lstm_step_bwd_kernel``, ``csrc/kernels/lstm_loop.hip``, ``csrc/common.h``
``cell_bwd``): built once per process on the CPU, never modified.
``test_lstm_bwd_cases.py`` proves references, bounds and emulations against
each other without a GPU; ``test_gpu_lstm_bwd.py`` holds the kernels to them.

One reverse step t on R rows and H hidden units (packed gate column 4u + g):
    dl   = scale * dh_logit + a W[ys] + b W[yx]          (token -1: no term)
    dh   = dG_{t+1} . whhT^T + keep(seed, t, r, u) * dl / (1 - p)
    dG_t, carry' = cell_bwd(dh, carry, saved slots, c_t, c_{t-1})
with dG_t stored as bf16 and the carry kept in fp32.

The bound is derived, not tuned: absolute errors are pushed through the same
formulas (multilinear in dh and the carry once the saved activations are
fixed).  Constants: U = 2^-24 per fp32 rounding; the GEMM's fp32 accumulation
(KD + 8) U sum |dG_{t+1}| |whhT|; EPS_T = 2^-21 absolute on the fast tanh
(exp, one reciprocal -- 1 ulp each -- and three roundings of values <= 1; for
|c| <= 8 the exp's argument scaling adds < 2^-24), hence 2 |tc| EPS_T + 4 U on
1 - tc^2; 4 U per product of up to four fp32 factors; BF_EPS = 2^-8 relative
for the bf16 store (round to nearest even, 8 significant bits: half an ulp of
2^-7).
"""
import functools
from types import SimpleNamespace

import torch

BF = torch.bfloat16
M32 = 0xFFFFFFFF
LSTM, GRU, RNN = 0, 1, 2
CELLS = (LSTM, GRU, RNN)
CELL_NAMES = {LSTM: 'lstm', GRU: 'gru', RNN: 'rnn'}
U = 2.0 ** -24
EPS_T = 2.0 ** -21
BF_EPS = 2.0 ** -8
SEED = 13579          # RNG word 0 (dropout); word 1 belongs to the sampler
OH_V = 50             # rows of the one-hot logit weights
OH_BIG = 32768.0      # row 0 of them: what a term gathered from the clamped row would add

MUTATIONS = ('cprev_is_ct', 'mask_from_other_step', 'mask_row_shifted', 'no_keep_scale',
             'carry_times_i', 'gate_slots_swapped', 'stale_dg_next', 'one_row_from_neighbour',
             'gru_nh_as_n', 'onehot_term_missing', 'scale_ignored')


def mutations_of(cell):
    """the mutations that change what this cell computes"""
    out = []
    for m in MUTATIONS:
        if m == 'gru_nh_as_n' and cell != GRU:
            continue
        if m == 'cprev_is_ct' and cell == RNN:     # the tanh RNN reads no previous state
            continue
        if m == 'carry_times_i' and cell == RNN:   # ... and carries nothing
            continue
        out.append(m)
    return out


# ---- the dropout keep-mask (common.h dropout_keep) ------------------------------

def _mul32(h, c):
    """(h * c) mod 2^32 for int64 tensors holding uint32 values."""
    lo, hi = h & 0xFFFF, h >> 16
    return (lo * c + (((hi * c) & 0xFFFF) << 16)) & M32


def _mix32(h):
    h = h ^ (h >> 16)
    h = _mul32(h, 0x85EBCA6B)
    h = h ^ (h >> 13)
    h = _mul32(h, 0xC2B2AE35)
    return h ^ (h >> 16)


def keep_mask(seed, step, R, H, p, device='cpu'):
    """(R, H) bool keep-mask of csrc/common.h dropout_keep(seed, step, r, u, p)."""
    r = torch.arange(R, device=device, dtype=torch.int64)[:, None]
    u = torch.arange(H, device=device, dtype=torch.int64)[None, :]
    h1 = _mix32((seed ^ ((step * 0x9E3779B1) & M32)) ^ _mul32(r, 0x7FEB352D))
    h = _mix32(h1 ^ _mul32(u, 0x846CA68B))
    u01 = ((h >> 8) + 1).float() * (1.0 / 16777216.0)
    return u01 > p


def bits(t):
    """bf16 tensor -> its 16-bit patterns (int16), for bit comparisons"""
    assert t.dtype == BF
    return t.contiguous().view(torch.int16)


# ---- case builders --------------------------------------------------------------

def _saved(cell, shape, g):
    """saved activations (..., H, 4) as valid bf16 values of the cell"""
    x = torch.randn(*shape, 4, generator=g) * 1.5
    if cell == LSTM:      # (i, f, g, o)
        s = torch.sigmoid(x)
        s[..., 2] = torch.tanh(x[..., 2])
    elif cell == GRU:     # (r, z, n, n_h)
        s = torch.sigmoid(x)
        s[..., 2] = torch.tanh(x[..., 2])
        s[..., 3] = x[..., 3]
    else:                 # (h, -)
        s = torch.zeros_like(x)
        s[..., 0] = torch.tanh(x[..., 0])
    return s.to(BF)


def _states(shape, g):
    """|c| <= 8; every 7th unit in [4, 8] so that tanh(c) saturates"""
    c = (torch.randn(*shape, generator=g) * 1.5).clamp(-3.5, 3.5)
    sat = (4.0 + 4.0 * torch.rand(*shape, generator=g)) * torch.sign(c)
    sat[..., 0] = 8.0 * torch.sign(c[..., 0]) + (c[..., 0] == 0)  # the end of the range itself
    c[..., ::7] = sat[..., ::7]
    return c.clamp(-8.0, 8.0)


def _onehot(shape, H, g, kind='both'):
    """one-hot operands over rows of `shape`: weights fp32, tokens int32 with
    -1 (weight 0) on every 5th row; row 0 of W large and finite.  kind: 'both',
    'a', 'b' (the other absent) or 'same' (ys == yx)."""
    W = (torch.randn(OH_V, H, generator=g) * 0.05).to(BF)
    W[0] = OH_BIG
    n = 1
    for d in shape:
        n *= d
    oh = SimpleNamespace(W=W, a=None, ys=None, b=None, yx=None)
    for i, (wn, tn) in enumerate((('a', 'ys'), ('b', 'yx'))):
        if kind in ('both', 'same') or kind == wn:
            w = torch.randn(n, generator=g) * 0.1
            tok = torch.randint(1, OH_V, (n,), generator=g, dtype=torch.int64).to(torch.int32)
            none = torch.arange(n) % 5 == 1 + i
            w[none] = 0.0
            tok[none] = -1
            setattr(oh, wn, w.view(*shape))
            setattr(oh, tn, tok.view(*shape))
    if kind == 'same':
        oh.yx = oh.ys.clone()
        oh.b = torch.where(oh.ys < 0, torch.zeros_like(oh.b), oh.b)
    return oh


@functools.lru_cache(maxsize=None)
def step_case(cell, R, H, KD=None, drop_p=0.5, step=7, has_next=True, has_cprev=True,
              has_scale=False, onehot=None, seed=0):
    """operands of one reverse step (see lstm_step_bwd_test)"""
    KD = 4 * H if KD is None else KD
    g = torch.Generator().manual_seed(7919 * seed + 1000 * cell + 31 * R + H + KD + step % 97)
    c = SimpleNamespace(cell=cell, R=R, H=H, KD=KD, p=drop_p, step=step, seed=SEED)
    c.whhT = (torch.randn(H, KD, generator=g) / H ** 0.5).to(BF)
    c.dg_next = (torch.randn(R, KD, generator=g) * 0.01).to(BF) if has_next else None
    c.dh_logit = torch.randn(R, H, generator=g) * 0.01
    c.dc_carry = torch.randn(R, H, generator=g) * 0.01
    c.gates = _saved(cell, (R, H), g).view(R, 4 * H)
    c.c_t = _states((R, H), g)
    c.c_prev = _states((R, H), g) if has_cprev else None
    c.scale = torch.randn(R, generator=g) if has_scale else None
    c.oh = _onehot((R,), H, g, onehot) if onehot else None
    return c


@functools.lru_cache(maxsize=None)
def chain_case(cell, R, H, T, drop_p=0.5, fold=False, seed=0):
    """operands of the whole reverse loop (see lstm_bwd_loop_test); fold: row
    scales and both one-hot terms"""
    g = torch.Generator().manual_seed(104729 * seed + 1000 * cell + 31 * R + H + 7 * T + fold)
    c = SimpleNamespace(cell=cell, R=R, H=H, T=T, KD=4 * H, p=drop_p, seed=SEED, case_seed=seed)
    c.whhT = (torch.randn(H, 4 * H, generator=g) / H ** 0.5).to(BF)
    c.dh = torch.randn(T, R, H, generator=g) * 0.01
    c.gates = _saved(cell, (T, R, H), g).view(T, R, 4 * H)
    c.c_all = _states((T, R, H), g)
    c.scale = torch.randn(T, R, generator=g) if fold else None
    c.oh = _onehot((T, R), H, g, 'both') if fold else None
    return c


def chain_step(c, t, dg_next, carry):
    """step t of a chain case as a step case, on the given dG_{t+1} (bf16 or
    None) and carry (fp32)"""
    s = SimpleNamespace(cell=c.cell, R=c.R, H=c.H, KD=c.KD, p=c.p, step=t, seed=c.seed)
    s.whhT, s.dg_next, s.dc_carry = c.whhT, dg_next, carry
    s.dh_logit, s.gates, s.c_t = c.dh[t], c.gates[t], c.c_all[t]
    s.c_prev = c.c_all[t - 1] if t > 0 else None
    s.scale = c.scale[t] if c.scale is not None else None
    s.oh = None
    if c.oh is not None:
        s.oh = SimpleNamespace(W=c.oh.W, a=c.oh.a[t], ys=c.oh.ys[t], b=c.oh.b[t], yx=c.oh.yx[t])
    return s


# ---- fp64 reference and bound ---------------------------------------------------

def fold_ref(dh_logit, scale, oh):
    """(dl, sum of the magnitudes of its terms), fp64: scale dh + a W[ys] + b W[yx]"""
    x = dh_logit.double()
    if scale is not None:
        x = x * scale.double().unsqueeze(-1)
    mag = x.abs()
    if oh is not None:
        W = oh.W.double()
        for w, y in ((oh.a, oh.ys), (oh.b, oh.yx)):
            if w is None:
                continue
            term = w.double().unsqueeze(-1) * W[y.clamp(min=0).long()]
            term = torch.where((y >= 0).unsqueeze(-1), term, torch.zeros_like(term))
            x = x + term
            mag = mag + term.abs()
    return x, mag


def _mul(x, Ex, coef, Ecoef):
    """x * coef with coef a product of at most four fp32 factors whose
    non-product parts carry the absolute error Ecoef: (value, error)"""
    return x * coef, Ex * coef.abs() + (x.abs() + Ex) * (Ecoef + 4 * U * coef.abs())


def _cell_ref(cell, dh, E_dh, carry, E_carry, s, ct, cp):
    """cell_bwd in fp64 with its error: (d (R, H, 4) before the bf16 store, its
    error, carry', its error)"""
    s0, s1, s2, s3 = (s[..., k] for k in range(4))
    zero = torch.zeros_like(dh)
    if cell == LSTM:
        tc = torch.tanh(ct)
        om = 1.0 - tc * tc
        E_om = 2 * tc.abs() * EPS_T + 4 * U
        A, E_A = _mul(dh, E_dh, s3 * om, s3.abs() * E_om)
        dc = carry + A
        E_dc = E_carry + E_A + U * (dc.abs() + E_carry + E_A)
        d0 = _mul(dc, E_dc, s2 * s0 * (1 - s0), 2 * U)
        d1 = _mul(dc, E_dc, cp * s1 * (1 - s1), 2 * U * cp.abs().clamp(min=1.0))
        d2 = _mul(dc, E_dc, s0 * (1 - s2 * s2), 2 * U)
        d3 = _mul(dh, E_dh, tc * s3 * (1 - s3), EPS_T * (s3 * (1 - s3)).abs() + 2 * U)
        cy = _mul(dc, E_dc, s1, zero)
    elif cell == GRU:
        r, z, n, nh = s0, s1, s2, s3
        d = dh + carry
        E_d = E_dh + E_carry + U * (d.abs() + E_dh + E_carry)
        d1 = _mul(d, E_d, (cp - n) * z * (1 - z), 2 * U * (cp.abs() + 1.0))
        da2, E_da2 = _mul(d, E_d, (1 - z) * (1 - n * n), 3 * U)
        d2 = (da2, E_da2)
        d3 = _mul(da2, E_da2, r, zero)
        d0 = _mul(da2, E_da2, nh * r * (1 - r), U * nh.abs())
        cy = _mul(d, E_d, z, zero)
    else:
        d = dh + carry
        E_d = E_dh + E_carry + U * (d.abs() + E_dh + E_carry)
        d0 = _mul(d, E_d, 1 - s0 * s0, 2 * U)
        d1 = d2 = d3 = cy = (zero, zero)
    dd = torch.stack([d0[0], d1[0], d2[0], d3[0]], -1)
    Ed = torch.stack([d0[1], d1[1], d2[1], d3[1]], -1)
    return dd, Ed, cy[0], cy[1]


def _step(c, dg, E_dg, carry, E_carry):
    """one step in fp64 on dG_{t+1} = dg (fp64 or None) known to E_dg and the
    carry known to E_carry: (dG (R, KD' = 4H) unrounded, its bound with the
    bf16 store, carry', its bound)"""
    R, H = c.R, c.H
    w = c.whhT.double()
    dl, dl_mag = fold_ref(c.dh_logit, c.scale, c.oh)
    inv = 1.0 / (1.0 - c.p) if c.p > 0 else 1.0
    keep = keep_mask(c.seed, c.step, R, H, c.p).double() if c.p > 0 else torch.ones(R, H, dtype=torch.float64)
    if dg is None:
        rec = E_rec = torch.zeros(R, H, dtype=torch.float64)
    else:
        aw = w.abs().t()
        rec = dg @ w.t()
        E_rec = E_dg @ aw + (w.size(1) + 8) * U * ((dg.abs() + E_dg) @ aw)
    dh = rec + keep * dl * inv
    E_dh = E_rec + 6 * U * keep * dl_mag * inv + U * dh.abs()
    s = c.gates.double().view(R, H, 4)
    cp = c.c_prev.double() if c.c_prev is not None else torch.zeros(R, H, dtype=torch.float64)
    d, E_d, cy, E_cy = _cell_ref(c.cell, dh, E_dh, carry, E_carry, s, c.c_t.double(), cp)
    E_d = E_d + BF_EPS * (d.abs() + E_d)
    return d.reshape(R, 4 * H), E_d.reshape(R, 4 * H), cy, E_cy


def _z(c, n):
    return torch.zeros(c.R, n, dtype=torch.float64)


def step_ref(c):
    """(dG (R, 4H), carry') in fp64 from the case's bf16 / fp32 operands"""
    dg = c.dg_next.double() if c.dg_next is not None else None
    d, _, cy, _ = _step(c, dg, _z(c, c.KD), c.dc_carry.double(), _z(c, c.H))
    return d, cy


def step_bound(c, E_dg_next=None, E_carry=None):
    """per-element bounds (dG (R, 4H) as stored, carry') for inputs known to
    E_dg_next (R, KD) / E_carry (R, H) (None: exact)"""
    dg = c.dg_next.double() if c.dg_next is not None else None
    _, E_d, _, E_cy = _step(c, dg, _z(c, c.KD) if E_dg_next is None else E_dg_next,
                            c.dc_carry.double(), _z(c, c.H) if E_carry is None else E_carry)
    return E_d, E_cy


@functools.lru_cache(maxsize=None)
def _chain(cell, R, H, T, drop_p, fold, seed):
    c = chain_case(cell, R, H, T, drop_p, fold, seed)
    dG, EG = [None] * T, [None] * T
    dg, E_dg = None, _z(c, c.KD)
    cy, E_cy = _z(c, H), _z(c, H)
    for t in range(T - 1, -1, -1):
        s = chain_step(c, t, None, None)
        dg, E_dg, cy, E_cy = _step(s, dg, E_dg, cy, E_cy)
        dG[t], EG[t] = dg, E_dg
    return torch.stack(dG), torch.stack(EG), cy, E_cy


def _key(c):
    return (c.cell, c.R, c.H, c.T, c.p, c.scale is not None, c.case_seed)


def chain_ref(c):
    """(dG (T, R, 4H) with dG_t kept unrounded along the chain, dc_out (R, H)), fp64"""
    dG, _, cy, _ = _chain(*_key(c))
    return dG, cy


def chain_bound(c):
    """step_bound applied from t = T - 1 down, each step's bound fed to the
    next as E_dg_next / E_carry: (bound of dG (T, R, 4H), bound of dc_out)"""
    _, EG, _, E_cy = _chain(*_key(c))
    return EG, E_cy


# ---- fp32 emulation of the kernels' arithmetic ----------------------------------

def tanh_fast32(x):
    """common.h tanhf_ in fp32: one exp, one reciprocal"""
    e = torch.exp(-2.0 * x.abs())
    return torch.copysign((1.0 - e) * (1.0 / (1.0 + e)), x)


def _fold32(dh_logit, scale, oh, mutation=None):
    x = dh_logit.float()
    if scale is not None and mutation != 'scale_ignored':
        x = x * scale.float().unsqueeze(-1)
    if oh is not None:
        W = oh.W.float()
        terms = [(oh.a, oh.ys), (oh.b, oh.yx)]
        if mutation == 'onehot_term_missing':
            terms = terms[:1] if oh.a is not None and oh.b is not None else []
        for w, y in terms:
            if w is not None:
                x = x + w.float().unsqueeze(-1) * W[y.clamp(min=0).long()]
    return x


def _emulate(c, dg, carry, mutation=None):
    """one step as the kernels compute it (fp32, fast tanh, bf16 dG):
    (dG (R, 4H) bf16, carry' fp32); dg: bf16 (R, KD) or None"""
    R, H, cell = c.R, c.H, c.cell
    dl = _fold32(c.dh_logit, c.scale, c.oh, mutation)
    inv = 1.0 / (1.0 - c.p) if c.p > 0 and mutation != 'no_keep_scale' else 1.0
    if c.p > 0:
        keep = keep_mask(c.seed, c.step + (1 if mutation == 'mask_from_other_step' else 0), R, H, c.p)
        if mutation == 'mask_row_shifted':
            keep = torch.roll(keep, 1, 0)
    else:
        keep = torch.ones(R, H, dtype=torch.bool)
    dh = torch.zeros(R, H)
    if dg is not None:
        dh = dg.float() @ c.whhT.float().t()
        if mutation == 'one_row_from_neighbour' and R > 1:
            dh[R - 1] = dh[R - 2]
    dh = dh + torch.where(keep, dl * inv, torch.zeros_like(dl))
    s = c.gates.float().view(R, H, 4)
    s0, s1, s2, s3 = (s[..., k] for k in range(4))
    if mutation == 'gate_slots_swapped':
        s0, s1 = s1, s0
    ct = c.c_t.float()
    cp = c.c_prev.float() if c.c_prev is not None else torch.zeros(R, H)
    if mutation == 'cprev_is_ct':
        cp = ct
    zero = torch.zeros(R, H)
    if cell == LSTM:
        tc = tanh_fast32(ct)
        dc = carry + dh * s3 * (1.0 - tc * tc)
        d = [dc * s2 * s0 * (1.0 - s0), dc * cp * s1 * (1.0 - s1), dc * s0 * (1.0 - s2 * s2),
             dh * tc * s3 * (1.0 - s3)]
        cy = dc * (s0 if mutation == 'carry_times_i' else s1)
    elif cell == GRU:
        r, z, n, nh = s0, s1, s2, (s2 if mutation == 'gru_nh_as_n' else s3)
        dd = dh + carry
        dz = dd * (cp - n)
        da2 = dd * (1.0 - z) * (1.0 - n * n)
        dr = da2 * nh
        d = [dr * r * (1.0 - r), dz * z * (1.0 - z), da2, da2 * r]
        cy = dd * (r if mutation == 'carry_times_i' else z)
    else:
        dd = dh + carry
        d = [dd * (1.0 - s0 * s0), zero, zero, zero]
        cy = zero
    return torch.stack(d, -1).reshape(R, 4 * H).to(BF), cy


def step_emulate(c, mutation=None):
    """(dG (R, 4H) bf16, carry') of one step in the kernel's arithmetic"""
    return _emulate(c, c.dg_next, c.dc_carry.float(), mutation)


def chain_emulate(c, mutation=None):
    """(dG (T, R, 4H) bf16, dc_out) of the loop in the kernels' arithmetic"""
    dG = [None] * c.T
    cy = torch.zeros(c.R, c.H)
    for t in range(c.T - 1, -1, -1):
        tn = t + 2 if mutation == 'stale_dg_next' else t + 1
        dg = dG[tn] if tn < c.T else None
        dG[t], cy = _emulate(chain_step(c, t, None, None), dg, cy, mutation)
    return torch.stack(dG), cy


def ratio(got, ref, bound):
    """max |got - ref| / bound (0 / 0 = 0, x / 0 = inf)"""
    err = (got.double() - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(q.max()) if q.numel() else 0.0


# ---- attention epilogue ---------------------------------------------------------

def att_epi_ok(vdiv, C, H):
    """lstm.hip att_bwd_epi_ok"""
    CP = 8 if C <= 8 else 16
    nv = (62 + vdiv) // vdiv + 1
    return (C <= 16 and vdiv >= 2 and H % 64 == 0 and nv * 64 * 4 * CP * 2 <= 5 * 512 * 16 and
            2 * 64 * 72 * 4 + nv * 64 * 4 * CP * 2 <= 2 * 3 * 16384)


def smallest_vdiv(C, H):
    return next(v for v in range(2, 65) if att_epi_ok(v, C, H))


@functools.lru_cache(maxsize=None)
def gate_table(R, H, vdiv, C, seed=0):
    """gvb16 (Bv, H, CP, 4) bf16, pad frames C..CP zero"""
    g = torch.Generator().manual_seed(15485863 * seed + 31 * R + H + 1000 * vdiv + C)
    CP = 8 if C <= 8 else 16
    gv = torch.zeros((R + vdiv - 1) // vdiv, H, CP, 4)
    gv[:, :, :C] = torch.randn(gv.size(0), H, C, 4, generator=g)
    return gv.to(BF)


def _dal_products(dG, gvb16, vdiv):
    R = dG.size(0)
    Bv, H, CP, _ = gvb16.shape
    d = dG[:, :4 * H].double().view(R, H, 1, 4)
    gv = gvb16.double()[torch.arange(R) // vdiv]            # (R, H, CP, 4)
    return (d * gv).view(R, H // 64, 64, CP, 4)


def dal_ref(dG, gvb16, vdiv):
    """dal_part (H / 64, R, CP): over the tile's 64 units and 4 gates, the fp64
    sum of dG[r][4u + g] as stored (bf16) times gvb16[video(r)][u][c][g]"""
    return _dal_products(dG, gvb16, vdiv).sum((2, 4)).permute(1, 0, 2).contiguous()


def dal_bound(dG, gvb16, vdiv):
    """(256 + 8) U sum |.| over the same products"""
    mag = _dal_products(dG, gvb16, vdiv).abs().sum((2, 4)).permute(1, 0, 2).contiguous()
    return (256 + 8) * U * mag
