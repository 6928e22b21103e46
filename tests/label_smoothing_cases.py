"""Shared cases, fp64 references and bounds of the label-smoothing tests
(``--label_smoothing``; ``csrc/kernels/label_smooth.hip`` and the ``ls_eps``
terms of ``vocab_grad.hip``): built once per process on the CPU, never
modified.  ``test_label_smoothing.py`` proves the closed forms, an emulation
in the kernels' arithmetic and the stated bounds against each other without a
GPU; ``test_gpu_label_smoothing.py`` holds the kernels to them.

Row (t, r) of an XE launch carries the gradient ``g`` of its smoothed
log-prob ``(1 - eps) lp[y] + eps mean_v lp[v]``; the dense gradient of the
logits is
    dS = (1 - eps) g onehot(y) + eps g / V - g softmax(x),
and with ``x = Hd W^T + b`` the three gradients of the vocab head are
``dHd = dS W``, ``dW = dS^T Hd``, ``db = sum_r dS_r``.  The kernels never form
dS: the fold writes ``alpha = -g s`` and adds ``(1 - eps) g / alpha`` to the
target's entry of the stored ``E`` (``dS - eps g / V = diag(alpha) E'``), and
the uniform part is rank-1 everywhere:
    dHd_r += eps g_r wbar,   dW_v += gs,   db_v += gs_b,
    wbar = mean_v W_v,  gs = (eps / V) sum_r g_r Hd_r,  gs_b = (eps / V) sum_r g_r.
``mean_v lp[v] = Hd . wbar + bbar - lse`` gives the forward without a dense
pass.

Bounds.  u = 2^-24 is half an ulp of fp32 (one rounding of a value of
magnitude m costs at most u m).  A sum of N fp32 terms accumulated in any
order is off by at most (N - 1) u sum |terms| to first order; the bounds use
N plus a margin for the partial rows' extra adds.
"""
import functools
from types import SimpleNamespace

import torch

import grad_kernel_cases as gc

BF = torch.bfloat16
U = 2.0 ** -24
EPS_VALUES = (0.1, 0.5)


@functools.lru_cache(maxsize=None)
def ls_case(zero_off, H, R=24, n=4, V=203, ldl=256, seed=0):
    """The range-guard case of ``grad_kernel_cases.guard_case`` as an XE launch
    (no sampled-token weights): every third row's vocab input is scaled x60 on
    alternate steps (LSE jumps of about +-100: listed rows, recomputed with
    s = 1), every row kind of ``grad_kernel_cases.KINDS`` among the targets
    (``b_zero`` / ``both_zero`` rows are the masked tokens: g = 0)."""
    g = torch.Generator().manual_seed(501 + 7 * zero_off + H + R + seed)
    wlog = (torch.rand(V, H, generator=g) * 0.2 - 0.1).to(BF)
    blog = torch.randn(V, generator=g) * 0.1
    scale = torch.ones(n, R, 1)
    jump = torch.arange(R) % 3 == 0
    scale[(0 if zero_off else 1)::2, jump] = 60.0
    hd = (torch.randn(n, R, H, generator=g) * scale).to(BF)
    x64 = hd.double() @ wlog.double().t() + blog.double()
    lse = torch.logsumexp(x64, 2).float()
    y_sel, dg_sel, labels, dg_xe, kind = gc._weights(n, R, V, n - 1, g, has_sel=False)
    c = SimpleNamespace(n=n, R=R, V=V, H=H, ldl=ldl, zero_off=zero_off, x64=x64, lse=lse,
                        E=gc.exp_store(x64, lse, zero_off, ldl), y_sel=y_sel, dg_sel=dg_sel,
                        labels=labels, dg_xe=dg_xe, kind=kind, hd=hd.view(n * R, H), wlog=wlog,
                        blog=blog)
    d = lse if zero_off else torch.cat([torch.zeros(1, R), lse[1:] - lse[:-1]], 0)
    c.listed = d.abs() > gc.EXP_SAFE_LSE_JUMP  # (n, R)
    c.exact = torch.exp(x64 - lse.double().unsqueeze(2))  # E of a listed row (own LSE as offset)
    c.g = dg_xe[:, :n].t().contiguous()        # (n, R) fp32: the rows' gradient
    c.y = labels[:, 1:n + 1].t().contiguous()  # (n, R) targets
    assert int((c.g == 0).sum()) > 0 and int(c.listed.sum()) > 0
    assert int((c.listed & (c.g != 0)).sum()) > 0
    return c


# ---- fp64 references ---------------------------------------------------------------

def wbar_ref(wlog, blog):
    """(wbar (H), bbar) fp64 from the bf16 weights / fp32 bias"""
    return wlog.double().mean(0), blog.double().mean()


def wbar_bound(wlog, blog):
    """per column: the fp32 sum of V terms over ragged blocks, then one
    multiply by the fp32 1 / V (2 more roundings)"""
    V = wlog.size(0)
    k = (V + 40) * U / V
    return k * wlog.double().abs().sum(0) + 1e-45, k * blog.double().abs().sum() + 1e-45


def dense_ds(c, eps):
    """(dS, p) fp64 (n, R, V): the smoothed XE gradient of the logits"""
    g = c.g.double()
    p = torch.softmax(c.x64, 2)
    dS = -g.unsqueeze(2) * p + (eps * g / c.V).unsqueeze(2)
    dS.scatter_add_(2, c.y.unsqueeze(2), ((1 - eps) * g).unsqueeze(2))
    return dS, p


def dense_grads(c, eps):
    """(dHd (n R, H), dW (V, H), db (V)) fp64 from the dense dS"""
    dS, _ = dense_ds(c, eps)
    dS = dS.view(-1, c.V)
    return dS @ c.wlog.double(), dS.t() @ c.hd.double(), dS.sum(0)


def smoothed_lp_ref(c, eps):
    """(n, R) fp64: (1 - eps) lp[y] + eps mean_v lp[v] from the dense log-probs"""
    lp = c.x64 - torch.logsumexp(c.x64, 2, keepdim=True)
    return (1 - eps) * lp.gather(2, c.y.unsqueeze(2)).squeeze(2) + eps * lp.mean(2)


def closed_forms(c, eps):
    """The rank-1 closed forms in fp64: (dHd, dW, db, smoothed lp) with the
    non-uniform part dS0 = (1 - eps) g onehot(y) - g p formed densely."""
    g = c.g.double()
    p = torch.softmax(c.x64, 2)
    dS0 = -g.unsqueeze(2) * p
    dS0.scatter_add_(2, c.y.unsqueeze(2), ((1 - eps) * g).unsqueeze(2))
    dS0 = dS0.view(-1, c.V)
    wbar, bbar = wbar_ref(c.wlog, c.blog)
    gf, hd = g.view(-1), c.hd.double()
    gs = (eps / c.V) * (gf.unsqueeze(1) * hd).sum(0)
    gsb = (eps / c.V) * gf.sum()
    dHd = dS0 @ c.wlog.double() + eps * gf.unsqueeze(1) * wbar
    dW = dS0.t() @ hd + gs
    db = dS0.sum(0) + gsb
    lse = torch.logsumexp(c.x64, 2)
    lpy = c.x64.gather(2, c.y.unsqueeze(2)).squeeze(2) - lse
    lp = (1 - eps) * lpy + eps * ((hd @ wbar).view(c.n, c.R) + bbar - lse)
    return dHd, dW, db, lp


def gsum_ref(c, eps):
    """(gs (H), gs_b) fp64 and their bounds: fp32 sums of n R products (each
    product eps g hd: two roundings), then the multiply by the fp32 1 / V"""
    gf, hd = c.g.double().view(-1), c.hd.double()
    terms = (eps / c.V) * gf.unsqueeze(1) * hd
    NR = gf.numel()
    k = (NR + 40) * U
    return (terms.sum(0), (eps / c.V) * gf.sum(),
            k * terms.abs().sum(0) + 1e-45, k * (eps / c.V) * gf.abs().sum() + 1e-45)


def alpha_ref(c, unit_s=None):
    """alpha (n, R) fp64 = -g s: the TOTAL weight, whatever eps"""
    s = torch.exp(gc.store_offsets(c.lse, c.zero_off) - c.lse.double())
    if unit_s is not None:
        s = torch.where(unit_s, torch.ones_like(s), s)
    return -c.g.double() * s


# ---- the kernels' arithmetic in plain torch --------------------------------------------

def f32(x):
    return torch.as_tensor(x, dtype=torch.float32)


def emulate(c, eps, unit_s=None):
    """fp32 emulation of the pieces, in the kernels' operation order where it
    matters: wbar (fp32 sums, one multiply by fp32 1 / V), smoothed lp, alpha,
    the one-hot weight (1 - eps) g, the fold's bf16 update of E, the shift
    coefficient eps g / alpha, gs.  Returns a namespace."""
    V = c.V
    inv_v = f32(1.0 / V)
    wbar = c.wlog.float().sum(0) * inv_v
    bbar = c.blog.sum() * inv_v
    e = f32(eps)
    one_m = f32(1.0) - e
    lse = c.lse
    lpy = (c.x64.gather(2, c.y.unsqueeze(2)).squeeze(2) - lse.double()).float()  # the combine's
    dot = (c.hd.float() * wbar).sum(1).view(c.n, c.R)
    lp = one_m * lpy + e * (dot + bbar - lse)
    off = torch.zeros_like(lse) if c.zero_off else torch.cat([lse[:1], lse[:-1]], 0)
    s = torch.exp(off - lse)
    if unit_s is not None:
        s = torch.where(unit_s, torch.ones_like(s), s)
    al = -(c.g) * s
    b = c.g * one_m
    live = al != 0
    inv = torch.where(live, 1.0 / torch.where(live, al, torch.ones_like(al)), torch.zeros_like(al))
    coef = torch.where(live & (c.g != 0), e * c.g * inv, torch.zeros_like(al))
    gs = ((e * c.g).view(-1, 1) * c.hd.float()).sum(0) * inv_v
    gsb = (e * c.g).sum() * inv_v
    return SimpleNamespace(wbar=wbar, bbar=bbar, lp=lp, alpha=al, b=b, coef=coef, gs=gs, gsb=gsb)


# ---- bounds --------------------------------------------------------------------------------

def lp_bound(c, eps):
    """(n, R) bound on the smoothed log-prob from an exact lp[y]: the fp32 dot
    of H products with the fp32 wbar (H + 8 roundings of sum |hd wbar|, and
    wbar's own error times |hd|), then four fp32 operations on the terms"""
    wb, bb = wbar_bound(c.wlog, c.blog)
    wbar, bbar = wbar_ref(c.wlog, c.blog)
    hd = c.hd.double().abs()
    dot_abs = (hd * wbar.abs()).sum(1).view(c.n, c.R)
    dot_err = (c.H + 8) * U * dot_abs + (hd * wb).sum(1).view(c.n, c.R) + bb
    lse = c.lse.double().abs()
    lpy = (c.x64.gather(2, c.y.unsqueeze(2)).squeeze(2) - torch.logsumexp(c.x64, 2)).abs()
    mags = (1 - eps) * lpy + eps * (dot_abs + bbar.abs() + lse)
    # (+ the fp32 rounding of the saved LSE itself, which lp[y] carries too)
    return eps * dot_err + 8 * U * mags + 2 * U * lse


def fold_bound(c, eps, p):
    """per-element bound (n, R, V) on |alpha E' - (dS - eps g / V)|, as
    ``grad_kernel_cases.fold_bound`` without a sampled-token weight: E rounded
    to bf16 when stored and when folded (2^-8, doubled: 2^-7 of the entry's
    terms), 1e-6 |g| for the fp32 exp / reciprocal / (1 - eps) g."""
    g = c.g.double().abs().unsqueeze(2)
    oh = torch.zeros_like(p)
    oh.scatter_(2, c.y.unsqueeze(2), 1.0)
    return 2.0 ** -7 * ((1 - eps) * g * oh + g * p) + 1e-6 * g


def shift_bound(c, eps, alpha, x_in):
    """per-element bound (n R, H) on |X_out - X_in - (eps g / alpha) wbar|:
    the coefficient (3 roundings), wbar's error, one fma rounding of the sum"""
    wb, _ = wbar_bound(c.wlog, c.blog)
    wbar, _ = wbar_ref(c.wlog, c.blog)
    live = (alpha != 0) & (c.g.double() != 0)
    k = torch.where(live, eps * c.g.double() / torch.where(live, alpha, torch.ones_like(alpha)),
                    torch.zeros_like(alpha)).view(-1, 1).abs()
    return k * (4 * U * wbar.abs() + wb) + 2 * U * (x_in.double().abs() + k * wbar.abs())


def dhd_bound(c, eps, p):
    """per-element bound (n R, H) on the composed dHd = alpha X + b W[y] against
    the dense dS W.  E carries one bf16 rounding (at most 2^-8 relative per
    entry: 2^-8 |g| (p |W|) if every entry erred the same way); every fp32 piece (X = E W: V products; alpha;
    the one-hot row; the shift) stays under 1e-5 of the sum of the magnitudes of
    dHd's terms ((V + 40) u = 1.45e-5 V / 203 ... taken as 2e-5)."""
    g = c.g.double().abs().view(-1, 1)
    Wa = c.wlog.double().abs()
    wbar, _ = wbar_ref(c.wlog, c.blog)
    pW = p.view(-1, c.V) @ Wa
    Wy = Wa[c.y.view(-1)]
    # (a listed row's E is recomputed from fp32 logits: 2^-7, as
    # test_gpu_grad_kernels.py::test_range_guard_rows_recomputed allows)
    rnd = torch.where(c.listed.view(-1, 1), 2.0 ** -7, 2.0 ** -8)
    return rnd * g * pW + 2e-5 * g * (pW + (1 - eps) * Wy + eps * wbar.abs()) + 1e-30


def ratio(err, bound):
    """max err / bound (0 / 0 = 0: an exact zero against a zero bound)"""
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max())


# ---- engine comparison --------------------------------------------------------------------

# (shape of tests/test_gpu_kernels.py::_SHAPES, scale of logit.weight): peaked
# softmax, so that the uniform term is a large share of every gradient
ENGINE_SHAPES = ((dict(V=300, H=64), 30.0), (dict(V=1299, H=512), 12.0))
ENGINE_IDS = ('h64', 'h512')
MIN_SHARE = 0.25
TOL_FLOOR = 0.06
