"""Hand-built cases for ``csrc/kernels/ensemble.hip`` (``ensemble_topk_kernel``)
with their fp64 reference, a numpy fp32 emulation of the kernel's operation
order, and mutations of it that the cases must catch.  Shared by
``tests/test_ensemble.py`` (CPU) and ``tests/test_gpu_ensemble.py``.

A case: ``M`` members, ``R`` rows, ``V`` columns, ``K``; per member fp32 logits
``(R, ldl)`` (``ldl = V`` rounded up to a multiple of 8, here always ``> V``;
the padding columns hold the sentinel ``PAD``), an fp32 ``(R,)`` LSE vector
(hand-made: the kernel only subtracts it) and the fp32 log-weight.  The
reference takes those fp32 inputs as exact and evaluates

    ``e[v] = logsumexp_m(logw_m + z_m[v] - lse_m)``

in fp64; its top-K is ordered by value descending, then index ascending.

The bound on ``|e - e_ref|`` per element
-----------------------------------------
The kernel computes, in fp32 and in this order, ``d_m = z_m - lse_m``, ``a_m =
d_m + logw_m``, ``mx = max_m a_m``, ``t_m = a_m - mx``, ``p_m = expf(t_m)``,
``s = p_0 + p_1 + ..`` (member order), ``l = logf(s)``, ``e = mx + l``.  With
``u = 2^-24`` the unit roundoff of one fp32 operation, ``S`` the largest
magnitude among ``d_m``, ``a_m`` and ``e`` of the case, and 1 ulp <= 2u
relative:

  * ``d_m`` and ``a_m``: one rounding each, ``|delta a_m| <= 2 u S``; ``mx`` is
    one of the ``a_m`` (an exact selection), so ``<= 2 u S`` as well;
  * ``t_m``: its own rounding ``u |t_m|`` plus both inputs' errors: the
    exponent is off by at most ``4 u S + u |t_m|``, which is the relative
    error it causes in ``p_m``;
  * ``expf``: ASSUMED <= 2 ulp, i.e. ``4 u`` relative.  HIP's math-API
    documentation lists the maximum ulp error of ``expf`` and ``logf``; it is
    not installed beside this project's toolchain, so the figure is assumed
    here (the public table gives 1 ulp for ``expf`` and 1-2 ulp for ``logf``;
    2 covers both);
  * in ``s >= 1`` (the maximum's term is ``exp(0) = 1``) term ``m`` weighs
    ``p_m / s <= p_m``, and ``|t_m| p_m <= 1 / e``: the terms' errors move
    ``s`` by at most ``4 u S + 4 u + u M / e`` relative; the ``M - 1``
    additions add ``(M - 1) u``.  A term flushed to zero (``t_m < -87``)
    changes ``s`` by less than ``2^-125``: nothing at this scale;
  * ``l = logf(s)``: a relative error of ``s`` is an absolute error of ``l``;
    ``logf`` itself, ASSUMED <= 2 ulp of ``l <= log 8 < 2.08``: ``8.4 u``;
  * ``e = mx + l``: one rounding, ``u S``.

Sum: ``|e - e_ref| <= u (5 S + M / e + (M - 1) + 4 + 8.4) <= u (5 S + 2 M +
13) = BOUND``.  For ``M = 1`` the kernel's value is the single fp32
subtraction ``z - lse``, and the expected value is that fp32 number exactly
(bound 0).

Separation: every case is built so that the ``K + 1`` largest reference values
of a row differ by more than ``2 * BOUND`` (here by about 0.5), except for
deliberate exact ties: columns that are bit-identical in every member, whose
values are therefore bit-identical in any fixed-order evaluation, so the
smaller index must come first.
"""
import numpy as np

PAD = np.float32(1e30)  # sentinel in columns V..ldl: never a candidate
U = 2.0 ** -24


def _ldl(V):
    return (V + 7) // 8 * 8


def bound(S, M):
    return 0.0 if M == 1 else U * (5.0 * S + 2.0 * M + 13.0)


def reference(logits, lse, logw, V):
    """fp64 mixture values (R, V) of the fp32 inputs; M = 1: the fp32
    difference ``z - lse`` itself."""
    M = len(logits)
    if M == 1:
        return (logits[0][:, :V] - lse[0][:, None]).astype(np.float64)
    a = np.stack([logits[m][:, :V].astype(np.float64) - lse[m].astype(np.float64)[:, None]
                  + np.float64(logw[m]) for m in range(M)])
    mx = a.max(0)
    return mx + np.log(np.exp(a - mx).sum(0))


def topk(e, K, rank=None, larger_index=False):
    """(values (R, K), indices (R, K)) of ``e`` ranked by ``rank`` (default
    ``e``) descending, ties to the smaller index."""
    rank = e if rank is None else rank
    R, n = rank.shape
    idx = np.arange(n)
    out_v, out_i = [], []
    for r in range(R):
        order = np.lexsort((-idx if larger_index else idx, -rank[r]))[:K]
        out_i.append(order)
        out_v.append(e[r, order])
    return np.stack(out_v), np.stack(out_i).astype(np.int64)


def _case(name, M, R, V, K, seed, weights=None, cols=None, dup=(), lse_shift=None, lse_all=None):
    """Random low logits, then ``min(K + 1, V)`` winner columns planted 0.5
    apart (the same columns in every row and member), ``dup = [(rank, col)]``
    bit-identical copies of a winner's column, ``lse_shift[m]`` added to member
    m's LSE, ``lse_all`` replacing every LSE."""
    rng = np.random.RandomState(seed)
    ldl = _ldl(V)
    assert ldl > V
    n_win = min(K + 1, V)
    taken = {c for _, c in dup}
    if cols is None:
        free = [c for c in rng.permutation(V) if c not in taken]
        cols = free[:n_win]
    cols = list(cols)
    assert len(cols) == n_win and len(set(cols) | taken) == n_win + len(taken)
    w = np.full(M, 1.0 / M) if weights is None else np.asarray(weights, np.float64)
    logw = np.log(w / w.sum()).astype(np.float32)
    logits, lse = [], []
    for m in range(M):
        z = rng.uniform(-6.0, -1.0, (R, ldl)).astype(np.float32)
        for j, c in enumerate(cols):
            z[:, c] = np.float32(10.0 + 0.5 * m - 0.5 * j)
        for j, c in dup:
            z[:, c] = z[:, cols[j]]
        z[:, V:] = PAD
        L = rng.uniform(2.0, 9.0, R).astype(np.float32)
        if lse_all is not None:
            L = np.full(R, lse_all, np.float32)
        if lse_shift is not None:
            L = (L + np.float32(lse_shift[m])).astype(np.float32)
        logits.append(z)
        lse.append(L)
    e = reference(logits, lse, logw, V)
    # M = 1: the kernel ranks the raw logits (as beam_topk_kernel), then subtracts
    ref_v, ref_i = topk(e, K, rank=logits[0][:, :V].astype(np.float64) if M == 1 else None)
    S = 0.0
    for m in range(M):
        d = logits[m][:, :V].astype(np.float64) - lse[m].astype(np.float64)[:, None]
        S = max(S, np.abs(d).max(), np.abs(d + np.float64(logw[m])).max())
    S = max(S, np.abs(e).max())
    return dict(name=name, M=M, R=R, V=V, K=K, ldl=ldl, logits=logits, lse=lse, logw=logw,
                e_ref=e, ref_v=ref_v, ref_i=ref_i, bound=bound(S, M), cols=cols, dup=list(dup))


def cases():
    return [
        _case('m1_v37_k5', 1, 3, 37, 5, 1),
        _case('m1_v1031_k16', 1, 1, 1031, 16, 2),
        _case('m2_v259_k9', 2, 7, 259, 9, 3),
        # weights over six decades; the K winners all in thread 3's stride (the
        # lane list holds every winner and hands them to the merge one by one)
        _case('m3_v1031_k5_stride_w1e-6', 3, 3, 1031, 5, 4, weights=[1.0, 1e-3, 1e-6],
              cols=[3, 259, 515, 771, 1027, 600]),
        _case('m8_v1031_k16', 8, 1, 1031, 16, 5, weights=[8, 7, 6, 5, 4, 3, 2, 1]),
        _case('m2_v5_k5_all', 2, 3, 5, 5, 6),                      # K = V, idle threads
        _case('m2_v37_k1', 2, 1, 37, 1, 7, weights=[0.3, 0.7]),
        _case('m8_v5_k1', 8, 7, 5, 1, 8),
        # three winners for a two-entry lane list, all in one thread's stride
        _case('m2_v1031_k2_stride', 2, 3, 1031, 2, 9, cols=[515, 3, 771]),
        # exact tie 256 columns apart (one thread): ranks 0 and 1 are columns 1, 257
        _case('m2_v259_k2_tie256', 2, 3, 259, 2, 10, cols=[257, 40, 90], dup=[(0, 1)]),
        # exact tie across waves, straddling the cut: rank 1 is column 70 (wave
        # 1) and column 5 (wave 0) copies it; K = 2 keeps column 5 only
        _case('m3_v1031_k2_tie_waves', 3, 1, 1031, 2, 11, weights=[0.5, 0.3, 0.2],
              cols=[300, 70, 900], dup=[(1, 5)]),
        # member 1 underflows against member 0: a_1 - mx < -100
        _case('m2_v259_k5_underflow', 2, 3, 259, 5, 12, lse_shift=[0.0, 150.0]),
        # z - lse near +100: expf overflows unless the maximum is subtracted first
        _case('m2_v37_k2_overflow', 2, 1, 37, 2, 13, lse_all=-90.0),
    ]


# -- the kernel's operation order in numpy fp32, and mutations of it -----------------
MUTATIONS = ('no_logw', 'wrong_lse', 'no_max', 'ties_larger', 'reads_padding')


def emulate(case, mutation=None):
    """(top_v (R, K) fp32, top_i (R, K)) as the kernel computes them."""
    f32 = np.float32
    M, V, K = case['M'], case['V'], case['K']
    n = case['ldl'] if mutation == 'reads_padding' else V
    z = [x[:, :n] for x in case['logits']]
    lse = [case['lse'][(m + 1) % M if mutation == 'wrong_lse' else m] for m in range(M)]
    larger = mutation == 'ties_larger'
    if M == 1:
        v, i = topk(z[0], K, larger_index=larger)
        return (v - lse[0][:, None]).astype(f32), i
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        a = []
        for m in range(M):
            d = (z[m] - lse[m][:, None]).astype(f32)
            a.append(d if mutation == 'no_logw' else (d + f32(case['logw'][m])).astype(f32))
        mx = a[0]
        for m in range(1, M):
            mx = np.maximum(mx, a[m])
        if mutation == 'no_max':
            mx = np.zeros_like(mx)
        s = np.zeros_like(mx)
        for m in range(M):
            s = (s + np.exp((a[m] - mx).astype(f32)).astype(f32)).astype(f32)
        e = (mx + np.log(s).astype(f32)).astype(f32)
    return topk(e, K, larger_index=larger)


def check(case, top_v, top_i):
    """None when (top_v, top_i) meets the case, else what is wrong."""
    top_v, top_i = np.asarray(top_v, np.float64), np.asarray(top_i, np.int64)
    if top_v.shape != case['ref_v'].shape or top_i.shape != case['ref_i'].shape:
        return 'shape %r' % (top_v.shape,)
    if (top_i < 0).any() or (top_i >= case['V']).any():
        return 'an index outside [0, V): padding returned'
    if not np.array_equal(top_i, case['ref_i']):
        return 'indices %r, expected %r' % (top_i.tolist(), case['ref_i'].tolist())
    if not np.isfinite(top_v).all():
        return 'non-finite value'
    err = np.abs(top_v - case['ref_v']).max()
    if err > case['bound']:
        return 'value error %.3g > bound %.3g' % (err, case['bound'])
    return None
