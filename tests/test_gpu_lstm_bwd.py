"""The backward's reverse-recurrence kernels one by one (``lstm.hip``
``lstm_step_bwd_kernel``; ``lstm_loop.hip`` ``lstm_bwd_loop_kernel``,
``lstm_bwd_ksplit_kernel`` and ``lstm_bwd_fold_kernel``; ``common.h``
``cell_bwd``) through the test entries ``lstm_step_bwd_test`` /
``lstm_bwd_loop_test``, against the fp64 references of ``lstm_bwd_cases.py``:
per-element derived bounds, bit equality where the kernel owes it.  Shapes sit
on the kernels' edges: ragged last row tiles, groups and row blocks, tile
counts that are no multiple of 8, both K-group instantiations, tail columns,
both parities of the loop's c rotation.

Out of scope here: the fused attention workgroups (``AttBwdEpi::flags``) and
``attention.hip``'s backward kernels; only the non-fused attention epilogue of
the step kernel (``dal_part``) is checked.  No test forces a poll timeout
(``test_gpu_bwd_loop.py`` does)."""
from types import SimpleNamespace

import pytest
import torch

import lstm_bwd_cases as lc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF = torch.bfloat16
SENTINEL = 0x7FC1  # a bf16 NaN pattern no kernel produces
CELLS = pytest.mark.parametrize('cell', lc.CELLS, ids=[lc.CELL_NAMES[c] for c in lc.CELLS])


def _ops():
    from cst_captioning_amd import _ext
    assert _ext.available(), 'native extension must be built for GPU tests'
    return _ext.ops()


def _dev(t):
    return None if t is None else t.to(DEV)


def _rng(c):
    return torch.tensor([c.seed, 2468], dtype=torch.int32, device=DEV)


def _oh(oh):
    if oh is None:
        return {}
    return {'oh_W': _dev(oh.W), 'oh_a': _dev(oh.a), 'oh_ys': _dev(oh.ys), 'oh_b': _dev(oh.b),
            'oh_yx': _dev(oh.yx)}


def _run_step(c, gvb16=None, vdiv=1, C=0):
    """lstm_step_bwd_test on a step case: [dG (R, KD) bf16, carry', dal_part] on the CPU"""
    def e(dt):
        return torch.empty(0, dtype=dt, device=DEV)
    out = _ops().lstm_step_bwd_test(
        _dev(c.dg_next) if c.dg_next is not None else e(BF), _dev(c.whhT), _dev(c.dh_logit),
        _dev(c.dc_carry), _dev(c.gates), _dev(c.c_t),
        _dev(c.c_prev) if c.c_prev is not None else e(torch.float32), c.p, _rng(c), c.step, c.cell,
        c.KD, SENTINEL, dh_scale=_dev(c.scale), gvb16=_dev(gvb16), vdiv=vdiv, C=C, **_oh(c.oh))
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def _check_step(c, out, tag):
    """dG within step_bound (exact inputs), the carry within its fp32 bound,
    the tail columns untouched"""
    dG, cy = out[0], out[1]
    H4 = 4 * c.H
    assert dG.shape == (c.R, c.KD) and dG.dtype == BF and cy.shape == (c.R, c.H)
    ref_d, ref_cy = lc.step_ref(c)
    E_d, E_cy = lc.step_bound(c)
    assert not bool(torch.isnan(dG[:, :H4].float()).any()), tag + ': dG columns not written'
    rd, rc = lc.ratio(dG[:, :H4], ref_d, E_d), lc.ratio(cy, ref_cy, E_cy)
    print('%s: dG err/bound %.3f carry err/bound %.3f' % (tag, rd, rc))
    assert rd <= 1.0, tag
    assert rc <= 1.0, tag
    if c.KD > H4:
        tail = lc.bits(dG)[:, H4:]
        want = torch.tensor(SENTINEL, dtype=torch.int32).to(torch.int16)
        assert bool((tail == want).all()), tag + ': tail columns written'


def _tag(c, extra=''):
    return '%s R=%d H=%d KD=%d p=%g step=%d %s' % (lc.CELL_NAMES[c.cell], c.R, c.H, c.KD, c.p,
                                                  c.step, extra)


STEP_SHAPES = [(R, H, 4 * H) for H in (64, 128) for R in (1, 63, 64, 65, 130)] + \
    [(130, 192, 768),   # 9 tiles: no multiple of 8 (the XCD remap's ragged part)
     (65, 64, 320),     # 5 K-tiles: the one-group instantiation, tail columns
     (65, 128, 640)]    # two groups with tail columns


@pytest.mark.parametrize('R,H,KD', STEP_SHAPES)
def test_step_matches_fp64_per_element(R, H, KD):
    for cell in lc.CELLS:
        for p in (0.0, 0.5):
            c = lc.step_case(cell, R, H, KD, p)
            _check_step(c, _run_step(c), _tag(c))


VARIANTS = {
    'no_dg_next': {'has_next': False},
    'no_c_prev': {'has_cprev': False},
    'dh_scale': {'has_scale': True},
    'onehot_both': {'has_scale': True, 'onehot': 'both'},
    'onehot_same_token': {'onehot': 'same'},
    'onehot_a_only': {'onehot': 'a'},
    'onehot_b_only': {'onehot': 'b'},
    'step_0': {'step': 0},
    'step_65539': {'step': 65539},
}


@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_step_variants(variant):
    for cell in lc.CELLS:
        for R, H, KD in ((65, 128, 512), (65, 64, 320)):
            c = lc.step_case(cell, R, H, KD, 0.5, **VARIANTS[variant])
            _check_step(c, _run_step(c), _tag(c, variant))


def test_step_keep_mask_bit_exact():
    """whhT = 0 and a zero carry: dG is exactly zero where keep_mask drops and
    non-zero in all four gate columns where it keeps"""
    R, H = 65, 128
    base = lc.step_case(lc.LSTM, R, H)
    for step in (0, 7, 65539):
        c = SimpleNamespace(**vars(base))
        c.step, c.dc_carry = step, torch.zeros(R, H)
        c.whhT = torch.zeros_like(base.whhT)
        c.dh_logit = torch.sign(base.dh_logit) * (base.dh_logit.abs() + 0.01)
        c.gates = torch.full((R, 4 * H), 0.5, dtype=BF)
        c.c_t, c.c_prev, c.scale, c.oh = torch.full((R, H), 0.5), torch.ones(R, H), None, None
        dG = _run_step(c)[0].float().view(R, H, 4)
        keep = lc.keep_mask(c.seed, step, R, H, 0.5)
        assert 0 < int(keep.sum()) < R * H
        assert bool((dG[~keep] == 0).all()), 'a dropped element received gradient'
        assert bool((dG[keep] != 0).all()), 'a kept element received none'


def test_step_one_minus_tanh_squared():
    """i = f = o = 1, dh = 1, no GEMM, no dropout: the returned carry is the
    kernel's 1 - tanh(c)^2 in fp32"""
    R, H = 65, 64
    base = lc.step_case(lc.LSTM, R, H, drop_p=0.0, has_next=False)
    c = SimpleNamespace(**vars(base))
    c.dc_carry = torch.zeros(R, H)
    grid = torch.linspace(-8.0, 8.0, R * H)
    grid[R * H // 2] = 0.0
    assert float(grid[0]) == -8.0 and float(grid[-1]) == 8.0
    c.c_t, c.c_prev = grid.view(R, H).contiguous(), torch.zeros(R, H)
    c.gates = torch.ones(R, 4 * H, dtype=BF)
    c.dh_logit, c.scale, c.oh = torch.ones(R, H), None, None
    cy = _run_step(c)[1].double()
    tc = torch.tanh(c.c_t.double())
    err = (cy - (1.0 - tc * tc)).abs()
    bound = 2 * tc.abs() * lc.EPS_T + 4 * lc.U
    print('1 - tanh^2: max err/bound %.3f' % float((err / bound).max()))
    assert bool((err <= bound).all())


@pytest.mark.parametrize('vdiv,C', [(lc.smallest_vdiv(8, 128), 8), (lc.smallest_vdiv(12, 128), 12),
                                    (20, 8), (20, 12)])
def test_step_attention_epilogue(vdiv, C):
    """the non-fused attention epilogue: dal_part from the dG the launch stored"""
    R, H = 130, 128
    CP = 8 if C <= 8 else 16
    gv = lc.gate_table(R, H, vdiv, C)
    assert bool((gv[:, :, C:] == 0).all())
    for cell in lc.CELLS:
        c = lc.step_case(cell, R, H, 4 * H, 0.5)
        out = _run_step(c, gv, vdiv, C)
        _check_step(c, out, _tag(c, 'att vdiv=%d C=%d' % (vdiv, C)))
        dal = out[2]
        assert dal.shape == (H // 64, R, CP)
        assert not bool(torch.isnan(dal).any()), 'dal_part not written everywhere'
        ref, bound = lc.dal_ref(out[0], gv, vdiv), lc.dal_bound(out[0], gv, vdiv)
        r = lc.ratio(dal, ref, bound)
        print('%s vdiv=%d C=%d: dal_part err/bound %.3f' % (lc.CELL_NAMES[cell], vdiv, C, r))
        assert r <= 1.0
        assert bool((dal[:, :, C:] == 0).all())


def test_step_entry_refuses_unsupported_attention_shape():
    c = lc.step_case(lc.LSTM, 130, 128)
    vdiv = lc.smallest_vdiv(8, 128) - 1
    with pytest.raises(RuntimeError):
        _run_step(c, lc.gate_table(130, 128, vdiv, 8), vdiv, 8)


# ---- the persistent loop --------------------------------------------------------

FORMS = {1: 'rowread', 0: 'ksplit'}


def _run_loop(c, form):
    """lstm_bwd_loop_test on a chain case, the error word 0 before and after:
    [dG (T, R, 4H) bf16, dc_out, dh as folded] on the CPU"""
    ops = _ops()
    ops.reset_device_errors(0)
    assert ops.device_errors(0) == 0
    out = ops.lstm_bwd_loop_test(_dev(c.whhT), _dev(c.dh), _dev(c.gates), _dev(c.c_all), c.p,
                                 _rng(c), c.cell, form, scale=_dev(c.scale), **_oh(c.oh))
    torch.cuda.synchronize()
    assert ops.device_errors(0) == 0, 'a team wait ran out of polls'
    return [o.cpu() for o in out]


def _check_chain(c, dG, dc, tag):
    """every step's dG and dc_out within chain_bound of chain_ref"""
    ref, ref_cy = lc.chain_ref(c)
    E, E_cy = lc.chain_bound(c)
    assert dG.shape == (c.T, c.R, 4 * c.H) and dG.dtype == BF and dc.shape == (c.R, c.H)
    assert not bool(torch.isnan(dG.float()).any()), tag + ': dG not written everywhere'
    assert not bool(torch.isnan(dc).any()), tag + ': dc_out not written everywhere'
    per_step = [lc.ratio(dG[t], ref[t], E[t]) for t in range(c.T)]
    rc = lc.ratio(dc, ref_cy, E_cy)
    print('%s: chain err/bound per step %s dc_out %.3f' % (tag, ['%.3f' % x for x in per_step], rc))
    assert max(per_step) <= 1.0, tag
    assert rc <= 1.0, tag


def _check_self_consistent(c, dG, tag):
    """from the loop's own stored dG_{t+1}: the carry-free outputs of step t
    (LSTM: the d3 column; RNN: all of dG) within the single-step bound"""
    if c.cell == lc.GRU:
        return
    worst = 0.0
    for t in range(c.T - 1):
        s = lc.chain_step(c, t, dG[t + 1], torch.zeros(c.R, c.H))
        ref, _ = lc.step_ref(s)
        E, _ = lc.step_bound(s)
        sel = slice(3, None, 4) if c.cell == lc.LSTM else slice(None)
        worst = max(worst, lc.ratio(dG[t][:, sel], ref[:, sel], E[:, sel]))
    print('%s: self-consistent err/bound %.3f' % (tag, worst))
    assert worst <= 1.0, tag


def _check_fold(c, dhf, tag):
    if c.scale is None and c.oh is None:
        assert torch.equal(dhf.view(torch.int32), c.dh.view(torch.int32)), tag + ': dh changed'
        return
    ref, mag = lc.fold_ref(c.dh, c.scale, c.oh)
    r = lc.ratio(dhf, ref, 4 * lc.U * mag)
    print('%s: fold err/bound %.3f' % (tag, r))
    assert r <= 1.0, tag


LOOP_SHAPES = [
    (lc.LSTM, 128, 8),      # one row per group
    (lc.LSTM, 128, 15),     # the last group has 1 row
    (lc.LSTM, 128, 130),    # 17-row groups, ragged last group, past the 16-row fragment
    (lc.LSTM, 128, 392),    # 49-row groups: two row blocks of 25 + 24
    (lc.LSTM, 256, 264),    # 33-row blocks: the third fragment holds one row
    (lc.LSTM, 512, 64),     # the third instantiation, 64 workgroups
    (lc.GRU, 128, 130),
    (lc.RNN, 128, 130),
]


@pytest.mark.parametrize('fold', [False, True], ids=['plain', 'folded'])
@pytest.mark.parametrize('T', [1, 2, 3, 4])
@pytest.mark.parametrize('cell,H,R', LOOP_SHAPES,
                         ids=['%s-H%d-R%d' % (lc.CELL_NAMES[s[0]], s[1], s[2]) for s in LOOP_SHAPES])
def test_loop_matches_fp64_per_element(cell, H, R, T, fold):
    c = lc.chain_case(cell, R, H, T, 0.5, fold)
    for form in (1, 0):
        tag = '%s %s R=%d H=%d T=%d fold=%d' % (FORMS[form], lc.CELL_NAMES[cell], R, H, T, fold)
        dG, dc, dhf = _run_loop(c, form)
        _check_fold(c, dhf, tag)
        _check_chain(c, dG, dc, tag)
        _check_self_consistent(c, dG, tag)


@CELLS
def test_loop_without_dropout(cell):
    c = lc.chain_case(cell, 130, 128, 3, 0.0, True)
    for form in (1, 0):
        tag = '%s %s p=0' % (FORMS[form], lc.CELL_NAMES[cell])
        dG, dc, dhf = _run_loop(c, form)
        _check_chain(c, dG, dc, tag)
        _check_self_consistent(c, dG, tag)


@CELLS
def test_forms_and_chained_step_launches_agree(cell):
    """both loop forms and T launches of the step kernel, each fed the one
    before's dG and carry, within chain_bound of the same reference"""
    c = lc.chain_case(cell, 130, 128, 4, 0.5, True)
    for form in (1, 0):
        dG, dc, _ = _run_loop(c, form)
        _check_chain(c, dG, dc, '%s %s shared case' % (FORMS[form], lc.CELL_NAMES[cell]))
    dGs, dg, cy = [None] * c.T, None, torch.zeros(c.R, c.H)
    for t in range(c.T - 1, -1, -1):
        dg, cy, _ = _run_step(lc.chain_step(c, t, dg, cy))
        dGs[t] = dg
    dG = torch.stack(dGs)
    _check_chain(c, dG, cy, 'step launches %s shared case' % lc.CELL_NAMES[cell])
    _check_self_consistent(c, dG, 'step launches %s' % lc.CELL_NAMES[cell])


def test_loop_entry_refuses_unsupported_shapes():
    c = lc.chain_case(lc.LSTM, 8, 128, 2)
    bad = lc.chain_case(lc.LSTM, 7, 128, 2)   # fewer rows than groups
    with pytest.raises(RuntimeError):
        _run_loop(bad, 1)
    with pytest.raises(RuntimeError):         # whhT of another width
        _ops().lstm_bwd_loop_test(_dev(c.whhT[:, :256].contiguous()), _dev(c.dh), _dev(c.gates),
                                  _dev(c.c_all), c.p, _rng(c), c.cell, 1)
