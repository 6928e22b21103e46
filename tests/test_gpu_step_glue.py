"""Framework glue launches taken off the training step's critical path:
FeatPool reading its rows out of the resident tables by index, the decoder's
rollout reading its label rows by index, the FeatPool epilogue's bf16 side
output, the gradient bucket's narrowed zero
fill, the end-of-sequence flag words / row masks initialised by the decode's
first launch, and the weight-gradient reduce storing through a destination
row map.  Every comparison is exact (``torch.equal``): none of these changes
touches a GEMM, a reduction order or an RNG draw."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _ops():
    from cst_captioning_amd import _ext
    assert _ext.available(), 'native extension must be built for GPU tests'
    return _ext.ops()


def _trainer(seed=0, layers=1, rnn_type='lstm', rl=True, L=6, drop=0.5, H=64):
    """Tiny trainer on the fused engine: V = 37, H = E = 64, 3 videos x 2
    captions, eager steps."""
    from cst_captioning_amd.cli import build_model
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import CaptionLoader, make_synthetic
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.train.trainer import Trainer
    V, B, S = 37, 3, 2
    ds = make_synthetic('msrvtt', num_videos=12, vocab_size=V, seq_length=L, feat_dims=[64, 32],
                        seed=seed)
    opt = default_opts(vocab_size=V, seq_length=L, feat_dims=[64, 32], train_seq_per_img=S,
                       batch_size=B, rnn_size=H, input_encoding_size=H, drop_prob_lm=drop,
                       num_layers=layers, rnn_type=rnn_type, use_rl=int(rl), use_rl_after=0,
                       use_cst=0, use_mixer=1, mixer_from=1, use_eos=1, impl='hip', cuda_graph=0,
                       learning_rate=1e-3)
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    torch.manual_seed(seed)
    dev = torch.device(DEV)
    model, engine = build_model(opt, dev, 'hip')
    assert engine is not None
    loader = CaptionLoader(ds, B, S, 'train', dev, seed=seed)
    tr = Trainer(opt, model, loader, None, DistContext(device=dev), engine)
    tr.rl_training = bool(rl)
    return tr, loader


class _pinned_seeds:
    """Dropout / sampling seeds pinned on the device for the trainers given."""

    def __init__(self, *trainers):
        self.trainers = trainers
        self.fixed = torch.tensor([24680, 13579], dtype=torch.int32, device=DEV)

    def __enter__(self):
        from cst_captioning_amd.ops import featpool as fp
        self.old = fp.SEED_SOURCE
        fp.SEED_SOURCE = lambda dev: self.fixed
        for tr in self.trainers:
            tr.engine._rng = lambda dev: self.fixed
        return self.fixed

    def __exit__(self, *exc):
        from cst_captioning_amd.ops import featpool as fp
        fp.SEED_SOURCE = self.old


def _featpool_operands(rows=70, dims=(64, 36), H=64, seed=0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    xs = [torch.randn(rows, d, generator=g).to(DEV) for d in dims]
    ws = [(torch.randn(H, d, generator=g) / d ** 0.5).to(DEV) for d in dims]
    bs = [(0.1 * torch.randn(H, generator=g)).to(DEV) for _ in dims]
    return xs, ws, bs


# ---- indexed FeatPool -------------------------------------------------------------

@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('C', [1, 3])
def test_indexed_featpool_equals_gathered_rows(C, p):
    """FeatPool reading its rows out of a resident table through an index
    (a repeat, unordered, the last row) against the same call on
    ``index_select``-ed rows: two modalities cut out of one concatenated table
    (widths 36 and 64: the second starts at a 16-byte-aligned, non-zero column
    offset), H = 64, C frames per table row; forward (fp32 and bf16) and every
    backward output, dropout seeds pinned."""
    ops = _ops()
    H = 64
    g = torch.Generator(device='cpu').manual_seed(11 * C)
    table = torch.randn(11, C, 100, generator=g).to(DEV)
    idx = torch.tensor([7, 0, 7, 3, 10], device=DEV)
    cut = lambda t: [t[..., :36].reshape(-1, 36), t[..., 36:].reshape(-1, 64)]
    xs_t, xs_g = cut(table), cut(table.index_select(0, idx))
    assert all(x.data_ptr() == t.data_ptr() for x, t in zip(xs_t, [table[..., :36], table[..., 36:]]))
    assert xs_t[1].data_ptr() % 16 == 0 and xs_t[1].data_ptr() != xs_t[0].data_ptr()
    ws = [(torch.randn(H, d, generator=g) / d ** 0.5).to(DEV) for d in (36, 64)]
    bs = [(0.1 * torch.randn(H, generator=g)).to(DEV) for _ in range(2)]
    rng = torch.tensor([24680, 13579], dtype=torch.int32, device=DEV)
    ref = ops.featpool_forward(xs_g, ws, bs, p, rng)
    out = ops.featpool_forward(xs_t, ws, bs, p, rng, idx, C)
    assert out.shape == (5 * C, 2 * H)
    assert torch.equal(out, ref)
    fc, fc16 = ops.featpool_forward16(xs_t, ws, bs, p, rng, idx, C)
    assert torch.equal(fc, ref) and torch.equal(fc16, ref.to(torch.bfloat16))
    if p == 0.0:  # the repeated table row gives the same output rows
        assert torch.equal(out[:C], out[2 * C:3 * C])
    dout = torch.randn(5 * C, 2 * H, generator=g).to(DEV)
    want = ops.featpool_backward(dout, ref, xs_g, ws, p, [])
    got = ops.featpool_backward(dout, out, xs_t, ws, p, [], idx, C)
    assert len(got) == len(want) == 4
    for a, b in zip(got, want):
        assert torch.equal(a, b) and a.abs().sum() > 0
    # (the kernels clamp an index to the table's rows, ``fp_row``; no
    # out-of-range index is passed here: a broken clamp must fail an
    # assertion, not read outside the table)


def test_training_step_reads_features_by_index():
    """The trainer hands the fused FeatPool the resident tables + the batch's
    index (nothing is gathered: ``feats`` never materialises in an SCST step),
    and the step equals the one run on the gathered copy."""
    a, la = _trainer(seed=6)
    b, lb = _trainer(seed=6)
    b._feats = lambda data: data['feats']  # (b: the gathered copy throughout)
    with _pinned_seeds(a, b):
        for _ in range(2):
            da, db = la.get_batch(), lb.get_batch()
            assert a.engine.reads_by_index(a.model, da.feats_indexed())
            oa, ob = a.train_step(da, 0), b.train_step(db, 0)
            torch.cuda.synchronize()
            assert not dict.__contains__(da, 'feats') and dict.__contains__(db, 'feats')
            assert torch.equal(oa['seq'], ob['seq'])
            assert torch.equal(a.bucket.grad, b.bucket.grad)
    assert torch.equal(a.bucket.data, b.bucket.data)
    # every other consumer still gets the gathered rows
    d = la.get_batch()
    f = d.feats_indexed()
    assert torch.equal(f[0], f.tables[0].index_select(0, f.index)) and len(f) == 2
    assert d.feats_indexed() is None  # (gathered now: the copy is the batch's features)


# ---- labels read by index ---------------------------------------------------------

@pytest.mark.parametrize('mixer_from', [1, 3])
def test_rollout_reads_label_rows_by_index(mixer_from):
    """The engine's rollout reading its label rows out of the resident table
    through a row index (a repeat, unordered, the table's last row) against
    the same call on ``index_select``-ed rows: the step-0 input token, the
    target lookups of the decode launches and the combines' ground-truth
    tokens (mixer_from = 3: tokens 1-2 teacher-forced, the rest sampled;
    1: all sampled)."""
    from cst_captioning_amd.data.dataset import IndexedLabels
    tr, loader = _trainer(seed=4)
    tr.model.train()
    tr.model.set_mixer_from(mixer_from)
    data = loader.get_batch()
    table = data.labels_indexed().table
    n = table.size(0)
    idx = torch.tensor([n - 1, 0, n - 1, 3, 1, 2], device=DEV)
    rows = table.index_select(0, idx)
    assert rows[:, 1:].ne(0).any()
    with _pinned_seeds(tr), torch.no_grad():
        seq_g, lp_g, _ = tr.engine.rollout(tr.model, tr._feats(data), rows)
        seq_i, lp_i, _ = tr.engine.rollout(tr.model, tr._feats(data),
                                           IndexedLabels(None, table, idx))
    torch.cuda.synchronize()
    assert torch.equal(seq_i, seq_g) and torch.equal(lp_i, lp_g)
    if mixer_from == 3:  # the teacher-forced tokens are the indexed rows' labels
        assert torch.equal(seq_i[:, :2], rows[:, 1:3])


@pytest.mark.parametrize('mixer_from', [1, 3])
def test_training_step_reads_labels_by_index(mixer_from):
    """The trainer hands the rollout the resident label table + the batch's
    caption rows (``labels`` never materialises in an SCST step), and the
    step -- forward, backward with its input-token rows, update -- equals the
    one run on the gathered copy.  The XE step still gets the gathered
    rows."""
    a, la = _trainer(seed=8)
    b, lb = _trainer(seed=8)
    a.opt.mixer_from = b.opt.mixer_from = mixer_from
    b._rollout_labels = lambda data: data['labels']  # (b: the gathered copy throughout)
    with _pinned_seeds(a, b):
        for _ in range(2):
            da, db = la.get_batch(), lb.get_batch()
            oa, ob = a.train_step(da, 0), b.train_step(db, 0)
            torch.cuda.synchronize()
            assert not dict.__contains__(da, 'labels') and dict.__contains__(db, 'labels')
            assert torch.equal(oa['seq'], ob['seq'])
            assert torch.equal(a.bucket.grad, b.bucket.grad)
    assert torch.equal(a.bucket.data, b.bucket.data)
    d = la.get_batch()
    lab = d.labels_indexed()
    assert torch.equal(lab.gathered(), lab.table.index_select(0, lab.index))
    assert d.labels_indexed() is None  # (gathered now: the copy is the batch's labels)
    x, lx = _trainer(seed=8, rl=False)
    dx = lx.get_batch()
    x.train_step(dx, 0)
    torch.cuda.synchronize()
    assert dict.__contains__(dx, 'labels')  # (the XE loss reads the gathered rows)


# ---- bf16 side output -------------------------------------------------------------

@pytest.mark.parametrize('p', [0.0, 0.5])
def test_featpool_bf16_side_output_equals_conversion(p):
    """The epilogue's bf16 copy is ``fc.to(bfloat16)`` (round to nearest
    even) and fc itself is what featpool_forward returns: random rows
    (exact zeros from the ReLU, dropped entries at p = 0.5) over more than one
    row tile, plus a modality with an identity weight whose inputs sit on the
    bf16 rounding boundaries (a value just above half an ulp rounds up, the two
    ties go to the even neighbour)."""
    ops = _ops()
    xs, ws, bs = _featpool_operands()
    H = 64
    # third modality: out = relu(x) exactly (w = I, b = 0; hi + lo split exact)
    edge = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -10,  # above the midpoint: up to 1 + 2^-7
                         1 + 2.0 ** -8,               # tie: down to the even 1.0
                         1 + 2.0 ** -7 + 2.0 ** -8,   # tie: up to the even 1 + 2^-6
                         -3.0, 0.0, 2.0 ** -20])
    x2 = edge.repeat(70 * H // edge.numel() + 1)[:70 * H].view(70, H).to(DEV)
    xs, ws, bs = xs + [x2], ws + [torch.eye(H, device=DEV)], bs + [torch.zeros(H, device=DEV)]
    rng = torch.tensor([24680, 13579], dtype=torch.int32, device=DEV)
    ref = ops.featpool_forward(xs, ws, bs, p, rng)
    fc, fc16 = ops.featpool_forward16(xs, ws, bs, p, rng)
    assert fc16.dtype == torch.bfloat16 and fc16.shape == fc.shape
    assert torch.equal(fc, ref)
    assert torch.equal(fc16, ref.to(torch.bfloat16))
    assert (ref == 0).any() and (ref > 0).any()
    if p == 0.0:  # the boundary inputs reached the conversion unchanged
        assert torch.equal(ref[:, 2 * H:], x2.clamp(min=0))
        got = fc16[:, 2 * H:].float().reshape(-1)[:3].tolist()
        assert got == [1 + 2.0 ** -7, 1.0, 1 + 2.0 ** -6]
    else:
        kept = (ref[:, 2 * H:] != 0)
        assert kept.any() and not kept[x2 > 0].all()  # some positive entries were dropped


# ---- narrowed zeroing -------------------------------------------------------------

def _two_steps(layers):
    """Step 1 (full fill) on two identical trainers, then step 2 with the
    bucket NaN-filled (a) / zero-filled by the test (b) beforehand."""
    a, la = _trainer(seed=2, layers=layers)
    b, lb = _trainer(seed=2, layers=layers)
    with _pinned_seeds(a, b):
        for tr, ld in ((a, la), (b, lb)):
            tr.train_step(ld.get_batch(), 0)
        assert not a.bucket.narrow_zeroed  # the first step always gets the full fill
        a.bucket.grad.fill_(float('nan'))
        b.bucket.grad.zero_()
        oa = a.train_step(la.get_batch(), 0)
        ob = b.train_step(lb.get_batch(), 0)
        torch.cuda.synchronize()
    return a, b, oa, ob, la


def test_narrowed_zero_fill_leaves_no_sentinel():
    """One-layer concat model: the second step's zero_grad skips the direct
    slots; a NaN sentinel in the whole bucket is gone after the step and every
    gradient equals the run whose bucket the test zeroed itself.  Then a step
    with a non-finite loss: counted as skipped, parameters unchanged."""
    a, b, oa, ob, la = _two_steps(layers=1)
    assert a.bucket.narrow_zeroed and b.bucket.narrow_zeroed
    assert torch.equal(oa['seq'], ob['seq'])
    assert not torch.isnan(a.bucket.grad).any()
    assert torch.equal(a.bucket.grad, b.bucket.grad)
    assert torch.equal(a.bucket.data, b.bucket.data)
    # the fills cover exactly the complement of the direct slots
    covered = torch.zeros(a.bucket.grad.numel(), dtype=torch.int32)
    for lo, hi in a.bucket._zero_pieces + a.bucket._over_pieces:
        covered[lo:hi] += 1
    assert bool((covered == 1).all())
    assert len(a.bucket._zero_pieces) <= len(a.bucket._over_pieces) + 1
    # non-finite loss: the update is skipped and counted
    orig = a.rl_loss

    def bad_loss(data, scb):
        loss, extra = orig(data, scb)
        return loss * float('nan'), extra
    a.rl_loss = bad_loss
    before = a.bucket.data.clone()
    skipped0 = int(a.optimizer.skipped().item())
    with _pinned_seeds(a):
        a.train_step(la.get_batch(), 0)
    torch.cuda.synchronize()
    assert int(a.optimizer.skipped().item()) == skipped0 + 1
    assert torch.equal(a.bucket.data, before)
    # and the step after it trains again, on finite gradients
    a.rl_loss = orig
    with _pinned_seeds(a):
        a.train_step(la.get_batch(), 0)
    torch.cuda.synchronize()
    assert torch.isfinite(a.bucket.grad).all() and torch.isfinite(a.bucket.data).all()
    assert not torch.equal(a.bucket.data, before)


def test_stacked_layers_keep_the_full_fill():
    """num_layers = 2 has no full direct coverage: the full fill stays, and
    the sentinel does not survive there either."""
    a, b, oa, ob, _ = _two_steps(layers=2)
    assert not a.bucket.narrow_zeroed and not a.engine.direct_slots_covered()
    assert torch.equal(oa['seq'], ob['seq'])
    assert not torch.isnan(a.bucket.grad).any()
    assert torch.equal(a.bucket.grad, b.bucket.grad)
    assert torch.isfinite(a.bucket.data).all()


def test_uncovered_backward_after_a_narrowed_fill_zeroes_the_slots():
    """A step that was promised coverage but whose backward takes another path
    (here: the direct video-gate hand-off is withheld) zeroes the direct slots
    itself before anything accumulates into them."""
    a, la = _trainer(seed=5)
    b, lb = _trainer(seed=5)
    with _pinned_seeds(a, b):
        for tr, ld in ((a, la), (b, lb)):
            tr.train_step(ld.get_batch(), 0)
        a.bucket.grad.fill_(float('nan'))
        b.bucket.grad.zero_()
        b.bucket._covered = lambda: False  # (b: the full fill throughout)
        for tr, ld in ((a, la), (b, lb)):
            tr.engine.wiv_keep, tr.engine.wiv = tr.engine.wiv, None  # no vg_bwd this step
            tr.train_step(ld.get_batch(), 0)
            tr.engine.wiv = tr.engine.wiv_keep
        torch.cuda.synchronize()
    assert not a.engine._last_bwd_covered
    assert not torch.isnan(a.bucket.grad).any()
    assert torch.equal(a.bucket.grad, b.bucket.grad)


# ---- flag words and row masks without fill launches -------------------------------

def _poison(value, *sizes):
    """Fill freed blocks of the given byte sizes with ``value`` bytes, so the
    next call's uninitialised buffers hold it whichever block the allocator
    hands back (the tests below do not depend on block reuse)."""
    keep = [torch.full((n,), value, dtype=torch.uint8, device=DEV) for n in sizes for _ in range(4)]
    torch.cuda.synchronize()
    del keep


def _flag_bytes(T):
    return (T + 1) * 64 * 32 * 4  # (T + 1) steps x 64 slots x 128-byte lines


def _eos_bias(model, value):
    with torch.no_grad():
        model.logit.bias.zero_()
        model.logit.bias[0] = value


def test_eos_flag_words_are_initialised_by_the_first_launch():
    """Call A never emits EOS (bias -70): every step's flag words end up set.
    Call B, same shapes (the allocator hands back the same blocks), emits EOS
    in every row at step 1 (bias +70): its tokens after step 1 are all 0."""
    tr, loader = _trainer(seed=3, drop=0.0)
    eng, model = tr.engine, tr.model
    model.train()
    model.set_seq_per_img(2)
    model.set_mixer_from(1)  # every token sampled
    data = loader.get_batch()
    feats, labels = data['feats'], data['labels']
    with torch.no_grad():
        _eos_bias(model, -70.0)
        seq_a, _, _ = eng.rollout(model, feats, labels)
        assert bool((seq_a != 0).all())
        del seq_a
        _poison(1, _flag_bytes(labels.size(1) - 1))
        _eos_bias(model, 70.0)
        seq_b, _, _ = eng.rollout(model, feats, labels)
        torch.cuda.synchronize()
    assert bool((seq_b[:, 1:] == 0).all())


def test_stale_eos_flags_do_not_keep_a_finished_decode_alive():
    """The same with teacher-forced tokens, where only the flag words can stop
    the decode: call A's labels never hold EOS (every flag word set); call B,
    on the same blocks, has EOS in every row at step 1 and non-EOS labels
    after it -- the reference stops decoding once every row emitted EOS at one
    step, so B's later tokens are 0 unless it read A's flags."""
    tr, loader = _trainer(seed=3, drop=0.0)
    eng, model = tr.engine, tr.model
    model.train()
    model.set_seq_per_img(2)
    model.set_mixer_from(0)  # teacher forcing at every step
    data = loader.get_batch()
    feats = data['feats']
    lab_a = data['labels'].clone()
    lab_a[:, 1:] = lab_a[:, 1:].clamp(min=5)
    lab_b = lab_a.clone()
    lab_b[:, 1] = 0
    with torch.no_grad():
        seq_a, _, _ = eng.rollout(model, feats, lab_a)
        assert torch.equal(seq_a, lab_a[:, 1:1 + seq_a.size(1)])
        del seq_a
        _poison(1, _flag_bytes(lab_a.size(1) - 1))
        seq_b, _, _ = eng.rollout(model, feats, lab_b)
        torch.cuda.synchronize()
    assert bool((seq_b == 0).all())


def test_row_masks_are_initialised_by_the_first_launch():
    """The greedy decode's per-row "unfinished" mask: call A finishes every
    row at once (bias +70: the masks end up 0), call B on the same blocks never
    emits EOS (bias -70) and must not see A's masks -- no token is forced to 0."""
    tr, loader = _trainer(seed=3, drop=0.0)
    eng, model = tr.engine, tr.model
    model.eval()
    feats = loader.get_batch()['feats']
    _eos_bias(model, 70.0)
    seq_a, _ = eng.sample(model, feats, {'sample_max': 1})
    assert bool((seq_a == 0).all())
    rows = seq_a.size(0)
    del seq_a
    _poison(0, rows, 512)
    _eos_bias(model, -70.0)
    seq_b, _ = eng.sample(model, feats, {'sample_max': 1})
    torch.cuda.synchronize()
    assert bool((seq_b != 0).all())


# ---- permuted store ---------------------------------------------------------------

@pytest.mark.parametrize('H', [64, 128])
@pytest.mark.parametrize('rnn_type', ['lstm', 'gru', 'rnn'])
def test_direct_slots_hold_pytorch_gate_order(rnn_type, H):
    """R = 6, T = 4: W_ih's token columns and W_hh written by the engine into
    their slots equal the packed result returned to autograd and unpacked
    there with ``index_select`` (+ the accumulate onto zeros).  At H = E = 64
    the weight-gradient kernel does not take the shape (N must be a multiple
    of 128), so that case covers the engine's gather + copy fallback into the
    slots; H = E = 128 runs the kernel's row-mapped store inside the engine."""
    tr, loader = _trainer(seed=4, rnn_type=rnn_type, rl=False, L=4, drop=0.0, H=H)
    eng, model = tr.engine, tr.model
    E = eng.E
    model.train()
    model.set_seq_per_img(2)
    data = loader.get_batch()
    assert data['labels'].size(0) == 6
    rnn = model.core.rnn
    grads = []
    for direct in (True, False):
        slots = eng.direct_grad_slots
        if not direct:
            eng.direct_grad_slots = None
        tr.bucket.grad.fill_(float('nan'))
        tr.bucket._covered = lambda: False  # (full fill: both runs start from zeros)
        tr.optimizer.zero_grad()
        loss, _ = tr.xe_loss(data)
        loss.backward()
        torch.cuda.synchronize()
        eng.direct_grad_slots = slots
        grads.append((rnn.weight_ih_l0.grad[:, :E].clone(), rnn.weight_hh_l0.grad.clone()))
    (ie_d, hh_d), (ie_a, hh_a) = grads
    assert torch.isfinite(ie_d).all() and torch.isfinite(hh_d).all()
    assert ie_d.abs().sum() > 0 and hh_d.abs().sum() > 0
    assert torch.equal(ie_d, ie_a)
    assert torch.equal(hh_d, hh_a)


@pytest.mark.parametrize('K', [70, 600])  # one pass / split-K + reduce
@pytest.mark.parametrize('rnn_type', ['lstm', 'gru', 'rnn'])
def test_wgrad_row_map_store(rnn_type, K):
    """The weight-gradient kernel's destination row map (single-pass store and
    the split-K reduce) at the smallest shape the kernel takes (N = 128): rows
    land where ``index_select`` + ``copy_`` of the unmapped result puts them,
    in a slot that is wider than N and not 16-byte aligned; the rest of the
    slot is untouched."""
    from cst_captioning_amd.models.decoder_engine import gate_maps, inverse_rows
    ops = _ops()
    H, N = 32, 128
    M = 4 * H
    g = torch.Generator(device='cpu').manual_seed(K)
    A = torch.randn(K, M, generator=g).to(DEV, torch.bfloat16)
    B = torch.randn(K, N, generator=g).to(DEV, torch.bfloat16)
    full = ops.wgrad_tn(A, B, M, N, K)
    for _, dst, _ in gate_maps(rnn_type, H):
        dst = dst.to(DEV)
        inv = inverse_rows(dst, M)
        rows, ld = dst.numel(), N + 40
        for shift in (0, 1):  # 16-byte aligned rows / rows at an odd float offset
            buf = torch.full((rows * ld + 4,), -7.0, device=DEV)
            slot = buf[shift:shift + rows * ld].view(rows, ld)
            ops.wgrad_tn_rows(A, B, M, N, K, slot, inv)
            want = torch.full((rows, ld), -7.0, device=DEV)
            want[:, :N].copy_(full.index_select(0, dst))
            torch.cuda.synchronize()
            assert torch.equal(slot, want)
            assert bool((buf[:shift] == -7.0).all()) and bool((buf[shift + rows * ld:] == -7.0).all())
