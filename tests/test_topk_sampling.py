"""Truncated (top-k / nucleus) sampling on the CPU: ``truncated_probs``
against hand-computed distributions and the fp64 oracle, the PyTorch path of
``CaptionModel.sample`` (greedy at ``top_k = 1``, unchanged at ``top_k = 0``,
membership, the draw frequencies), ``sample_mbr`` with ``mbr_top_k`` /
``mbr_top_p``, the flags and ``Trainer.validate``."""
import math

import numpy as np
import pytest
import torch

import topk_sampling_cases as tc

MARGIN = 1e-3  # least distance of a nucleus cut from the cumulative mass


def _tp(lp, k, p=1.0, tau=1.0):
    from cst_captioning_amd.models.caption_model import truncated_probs
    return truncated_probs(torch.as_tensor(lp, dtype=torch.float64).view(1, -1), k, p, tau)[0]


P4 = np.array([0.5, 0.2, 0.2, 0.1])


def test_truncated_probs_top1_and_full_softmax():
    lp = np.log(P4)
    assert _tp(lp, 1).tolist() == [1.0, 0.0, 0.0, 0.0]
    # k = V, p = 1: the plain tempered softmax; top_k = 0 the same
    np.testing.assert_allclose(_tp(lp, 4).numpy(), P4, rtol=1e-12)
    np.testing.assert_allclose(_tp(lp, 0).numpy(), P4, rtol=1e-12)
    sq = P4 ** 2 / (P4 ** 2).sum()  # tau = 0.5 squares the probabilities
    np.testing.assert_allclose(_tp(lp, 4, 1.0, 0.5).numpy(), sq, rtol=1e-12)
    np.testing.assert_allclose(_tp(lp, 0, 1.0, 0.5).numpy(), sq, rtol=1e-12)
    # top 3 at tau = 2: square roots of 0.5, 0.2, 0.2
    r = np.sqrt(P4[:3])
    np.testing.assert_allclose(_tp(lp, 3, 1.0, 2.0).numpy(), list(r / r.sum()) + [0.0],
                               rtol=1e-12)


def test_truncated_probs_nucleus_cut_in_the_middle():
    lp = np.log(P4)
    # top 3: q = (5, 2, 2) / 9, cumulative 0.556, 0.778, 1; p = 0.7 keeps two
    ex = tc.exact_truncated(lp, 3, 0.7, 1.0)
    assert ex.m == 2 and ex.margin >= MARGIN
    np.testing.assert_allclose(_tp(lp, 3, 0.7).numpy(), [5 / 7, 2 / 7, 0, 0], rtol=1e-12)
    # p = 0.5 keeps the first alone, p = 0.8 all three
    assert tc.exact_truncated(lp, 3, 0.5, 1.0).margin >= MARGIN
    assert _tp(lp, 3, 0.5).tolist() == [1.0, 0.0, 0.0, 0.0]
    assert tc.exact_truncated(lp, 3, 0.8, 1.0).margin >= MARGIN
    np.testing.assert_allclose(_tp(lp, 3, 0.8).numpy(), [5 / 9, 2 / 9, 2 / 9, 0], rtol=1e-12)
    # tau = 0.5 inside the top 3: (25, 4, 4) / 33, cumulative 0.758, 0.879, 1
    ex = tc.exact_truncated(lp, 3, 0.8, 0.5)
    assert ex.m == 2 and ex.margin >= MARGIN
    np.testing.assert_allclose(_tp(lp, 3, 0.8, 0.5).numpy(), [25 / 29, 4 / 29, 0, 0], rtol=1e-12)


def test_truncated_probs_equal_values_keep_the_smaller_index():
    lp = np.log(np.array([0.2, 0.5, 0.1, 0.2]))
    np.testing.assert_allclose(_tp(lp, 2).numpy(), [2 / 7, 5 / 7, 0, 0], rtol=1e-12)
    # all equal: the first k indices, in order; the nucleus takes a prefix of them
    lp = np.log(np.full(5, 0.2))
    assert _tp(lp, 3).tolist() == pytest.approx([1 / 3, 1 / 3, 1 / 3, 0, 0])
    assert tc.exact_truncated(lp, 3, 0.5, 1.0).margin >= MARGIN
    assert _tp(lp, 3, 0.5).tolist() == pytest.approx([0.5, 0.5, 0, 0, 0])


@pytest.mark.parametrize('layout', tc.LAYOUTS)
def test_truncated_probs_matches_oracle_on_kernel_cases(layout):
    from cst_captioning_amd.models.caption_model import truncated_probs
    x = tc.kernel_logits(300, layout)
    lp = torch.log_softmax(torch.from_numpy(x).double(), 0)
    for k in (1, 2, 5, 8):
        for tau in (1.0, 0.7):
            for p in (1.0, 0.9, 0.5):
                ex = tc.exact_truncated(x, k, p, tau)
                assert ex.margin >= MARGIN, (layout, k, tau, p, ex.margin)
                got = truncated_probs(lp.view(1, -1), k, p, tau)[0].numpy()
                assert (got > 0).sum() == ex.m and set(np.flatnonzero(got)) == set(ex.order[:ex.m])
                np.testing.assert_allclose(got, ex.probs, rtol=1e-9, atol=1e-15)
                # fp32 input: the same kept set
                got32 = truncated_probs(lp.float().view(1, -1), k, p, tau)[0]
                assert got32.dtype == torch.float32
                assert set(np.flatnonzero(got32.numpy())) == set(ex.order[:ex.m])


def test_truncation_argument_errors():
    from cst_captioning_amd.models.caption_model import check_truncation, truncated_probs
    lp = torch.log_softmax(torch.randn(2, 6), 1)
    for k, p in [(-1, 1.0), (1.5, 1.0), (2, 0.0), (2, 1.5), (2, float('nan')), (2, -0.1),
                 (2, float('inf')), (0, 0.9), (7, 1.0)]:
        with pytest.raises(ValueError):
            truncated_probs(lp, k, p)
    with pytest.raises(ValueError):
        truncated_probs(lp, 2, 1.0, 0.0)
    assert check_truncation(0, 1.0) == (0, 1.0) and check_truncation(3, 0.5, 10) == (3, 0.5)


# -- the PyTorch path of sample ------------------------------------------------------
def _model(**extra):
    from cst_captioning_amd.cli import build_model
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import make_synthetic
    ds = make_synthetic('msvd', num_videos=10, vocab_size=40, seq_length=10, feat_dims=[16, 8],
                        seed=3)
    kw = dict(batch_size=4, train_seq_per_img=3, rnn_size=32, input_encoding_size=32,
              beam_size=1, impl='torch', drop_prob_lm=0.0)
    kw.update(extra)
    opt = default_opts(**kw)
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    opt.vocab_size, opt.seq_length, opt.feat_dims = ds.vocab_size, ds.seq_length, ds.feat_dims
    torch.manual_seed(7)
    model, _ = build_model(opt, torch.device('cpu'), 'torch')
    with torch.no_grad():  # a decoder that says something
        model.logit.weight.mul_(3.0)
    model.eval()
    return model, ds


def _feats(ds, B=4):
    from cst_captioning_amd.data import CaptionLoader
    return CaptionLoader(ds, B, 3, 'test', 'cpu').get_batch_at(0)['feats']


def test_sample_top1_is_greedy_and_top0_is_unchanged():
    model, ds = _model()
    feats = _feats(ds)
    g_seq, g_lp = model.sample(feats, {'sample_max': 1})
    torch.manual_seed(1)
    seq, lp = model.sample(feats, {'sample_max': 0, 'top_k': 1, 'temperature': 0.7})
    assert torch.equal(seq, g_seq) and torch.equal(lp, g_lp)
    # greedy ignores both keys
    seq, lp = model.sample(feats, {'sample_max': 1, 'top_k': 3, 'top_p': 0.5})
    assert torch.equal(seq, g_seq) and torch.equal(lp, g_lp)
    # top_k = 0: the call without the keys, draw for draw
    for tau in (1.0, 0.8):
        torch.manual_seed(5)
        a = model.sample(feats, {'sample_max': 0, 'temperature': tau})
        torch.manual_seed(5)
        b = model.sample(feats, {'sample_max': 0, 'temperature': tau, 'top_k': 0, 'top_p': 1.0})
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for bad in ({'top_k': -1}, {'top_p': 0.0}, {'top_p': 0.9}, {'top_k': 2, 'top_p': 1.01},
                {'top_k': 41}):
        with pytest.raises(ValueError):
            model.sample(feats, dict(bad, sample_max=0))


@pytest.mark.parametrize('k,p,tau', [(3, 0.9, 1.0), (5, 1.0, 0.7), (2, 0.97, 2.0)])
def test_sample_membership(k, p, tau):
    model, ds = _model()
    feats = _feats(ds)
    model.set_seq_per_img(6)
    torch.manual_seed(2)
    seq, lp = model.sample(feats, {'sample_max': 0, 'top_k': k, 'top_p': p, 'temperature': tau,
                                   'expand_feat': 1})
    assert seq.size(0) == 24
    pred = tc.teacher_force(model, feats, seq, 6)
    inside, _, alive, lp_ref = tc.membership(pred, seq, k, p, tau)
    assert alive.sum() > 24 and inside[alive].all()
    n = pred.size(1)
    assert (lp[:, :n].double() - lp_ref).abs()[alive].max() < 1e-5  # the untruncated log-prob
    # the draws are not all the best word: the truncation leaves a choice
    assert (seq[:, :n] != pred.argmax(2))[alive].any()
    # the plain sampler leaves the top-k set somewhere in as many draws
    torch.manual_seed(2)
    seq0, _ = model.sample(feats, {'sample_max': 0, 'temperature': 2.0, 'expand_feat': 1})
    pred0 = tc.teacher_force(model, feats, seq0, 6)
    in0, _, alive0, _ = tc.membership(pred0, seq0, k, p, tau)
    assert not in0[alive0].all()


def test_sampler_chi_square_against_truncated_probs():
    """The first sampled word of 6,000 rows of one video: every row draws from
    the same distribution, known from the teacher-forced log-probs."""
    from scipy.stats import chisquare
    from cst_captioning_amd.models.caption_model import truncated_probs
    model, ds = _model()
    feats = _feats(ds, B=1)
    k, p, tau, N = 8, 0.9, 0.7, 6000
    model.set_seq_per_img(N)
    torch.manual_seed(13)
    seq, _ = model.sample(feats, {'sample_max': 0, 'top_k': k, 'top_p': p, 'temperature': tau,
                                  'expand_feat': 1})
    pred = tc.teacher_force(model, feats, seq[:1], 1)
    lp0 = pred[0, 0].double()
    ex = tc.exact_truncated(lp0.numpy(), k, p, tau)
    assert ex.margin >= MARGIN and ex.m >= 3, (ex.m, ex.margin)
    want = truncated_probs(lp0.view(1, -1), k, p, tau)[0].numpy()
    np.testing.assert_allclose(want, ex.probs, rtol=1e-9, atol=1e-15)
    counts = np.bincount(seq[:, 0].numpy(), minlength=len(want))
    assert counts[want == 0].sum() == 0
    kept = want > 0
    assert (want[kept] * N >= 5).all()
    stat, pval = chisquare(counts[kept], want[kept] * N)
    assert pval > 1e-4, (stat, pval)


def test_sample_mbr_truncates_the_sampled_rows_only():
    from cst_captioning_amd.ops.mbr import PeerCiderD
    model, ds = _model()
    feats = _feats(ds)
    scorer = PeerCiderD(ds.df, use_eos=1, backend='cpu')
    base = {'decode': 'mbr', 'beam_size': 1, 'mbr_samples': 6, 'mbr_temperature': 0.9,
            'mbr_scorer': scorer}
    before = model.seq_per_img
    torch.manual_seed(11)
    plain = model.sample_mbr(feats, base)[2]['pool']
    torch.manual_seed(11)
    same = model.sample_mbr(feats, dict(base, mbr_top_k=0, mbr_top_p=1.0))[2]['pool']
    assert torch.equal(plain, same)
    torch.manual_seed(11)
    pool = model.sample_mbr(feats, dict(base, mbr_top_k=3, mbr_top_p=0.9))[2]['pool']
    assert model.seq_per_img == before
    B, G, T = pool.shape
    assert (B, G) == (4, 7)
    # row 0, the standard caption, is what it was
    std, _ = model.sample(feats, {'beam_size': 1})
    assert torch.equal(pool[:, 0, :std.size(1)], std) and not pool[:, 0, std.size(1):].any()
    w = min(T, plain.size(2))
    assert torch.equal(pool[:, 0, :w], plain[:, 0, :w])
    # rows 1..N obey membership under their own teacher-forced log-probs
    rows = pool[:, 1:].reshape(B * 6, T)
    pred = tc.teacher_force(model, feats, rows, 6)
    inside, _, alive, _ = tc.membership(pred, rows, 3, 0.9, 0.9)
    assert inside[alive].all()
    plain_rows = plain[:, 1:].reshape(B * 6, -1)
    in0, _, alive0, _ = tc.membership(tc.teacher_force(model, feats, plain_rows, 6), plain_rows,
                                      3, 0.9, 0.9)
    assert not in0[alive0].all()  # (the plain pool does leave the set)
    for bad in ({'mbr_top_k': -2}, {'mbr_top_p': 0.5}, {'mbr_top_k': 2, 'mbr_top_p': 0.0}):
        with pytest.raises(ValueError):
            model.sample_mbr(feats, dict(base, **bad))


# -- flags, trainer ------------------------------------------------------------------
def test_flags_defaults_and_refusals(capsys):
    from cst_captioning_amd.config import default_opts, parse_opts
    opt = parse_opts([])
    assert (opt.mbr_top_k, opt.mbr_top_p) == (0, 1.0)
    assert type(opt.mbr_top_k) is int and type(opt.mbr_top_p) is float
    d = default_opts()
    assert (d.mbr_top_k, d.mbr_top_p) == (0, 1.0)
    opt = parse_opts(['--decode', 'mbr', '--mbr_top_k', '3', '--mbr_top_p', '0.9'])
    assert (opt.mbr_top_k, opt.mbr_top_p) == (3, 0.9)
    assert parse_opts(['--mbr_top_k', '12']).mbr_top_k == 12
    for bad in (['--mbr_top_k', '-1'], ['--mbr_top_k', '2.5'], ['--mbr_top_k', 'x'],
                ['--mbr_top_k', '3', '--mbr_top_p', '0'],
                ['--mbr_top_k', '3', '--mbr_top_p', '1.2'],
                ['--mbr_top_k', '3', '--mbr_top_p', '-0.5'],
                ['--mbr_top_k', '3', '--mbr_top_p', 'nan'],
                ['--mbr_top_k', '3', '--mbr_top_p', 'inf'],
                ['--mbr_top_p', '0.9'],
                ['--mbr_top_k', '0', '--mbr_top_p', '0.5']):
        with pytest.raises(SystemExit):
            parse_opts(bad)
        assert 'mbr_top' in capsys.readouterr().err, bad


def _trainer(**extra):
    from cst_captioning_amd.cli import build_model
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import CaptionLoader, make_synthetic
    from cst_captioning_amd.train.trainer import Trainer
    ds = make_synthetic('msvd', num_videos=10, vocab_size=40, seq_length=10, feat_dims=[16, 8],
                        seed=3)
    kw = dict(batch_size=4, train_seq_per_img=3, test_batch_size=4, test_seq_per_img=3,
              rnn_size=32, input_encoding_size=32, beam_size=2, impl='torch', drop_prob_lm=0.0,
              val_scorer='tokens', max_epochs=1, print_log_interval=0, use_eos=1)
    kw.update(extra)
    opt = default_opts(**kw)
    dev = torch.device('cpu')
    opt.vocab = {i: w for i, w in enumerate(ds.vocab)}
    opt.vocab_size, opt.seq_length, opt.feat_dims = ds.vocab_size, ds.seq_length, ds.feat_dims
    torch.manual_seed(7)
    model, engine = build_model(opt, dev, 'torch')
    train = CaptionLoader(ds, 4, 3, 'train', dev)
    val = CaptionLoader(ds, 4, 3, 'test', dev)
    return Trainer(opt, model, train, val, None, engine), val, ds


def test_trainer_validate_with_truncated_mbr():
    from cst_captioning_amd.train.trainer import Trainer
    tr, val, ds = _trainer(decode='mbr', mbr_samples=5, mbr_top_k=3, mbr_top_p=0.9)
    o = tr.decode_opts()
    assert (o['mbr_top_k'], o['mbr_top_p']) == (3, 0.9)
    torch.manual_seed(3)
    res = tr.validate(val)
    assert len(res['predictions']) == 10
    assert all(isinstance(p['mbr_score'], float) for p in res['predictions'])
    assert math.isfinite(res['scores']['CIDEr'])
    # the defaults leave the decode options' truncation off
    tr0, _, _ = _trainer(decode='mbr', mbr_samples=5)
    o = tr0.decode_opts()
    assert (o['mbr_top_k'], o['mbr_top_p']) == (0, 1.0)
    # option objects built without the parser are checked at set-up
    for k, p in [(-1, 1.0), (0, 0.5), (3, 0.0), (3, 1.5), (3, float('nan'))]:
        tr.opt.mbr_top_k, tr.opt.mbr_top_p = k, p
        with pytest.raises(ValueError, match='mbr_top'):
            Trainer(tr.opt, tr.model, tr.train_loader, val, None, None)
