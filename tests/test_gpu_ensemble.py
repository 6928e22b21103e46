"""Ensemble decoding on the fused engine: ``csrc/kernels/ensemble.hip`` through
its test route on the cases of ``tests/ensemble_cases.py``, its greedy
epilogue, ``beam_search.cpp`` ensemble_decode against a single member (bit
for bit), against the PyTorch ensemble on bf16-rounded weights (the project's
beam criterion) and against the members' own teacher-forced log-probs, the
refusals, and ``Trainer.test`` with an ensemble.  Tiny engine shapes
throughout (those of ``tests/test_gpu_cells.py``).

Greedy rows are compared up to and including a row's first 0: after it the
kernel writes log-prob 0 (its end-of-sequence rule) where the PyTorch loop
keeps recording the arg-max of rows it has already masked."""
import copy
import math

import numpy as np
import pytest
import torch

import ensemble_cases as ec

gpu = pytest.mark.gpu
DEV = 'cuda'
V, L, B = 300, 12, 6
DIMS = [48, 32]


def _member(cell, H, seed, dev, C=1, model_type='concat', layers=1, engine=True):
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.models import CaptionModel
    opt = default_opts(vocab_size=V, seq_length=L, feat_dims=DIMS, train_seq_per_img=1,
                       rnn_size=H, input_encoding_size=2 * H if model_type == 'standard' else H,
                       drop_prob_lm=0.0, rnn_type=cell, num_chunks=C, model_type=model_type,
                       num_layers=layers)
    torch.manual_seed(seed)
    model = CaptionModel(opt).to(dev)
    with torch.no_grad():  # peaked distributions: few near-ties
        model.logit.weight.mul_(9.0)
        model.core.rnn.weight_hh_l0.mul_(2.0)
    model.eval()
    eng = None
    if engine:
        from cst_captioning_amd.models.decoder_engine import DecoderEngine
        eng = DecoderEngine(model, opt)
    return model, eng


def _feats(dev, C=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, C, d, generator=g).to(dev) for d in DIMS]


# (name, members (cell, H), weights, num_chunks)
ENSEMBLES = [('m2_lstm_gru', [('lstm', 64), ('gru', 128)], [0.6, 0.4], 1),
             ('m3_att2', [('lstm', 64), ('gru', 128), ('lstm', 128)], None, 2)]


def _ensemble(spec, dev, engine=True):
    from cst_captioning_amd.models.ensemble import EnsembleCaptionModel
    name, kinds, weights, C = spec
    ms, engs = zip(*[_member(c, H, 10 + i, dev, C=C, engine=engine)
                     for i, (c, H) in enumerate(kinds)])
    ens = EnsembleCaptionModel(list(ms), weights)
    if engine:
        from cst_captioning_amd.models.decoder_engine import EnsembleEngine
        EnsembleEngine(ens, list(engs))
    return ens, list(engs)


def _bf16_twin(ens):
    from cst_captioning_amd.models.ensemble import EnsembleCaptionModel
    ms = [copy.deepcopy(m) for m in ens.members]
    for m in ms:
        m.impl, m._engine = 'torch', None
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(p.bfloat16().float())
    return EnsembleCaptionModel(ms, ens.weights)


def _pad(x, n):
    return torch.nn.functional.pad(x, (0, n - x.size(1)))


def _live(seq):
    """Positions up to and including each row's first 0."""
    ended = (seq == 0).cumsum(1)
    return (ended - (seq == 0).long()) == 0


def _decode(ens, feats, K):
    seq, lp = ens.sample(feats, {'beam_size': K})
    n = L if K > 1 else L - 2
    return _pad(seq, n), _pad(lp.float(), n)


def _agreement(a, b, greedy):
    """(share of identical rows, largest log-prob difference on them): greedy
    rows up to their first 0, beam rows whole (a beam goes on after a 0)."""
    (sa, la), (sb, lb) = a, b
    same = (sa == sb).all(1)
    live = (_live(sa) if greedy else torch.ones_like(sa, dtype=torch.bool)) & same[:, None]
    return same.float().mean().item(), float(((la - lb).abs() * live).max())


@pytest.mark.parametrize('spec', ENSEMBLES, ids=[s[0] for s in ENSEMBLES])
def test_bf16_rounding_alone_keeps_the_criterion_on_the_cpu(spec):
    """The 0.8 cap of the GPU comparison below hides nothing: with these seeds
    the PyTorch ensemble with fp32 weights and the same ensemble with
    bf16-rounded weights already agree on at least 0.8 of the rows."""
    ens, _ = _ensemble(spec, 'cpu', engine=False)
    twin = _bf16_twin(ens)
    feats = _feats('cpu', spec[3])
    with torch.no_grad():
        for K in (1, 3, 9):
            frac, _ = _agreement(_decode(ens, feats, K), _decode(twin, feats, K), K == 1)
            assert frac >= 0.8, (K, frac)


# -- the kernel through its test route -----------------------------------------------------
def _route(C, case, unfinished=None):
    e = torch.empty(0, device=DEV)
    return C.vocab_select(e, e, e, e, 1, 1.0, 0,
                          ens_logits=[torch.from_numpy(z).to(DEV) for z in case['logits']],
                          ens_lse=[torch.from_numpy(x).to(DEV) for x in case['lse']],
                          ens_logw=[float(x) for x in case['logw']], ens_V=case['V'],
                          ens_K=case['K'], ens_unfinished=unfinished)


CASES = ec.cases()


@gpu
@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_kernel_meets_every_case(case):
    from cst_captioning_amd import _ext
    C = _ext.ops()
    v, i = _route(C, case)
    v2, i2 = _route(C, case)
    assert torch.equal(v, v2) and torch.equal(i, i2)  # a relaunch is bit-equal
    v, i = v.cpu().numpy(), i.cpu().numpy()
    err = np.abs(v.astype(np.float64) - case['ref_v']).max() if i.shape == case['ref_i'].shape \
        else float('nan')
    print('%s: max |e - e_ref| = %.3g, bound %.3g' % (case['name'], err, case['bound']))
    assert (i >= 0).all() and (i < case['V']).all() and (np.abs(v) < 1e20).all()  # no padding
    assert ec.check(case, v, i) is None, ec.check(case, v, i)
    if case['M'] == 1:  # bit-equal to z - lse
        want = np.take_along_axis(case['logits'][0], i.astype(np.int64), 1) - case['lse'][0][:, None]
        assert np.array_equal(v, want)


@gpu
def test_greedy_epilogue_keeps_finished_rows_at_zero():
    """Three hand-made steps of 4 rows x 2 members: row 0 draws 0 at step 1,
    row 1 at step 2, row 2 never, row 3 at step 1 and a non-zero arg-max later
    (which the rule must suppress)."""
    from cst_captioning_amd import _ext
    C = _ext.ops()
    R, Vv, ldl = 4, 37, 40
    arg = [[0, 5, 7, 0], [9, 0, 8, 11], [4, 6, 3, 12]]  # the mixture's arg-max per step and row
    unf = torch.ones(R, dtype=torch.uint8, device=DEV)
    logw = [math.log(0.25), math.log(0.75)]
    alive = [True] * R
    for t in range(3):
        rng = np.random.RandomState(t)
        z = [rng.uniform(-6, -1, (R, ldl)).astype(np.float32) for _ in range(2)]
        lse = [rng.uniform(2, 5, R).astype(np.float32) for _ in range(2)]
        for r in range(R):
            for m in range(2):
                z[m][r, arg[t][r]] = 6.0 + m
                z[m][r, Vv:] = ec.PAD
        e = ec.reference(z, lse, np.float32(logw), Vv)
        out = C.vocab_select(*[torch.empty(0, device=DEV)] * 4, 1, 1.0, 0,
                             ens_logits=[torch.from_numpy(x).to(DEV) for x in z],
                             ens_lse=[torch.from_numpy(x).to(DEV) for x in lse],
                             ens_logw=logw, ens_V=Vv, ens_K=1, ens_unfinished=unf)
        top_v, top_i, tok, lp, nxt = [x.cpu().numpy() for x in out]
        assert top_i[:, 0].tolist() == arg[t]
        for r in range(R):
            was = alive[r]
            alive[r] = was and arg[t][r] > 0
            assert tok[r] == nxt[r] == (arg[t][r] if was else 0)
            if was:
                assert abs(lp[r] - e[r, arg[t][r]]) <= ec.bound(12.0, 2)
            else:
                assert lp[r] == 0.0
        assert unf.cpu().tolist() == [int(a) for a in alive]
    assert alive == [False, False, True, False]


# -- one member: the orchestration, bit for bit ---------------------------------------------
@gpu
@pytest.mark.parametrize('kind', [dict(), dict(layers=2), dict(model_type='standard')],
                         ids=['concat', 'two_layers', 'standard'])
def test_one_member_decode_is_bit_equal_to_the_engine(kind):
    from cst_captioning_amd.models.decoder_engine import EnsembleEngine
    from cst_captioning_amd.models.ensemble import EnsembleCaptionModel
    model, eng = _member('lstm', 64, 3, DEV, **kind)
    feats = _feats(DEV)
    ens = EnsembleCaptionModel([model])
    EnsembleEngine(ens, [eng])
    with torch.no_grad():
        seq, lp = eng.sample_beam(model, feats, {'beam_size': 9})  # (K > 8: the dense path)
        eseq, elp = ens.sample_beam(feats, {'beam_size': 9})
    assert seq.shape == (B, L) and (seq != 0).any()
    assert torch.equal(seq, eseq) and torch.equal(lp, elp)


# -- several members ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('K', [1, 3, 9])
@pytest.mark.parametrize('spec', ENSEMBLES, ids=[s[0] for s in ENSEMBLES])
def test_ensemble_decode_matches_torch_and_itself(spec, K):
    from cst_captioning_amd.utils.text import BOS
    ens, engs = _ensemble(spec, DEV)
    twin = _bf16_twin(ens)
    feats = _feats(DEV, spec[3])
    with torch.no_grad():
        got = _decode(ens, feats, K)
        again = _decode(ens, feats, K)
        want = _decode(twin, feats, K)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    frac, err = _agreement(got, want, K == 1)
    print('%s K=%d: %.2f of the rows identical, max log-prob difference %.4f' %
          (spec[0], K, frac, err))
    assert frac >= 0.8, (got[0], want[0])
    assert err < 0.05
    # self-consistency: every member's engine teacher-forced on the returned
    # sequence, mixed in fp64
    seq, lp = got
    labels = torch.cat([torch.full_like(seq[:, :1], BOS), seq, torch.zeros_like(seq[:, :1])], 1)
    with torch.no_grad():
        dense = [e.forward_full(m, feats, labels)[0].double()
                 for m, e in zip(ens.members, engs)]
    mix = torch.logsumexp(torch.stack([d + lw for d, lw in zip(dense, ens.log_weights)]), 0)
    n = seq.size(1)
    tf = mix[:, :n].gather(2, seq.unsqueeze(2)).squeeze(2)
    # greedy: up to the row's first 0; beam: the positions the winning beam
    # wrote (it may go on after a 0; unwritten positions hold exactly 0)
    live = _live(seq) if K == 1 else lp != 0
    assert live.any(1).all()
    d = ((tf - lp.double()).abs() * live).max().item()
    print('self-consistency: max |lp - teacher-forced mixture| = %.4f' % d)
    assert d < 0.05
    if K == 1:
        gap = ((mix[:, :n].max(2).values - tf) * live).max().item()
        print('greedy: max (row maximum - chosen) = %.4f' % gap)
        assert gap < 0.1
        assert (lp[~live] == 0).all() and (seq[~live] == 0).all()


# -- refusals -------------------------------------------------------------------------------------
@gpu
def test_refusals_before_any_launch():
    from cst_captioning_amd import _ext
    from cst_captioning_amd.utils.text import BOS
    C = _ext.ops()
    model, eng = _member('lstm', 64, 5, DEV)
    feats = _feats(DEV)
    vg, blog, att, state0 = eng._decode_operands(model, feats)

    def pack(wlog=eng.wlog, blog=blog, vg=vg, att=()):
        m = torch.tensor([eng.cell, len(att), 0, 0])
        return [eng.wx, eng.ptab, eng.whh, wlog, blog, vg, m] + list(att)

    def run(K=3, ensemble=(), w=None, wlog=eng.wlog, b=blog, att=(), greedy=False):
        w = [math.log(1.0 / (1 + len(ensemble)))] * (1 + len(ensemble)) if w is None else w
        return C.beam_search(eng.wx, eng.ptab, eng.whh, wlog, b, vg, K, L, BOS, list(att),
                             eng.cell, [], [], ensemble=list(ensemble), ens_weights=w,
                             ens_greedy=greedy)

    torch.cuda.synchronize()
    assert run(ensemble=[pack()])[0].shape == (B, L)  # the operands themselves are fine
    with pytest.raises(RuntimeError, match='members'):
        run(ensemble=[pack()] * 8)                                  # M = 9
    with pytest.raises(RuntimeError, match='beam_size'):
        run(K=17, ensemble=[pack()])
    with pytest.raises(RuntimeError, match='vocab_size'):             # K > V
        run(K=12, ensemble=[pack(eng.wlog[:10], blog[:10])], wlog=eng.wlog[:10], b=blog[:10])
    with pytest.raises(RuntimeError, match='vocab_size'):             # members differ in V
        run(ensemble=[pack(eng.wlog[:100], blog[:100])])
    with pytest.raises(RuntimeError, match='videos'):                 # ... in B
        run(ensemble=[pack(vg=vg[:3])])
    H4, A = 4 * eng.H, 64

    def fake_att(Cn):
        f = lambda *s: torch.zeros(*s, device=DEV)
        return [f(B, Cn, H4), f(B, Cn, A), torch.zeros(A, eng.H, device=DEV, dtype=torch.bfloat16),
                f(A), f(1)]
    with pytest.raises(RuntimeError, match='frames'):                 # ... in attention frames
        run(ensemble=[pack(att=fake_att(3))], att=fake_att(2))
    for bad in (float('nan'), float('inf'), -float('inf')):
        with pytest.raises(RuntimeError, match='log-weight'):
            run(ensemble=[pack()], w=[math.log(0.5), bad])
    with pytest.raises(RuntimeError, match='log-weights'):
        run(ensemble=[pack()], w=[0.0])
    with pytest.raises(RuntimeError):                                 # packs without weights
        C.beam_search(eng.wx, eng.ptab, eng.whh, eng.wlog, blog, vg, 3, L, BOS, [], eng.cell, [],
                      [], ensemble=[pack()])
    # the kernel's test route
    case = CASES[2]
    z = [torch.from_numpy(x).to(DEV) for x in case['logits']]
    ls = [torch.from_numpy(x).to(DEV) for x in case['lse']]
    e = torch.empty(0, device=DEV)
    sel = lambda **kw: C.vocab_select(e, e, e, e, 1, 1.0, 0, **kw)
    for kw in (dict(ens_logits=z * 5, ens_lse=ls * 5, ens_logw=[0.0] * 10, ens_V=259, ens_K=2),
               dict(ens_logits=z, ens_lse=ls, ens_logw=[0.0, 0.0], ens_V=259, ens_K=17),
               dict(ens_logits=z, ens_lse=ls, ens_logw=[0.0, 0.0], ens_V=5, ens_K=6),
               dict(ens_logits=z, ens_lse=ls, ens_logw=[0.0, float('nan')], ens_V=259, ens_K=2),
               dict(ens_logits=z, ens_lse=ls, ens_logw=[0.0, 0.0], ens_V=270, ens_K=2)):
        with pytest.raises(RuntimeError):
            sel(**kw)
    torch.cuda.synchronize()


# -- Trainer.test ---------------------------------------------------------------------------------
@gpu
def test_trainer_test_with_an_ensemble_tokens_and_strings():
    from cst_captioning_amd.cli import build_model
    from cst_captioning_amd.config import default_opts
    from cst_captioning_amd.data import CaptionLoader, make_synthetic
    from cst_captioning_amd.models.decoder_engine import EnsembleEngine
    from cst_captioning_amd.models.ensemble import EnsembleCaptionModel
    from cst_captioning_amd.parallel import DistContext
    from cst_captioning_amd.train.trainer import Trainer
    ds = make_synthetic('msrvtt', num_videos=24, vocab_size=V, seq_length=L, feat_dims=DIMS, seed=0)
    dev = torch.device(DEV)
    out = {}
    for scorer in ('tokens', 'strings'):
        members, engines = [], []
        for i, (cell, H) in enumerate([('lstm', 64), ('gru', 128)]):
            opt = default_opts(batch_size=8, train_seq_per_img=5, test_batch_size=10,
                               test_seq_per_img=5, rnn_size=H, input_encoding_size=H, beam_size=3,
                               impl='hip', drop_prob_lm=0.5, val_scorer=scorer, rnn_type=cell,
                               vocab_size=ds.vocab_size, seq_length=ds.seq_length,
                               feat_dims=ds.feat_dims)
            opt.vocab = {j: w for j, w in enumerate(ds.vocab)}
            torch.manual_seed(20 + i)
            m, e = build_model(opt, dev, 'hip')
            assert e is not None
            members.append(m)
            engines.append(e)
            if i == 0:
                opt0 = opt
        loader = CaptionLoader(ds, 10, 5, 'test', dev)
        tr = Trainer(opt0, members[0], loader, None, DistContext(device=dev), engines[0])
        assert tr.ensemble is None
        single = tr.test(loader)
        tr.ensemble = EnsembleCaptionModel([m.eval() for m in members], [0.5, 0.5])
        EnsembleEngine(tr.ensemble, engines)
        out[scorer] = tr.test(loader)
        assert {'Bleu_4', 'CIDEr', 'ROUGE_L', 'METEOR', 'Loss'} <= set(out[scorer]['scores'])
        assert np.isfinite(out[scorer]['scores']['Loss'])
        assert out[scorer]['scores']['Loss'] != single['scores']['Loss']
    assert out['tokens']['predictions'] == out['strings']['predictions']
    assert len(out['tokens']['predictions']) == 24
