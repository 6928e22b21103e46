"""Ensemble decoding: several trained :class:`CaptionModel` s average their
per-step word distributions at test time.

With ``lp_m`` member ``m``'s ``log_softmax`` output for a row and ``w`` the
normalised weights, every step decodes under

    ``lp_ens[v] = logsumexp_m(log w_m + lp_m[v])``

the log of the weighted arithmetic mean of the members' probabilities.  The
members may differ in ``rnn_type``, ``model_type``, ``rnn_size``,
``num_layers`` and ``input_encoding_size``; they share the vocabulary (the
same word list), ``seq_length``, ``feat_dims`` and ``num_chunks``, and read the
same ``feats``.  Each member keeps its own recurrent state and receives the
same token; beam search applies one parent re-indexing to every member.

The loops here are those of :meth:`CaptionModel.sample` (greedy) and
:meth:`CaptionModel.sample_beam` with ``logprobs`` replaced by ``lp_ens``; with
one member every output is bit-equal to the member's own (the single value is
taken without a logsumexp round trip).  On the GPU the same decode runs on the
members' fused engines (:class:`EnsembleEngine`, ``csrc/beam_search.cpp``
``ensemble_decode`` and ``csrc/kernels/ensemble.hip``).  Sampling from an
ensemble (``sample_max = 0``, ``decode = 'mbr'``, ``top_k`` / ``top_p``) is not
provided.
"""
import logging
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

logger = logging.getLogger(__name__)

MAX_MEMBERS = 8  # csrc/launchers.h ENS_MAXM
SHARED_FIELDS = ('vocab', 'seq_length', 'feat_dims', 'num_chunks')


def normalise_weights(weights, n):
    """``n`` positive finite weights (None: uniform) normalised to sum 1, as a
    list of floats; ValueError otherwise."""
    if weights is None:
        return [1.0 / n] * n
    w = [float(x) for x in weights]
    if len(w) != n:
        raise ValueError('%d ensemble weights for %d members' % (len(w), n))
    for x in w:
        if not (math.isfinite(x) and x > 0.0):
            raise ValueError('ensemble weights must be positive and finite, got %r' % (x,))
    tot = math.fsum(w)
    return [x / tot for x in w]


def field_mismatch(a, b):
    """The first of the fields the members of an ensemble must share in which
    two option namespaces differ (``vocab`` compared as the word list), or
    None."""
    for k in SHARED_FIELDS:
        va, vb = getattr(a, k, None), getattr(b, k, None)
        if k == 'vocab':
            if va is None and vb is None:
                continue
            same = va is not None and vb is not None and \
                {str(i): w for i, w in dict(va).items()} == {str(i): w for i, w in dict(vb).items()}
        elif k == 'feat_dims':
            same = list(va or []) == list(vb or [])
        elif k == 'num_chunks':
            same = (va or 1) == (vb or 1)
        else:
            same = va == vb
        if not same:
            return k
    return None


def mix_logprobs(lps, logw):
    """``logsumexp_m(logw[m] + lps[m])`` over a list of same-shaped log-prob
    tensors; one member: the tensor itself."""
    if len(lps) == 1:
        return lps[0]
    return torch.logsumexp(torch.stack([lp.float() + lw for lp, lw in zip(lps, logw)], 0), 0)


class EnsembleCaptionModel(nn.Module):

    def __init__(self, members, weights=None, vocabs=None):
        """``members``: 1 to 8 :class:`CaptionModel` s; ``weights``: positive
        finite numbers, one per member (default uniform); ``vocabs``: the
        members' word lists (``{index: word}``), compared when given -- a
        model itself only knows its vocabulary's size."""
        super().__init__()
        members = list(members)
        if not 1 <= len(members) <= MAX_MEMBERS:
            raise ValueError('an ensemble has 1 to %d members, got %d' % (MAX_MEMBERS, len(members)))
        m0 = members[0]
        for i, m in enumerate(members[1:], 1):
            for k in ('vocab_size', 'seq_length', 'feat_dims', 'num_chunks'):
                if getattr(m, k) != getattr(m0, k):
                    raise ValueError('ensemble member %d differs from member 0 in %s: %r vs %r'
                                     % (i, k, getattr(m, k), getattr(m0, k)))
        if vocabs is not None:
            vocabs = [{str(i): w for i, w in dict(v).items()} for v in vocabs]
            if len(vocabs) != len(members):
                raise ValueError('one vocabulary per ensemble member')
            for i, v in enumerate(vocabs[1:], 1):
                if v != vocabs[0]:
                    raise ValueError('ensemble member %d differs from member 0 in vocab (the word '
                                     'lists differ)' % i)
        self.members = nn.ModuleList(members)
        self.weights = normalise_weights(weights, len(members))
        self.log_weights = [math.log(w) for w in self.weights]
        self.vocab_size = m0.vocab_size
        self.seq_length = m0.seq_length
        self.feat_dims = list(m0.feat_dims)
        self.num_chunks = m0.num_chunks
        self.bos_index = m0.bos_index
        self._engine = None  # EnsembleEngine, attached by its constructor

    # -- the members' steps ----------------------------------------------------
    def _mix(self, lps):
        return mix_logprobs(lps, self.log_weights)

    @staticmethod
    def _check_decode(opt):
        if opt.get('decode', 'standard') == 'mbr':
            raise ValueError("an ensemble does not decode with decode = 'mbr'")
        if opt.get('sample_max', 1) != 1:
            raise ValueError('an ensemble decodes greedily or by beam search (sample_max = 1)')
        if opt.get('top_k', 0) or opt.get('top_p', 1.0) != 1.0:
            raise ValueError('an ensemble does not sample: top_k / top_p are not supported')

    def forward(self, feats, seq):
        """``(lp_ens (N, T, V), seq, lp_ens of seq)`` from the members'
        teacher-forced passes."""
        outs = [m(feats, seq) for m in self.members]
        if len(outs) == 1:
            return outs[0]
        n = min(o[0].size(1) for o in outs)  # (a member may stop early on all-EOS inputs)
        dense = self._mix([o[0][:, :n] for o in outs])
        s_seq = outs[0][1][:, :max(n - 1, 0)]
        s_lp = dense[:, :s_seq.size(1)].gather(2, s_seq.unsqueeze(2)).squeeze(2)
        return dense, s_seq, s_lp

    # -- greedy decoding -------------------------------------------------------
    def sample(self, feats, opt={}):
        self._check_decode(opt)
        if opt.get('beam_size', 1) > 1:
            return self.sample_beam(feats, opt)
        if self._engine is not None:
            return self._engine.sample(feats, opt)
        ms = list(self.members)
        if len(ms) == 1:
            return ms[0].sample(feats, opt)
        ctxs = []
        for m in ms:
            ctx = m._video_ctx(m.encode(feats))
            if opt.get('expand_feat', 0) == 1:
                ctx = m._expand_ctx(ctx, m.feat_expander.n)
            ctxs.append(ctx)
        n = next(iter(ctxs[0].values())).size(0)
        dev = next(self.parameters()).device
        states = [m.init_hidden(n) for m in ms]
        for i, m in enumerate(ms):  # 'standard': the video vector is the input of step -1
            if m.model_type == 'standard':
                _, states[i] = m._step(m._first_input(ctxs[i]), ctxs[i], states[i])
        seq, seq_lp = [], []
        unfinished = None
        logprobs = None
        for t in range(0, self.seq_length - 1):
            if t == 0:
                it = torch.full((n,), self.bos_index, dtype=torch.long, device=dev)
            else:
                lp_t, it = torch.max(logprobs.detach(), 1)
            it_in = it
            if t >= 1:
                unfinished = (it > 0) if unfinished is None else unfinished & (it > 0)
                it = it * unfinished
                seq.append(it)
                seq_lp.append(lp_t.view(-1))
                if int(unfinished.sum()) == 0:
                    break
            lps = []
            for i, m in enumerate(ms):
                out, states[i] = m._step(m.embed(it_in), ctxs[i], states[i])
                lps.append(F.log_softmax(m.logit(out), dim=-1))
            logprobs = self._mix(lps)
        return torch.stack(seq, 1), torch.stack(seq_lp, 1)

    # -- beam search -------------------------------------------------------------
    def sample_beam(self, feats, opt={}):
        self._check_decode(opt)
        if self._engine is not None:
            return self._engine.sample_beam(feats, opt)
        ms = list(self.members)
        if len(ms) == 1:
            return ms[0].sample_beam(feats, opt)
        K = opt.get('beam_size', 5)
        V, T = self.vocab_size, self.seq_length
        if K > V:
            raise ValueError('beam_size > vocab_size')
        ctx0 = [m._video_ctx(m.encode(feats)) for m in ms]
        B = next(iter(ctx0[0].values())).size(0)
        dev = next(self.parameters()).device
        ctxs = [m._expand_ctx(c, K) for m, c in zip(ms, ctx0)]
        states = [m.init_hidden(B * K) for m in ms]
        for i, m in enumerate(ms):
            if m.model_type == 'standard':
                _, states[i] = m._step(m._first_input(ctxs[i]), ctxs[i], states[i])
        beam_seq = torch.zeros(B, K, T, dtype=torch.long, device=dev)
        beam_lp = torch.zeros(B, K, T, device=dev)
        beam_sum = torch.zeros(B, K, device=dev)
        best_ppl = torch.full((B,), math.inf, device=dev)
        best_seq = torch.zeros(B, T, dtype=torch.long, device=dev)
        best_lp = torch.zeros(B, T, device=dev)
        bidx = torch.arange(B, device=dev)[:, None]
        logprobs = None
        for t in range(0, T - 1):
            if t == 0:
                tok_in = torch.full((B * K,), self.bos_index, dtype=torch.long, device=dev)
            else:
                lp = logprobs.float().view(B, K, V)
                ys, ix = lp.topk(K, dim=2)  # per beam, best words first
                rows = 1 if t == 1 else K
                # reference candidate order: for c (word rank): for q (beam)
                cand_p = (beam_sum[:, :rows, None] + ys[:, :rows, :]).transpose(1, 2)
                cand_p = cand_p.reshape(B, K * rows)
                order = torch.sort(cand_p, dim=1, descending=True, stable=True).indices[:, :K]
                q = order % rows
                c = order // rows
                tok = ix[bidx, q, c]
                raw = ys[bidx, q, c]
                beam_sum = cand_p.gather(1, order)
                beam_seq = beam_seq[bidx, q]
                beam_lp = beam_lp[bidx, q]
                beam_seq[:, :, t - 1] = tok
                beam_lp[:, :, t - 1] = raw
                src = (bidx * K + q).reshape(-1)
                # the parent re-indexing, applied to every member's state
                states = [tuple(s[:, src] for s in st) if isinstance(st, tuple) else st[:, src]
                          for st in states]
                done = (tok == 0) | (t == T - 2)
                ppl = torch.exp(-beam_sum / (t - 1)) if t > 1 else \
                    torch.full_like(beam_sum, 10000.0)
                for v in range(K):  # harvest in the reference's order (earliest wins ties)
                    upd = done[:, v] & (ppl[:, v] < best_ppl)
                    best_ppl = torch.where(upd, ppl[:, v], best_ppl)
                    best_seq = torch.where(upd[:, None], beam_seq[:, v], best_seq)
                    best_lp = torch.where(upd[:, None], beam_lp[:, v], best_lp)
                tok_in = tok.reshape(-1)
            lps = []
            for i, m in enumerate(ms):
                out, states[i] = m._step(m.embed(tok_in), ctxs[i], states[i])
                lps.append(F.log_softmax(m.logit(out), dim=-1))
            logprobs = self._mix(lps)
        return best_seq, best_lp

