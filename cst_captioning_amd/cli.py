"""Command-line entry points: ``train`` and ``test``.

Same flags and flow as ``/root/reference/train.py:421-519`` and
``/root/reference/test.py:22-77``; one process per GPU under torchrun for
data parallelism (``torchrun --nproc-per-node N -m cst_captioning_amd.cli train ...``).
"""
import json
import logging
import os
import sys
from datetime import datetime

import numpy as np
import torch

from .config import parse_opts
from .data import CaptionLoader, VideoCaptionDataset, make_splits
from .models import CaptionModel
from .parallel import init_distributed

logger = logging.getLogger('cst_captioning_amd')


def setup_logging(opt, rank=0):
    level = getattr(logging, opt.loglevel.upper()) if rank == 0 else logging.WARNING
    logging.basicConfig(level=level, format='%(asctime)s:%(levelname)s: %(message)s')


def seed_everything(seed, rank=0):
    np.random.seed(seed + rank)
    torch.manual_seed(seed + rank)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed + rank)


def load_splits(opt):
    tokens = getattr(opt, 'consensus_scorer', 'file') == 'tokens'
    if tokens and opt.train_bcmrscores_pkl:
        raise ValueError('--consensus_scorer tokens computes the consensus scores itself; '
                         '--train_bcmrscores_pkl must not be given with it')
    if getattr(opt, 'reward_mix', ''):
        from .ops.reward_mix import check_consensus_route
        check_consensus_route(opt)
    if opt.synthetic:
        n = opt.synthetic_videos or None
        return make_splits(opt.synthetic, vocab_size=opt.synthetic_vocab,
                           seq_length=opt.seq_length, feat_dims=opt.feat_dims,
                           num_chunks=opt.num_chunks, train_videos=n, seed=opt.seed,
                           # (--consensus_scorer tokens: the trainer computes them)
                           with_consensus=not tokens and (
                               bool(opt.use_cst and opt.scb_baseline == 1) or
                               bool(opt.use_cst and not opt.use_mixer)),
                           seq_per_img=opt.train_seq_per_img)
    df = opt.train_cached_tokens if isinstance(opt.train_cached_tokens, str) else None
    tr = VideoCaptionDataset.from_files(opt.train_label_h5, opt.train_feat_h5, opt.num_chunks,
                                        opt.train_bcmrscores_pkl, opt.eval_metric,
                                        opt.train_cocofmt_file, df)
    va = VideoCaptionDataset.from_files(opt.val_label_h5, opt.val_feat_h5, opt.num_chunks,
                                        cocofmt_file=opt.val_cocofmt_file) \
        if opt.val_label_h5 else None
    te = VideoCaptionDataset.from_files(opt.test_label_h5, opt.test_feat_h5, opt.num_chunks,
                                        cocofmt_file=opt.test_cocofmt_file) \
        if opt.test_label_h5 else None
    return tr, va, te


def build_model(opt, device, impl=None):
    model = CaptionModel(opt).to(device)
    impl = impl or opt.impl
    engine = None
    if impl == 'auto':
        impl = 'hip' if device.type == 'cuda' else 'torch'
    if impl == 'hip' and getattr(opt, 'precision', 'bf16') == 'fp32':
        # the fused engine computes with bf16 MFMA operands; fp32 means the
        # plain PyTorch path
        logger.warning('--precision fp32: using the PyTorch decoder path (the HIP engine is bf16)')
        return model, None
    if impl == 'hip':
        from .models.decoder_engine import DecoderEngine, engine_unsupported_reason
        why = engine_unsupported_reason(opt)
        if why is not None:
            # (the engine covers lstm / gru / rnn cells, concat / standard /
            # manet models, up to 5 stacked layers and temporal attention)
            logger.warning('fused HIP decoder: %s; using the PyTorch decoder path', why)
            return model, None
        engine = DecoderEngine(model, opt)
        model.impl = 'hip'
        model._engine = engine
    return model, engine


def train_main(argv=None):
    opt = parse_opts(argv)
    ctx = init_distributed()
    setup_logging(opt, ctx.rank)
    logger.info('Input arguments: %s', json.dumps(vars(opt), sort_keys=True, indent=4,
                                                 default=str))
    seed_everything(opt.seed, ctx.rank)
    tr, va, te = load_splits(opt)
    dev = ctx.device
    train_loader = CaptionLoader(tr, opt.batch_size, opt.train_seq_per_img, 'train', dev,
                                 ctx.rank, ctx.world_size, opt.seed)
    val_loader = CaptionLoader(va, opt.test_batch_size, opt.test_seq_per_img, 'test', dev) \
        if va is not None else None
    test_loader = CaptionLoader(te, opt.test_batch_size, opt.test_seq_per_img, 'test', dev) \
        if te is not None else None
    opt.vocab = train_loader.get_vocab()
    opt.vocab_size = train_loader.get_vocab_size()
    opt.seq_length = train_loader.get_seq_length()
    opt.feat_dims = train_loader.get_feat_dims()
    if opt.model_file:
        opt.history_file = opt.model_file.replace('.pth', '_history.json', 1)
        d = os.path.dirname(opt.model_file)
        if d:
            os.makedirs(d, exist_ok=True)
    logger.info('Building model...')
    model, engine = build_model(opt, dev)
    from .train.trainer import Trainer
    trainer = Trainer(opt, model, train_loader, val_loader, ctx, engine)
    if opt.result_file:  # (--val_scorer tokens: refuse an unscorable test split before training)
        trainer.check_val_scorer(test_loader)
    start = datetime.now()
    infos = trainer.train()
    logger.info('Best val %s score: %f. Best iter: %d. Best epoch: %d', opt.eval_metric,
                infos['best_score'], infos['best_iter'], infos['best_epoch'])
    logger.info('Training time: %s', datetime.now() - start)
    if opt.result_file and test_loader is not None:
        from .train.checkpoint import load_checkpoint
        if opt.model_file and os.path.exists(opt.model_file):
            model.load_state_dict(load_checkpoint(opt.model_file, dev)['model'])
            if engine is not None:
                engine.refresh_weights()
        trainer.test(test_loader)
    ctx.destroy()
    return infos


def _mbr_needs_df(opt):
    """--decode mbr: whether the utility has a CIDEr-D term (--mbr_mix empty: CIDEr-D)."""
    mix = getattr(opt, 'mbr_mix', '') or ''
    if not mix:
        return True
    from .ops.reward_mix import parse_reward_mix
    return parse_reward_mix(mix, '--mbr_mix')[0] != 0


MEMBER_FIELDS = ('model_type', 'rnn_type', 'rnn_size', 'num_layers', 'input_encoding_size')


def load_ensemble_members(opt, copt):
    """--ensemble_files, checked before any model is built: ``[(file, checkpoint,
    options)]`` of members 1..M-1, each member's options = ``opt`` with the
    model's type, sizes and cell from its own checkpoint.  ``copt``: member
    0's checkpoint options.  ValueError on a wrong weight count, more than 8
    members, --decode mbr, or a member whose vocab, seq_length, feat_dims or
    num_chunks differs (naming the file and the field)."""
    import copy
    from .models.ensemble import MAX_MEMBERS, field_mismatch
    from .train.checkpoint import load_checkpoint
    files = list(opt.ensemble_files)
    M = 1 + len(files)
    if opt.decode == 'mbr':
        raise ValueError('--ensemble_files does not go with --decode mbr (an ensemble decodes '
                         'greedily or by beam search)')
    if M > MAX_MEMBERS:
        raise ValueError('--ensemble_files: %d members, at most %d (--model_file included)'
                         % (M, MAX_MEMBERS))
    if opt.ensemble_weights and len(opt.ensemble_weights) != M:
        raise ValueError('--ensemble_weights: %d weights for %d members (--model_file first)'
                         % (len(opt.ensemble_weights), M))
    ref = copy.copy(copt)
    ref.num_chunks = opt.num_chunks  # (member 0 decodes with the command's --num_chunks)
    out = []
    for f in files:
        ck = load_checkpoint(f, 'cpu')
        why = field_mismatch(ref, ck['opt'])
        if why is not None:
            raise ValueError('--ensemble_files %s: %s differs from --model_file\'s' % (f, why))
        mopt = copy.copy(opt)
        for k in MEMBER_FIELDS:
            if hasattr(ck['opt'], k):
                setattr(mopt, k, getattr(ck['opt'], k))
        out.append((f, ck, mopt))
    return out


def test_main(argv=None):
    opt = parse_opts(argv)
    ctx = init_distributed()
    setup_logging(opt, ctx.rank)
    # --mbr_mix without CIDEr reads no df table: none is asked for
    mbr_df = opt.decode == 'mbr' and _mbr_needs_df(opt)
    if mbr_df and not opt.synthetic:
        # consensus decoding scores under the TRAINING set's df table (the
        # synthetic split carries its own); refused here, before the model is built
        if not isinstance(opt.train_cached_tokens, str):
            raise ValueError('--decode mbr needs the CIDEr-D document-frequency table of the '
                             'training set: --train_cached_tokens')
        from .prepro.ciderdf import load_packed_df
        opt.mbr_df = load_packed_df(opt.train_cached_tokens)
    from .train.checkpoint import load_checkpoint
    ck = load_checkpoint(opt.model_file, 'cpu')
    copt = ck['opt']
    for k in ('model_type', 'vocab', 'vocab_size', 'seq_length', 'feat_dims'):
        setattr(opt, k, getattr(copt, k))
    others = load_ensemble_members(opt, copt) if opt.ensemble_files else []
    if opt.synthetic:
        _, _, te = load_splits(opt)
    else:
        te = VideoCaptionDataset.from_files(opt.test_label_h5, opt.test_feat_h5,
                                            opt.num_chunks,
                                            cocofmt_file=opt.test_cocofmt_file)
    loader = CaptionLoader(te, opt.test_batch_size, opt.test_seq_per_img, 'test', ctx.device)
    from .train.trainer import Trainer, check_val_scorer
    check_val_scorer(opt, loader)
    if mbr_df and opt.synthetic and te.df is None:
        raise ValueError('--decode mbr needs a CIDEr-D document-frequency table; the '
                         'synthetic split has none')
    assert opt.vocab_size == loader.get_vocab_size()
    assert opt.seq_length == loader.get_seq_length()
    assert list(opt.feat_dims) == list(loader.get_feat_dims())
    model, engine = build_model(opt, ctx.device)
    model.load_state_dict(ck['model'])
    if engine is not None:
        engine.refresh_weights()
    trainer = Trainer(opt, model, loader, None, ctx, engine)
    if opt.ensemble_files:
        trainer.ensemble = build_ensemble(opt, ctx.device, model, engine, others)
    res = trainer.test(loader)
    ctx.destroy()
    return res


def build_ensemble(opt, device, model, engine, others):
    """The EnsembleCaptionModel of --ensemble_files around member 0 (``model``,
    ``engine``): the other members built from their own checkpoints' options.
    On the fused engine when every member runs on it; else the whole ensemble
    decodes through the PyTorch path (logged once)."""
    from .models.ensemble import EnsembleCaptionModel
    members, engines = [model], [engine]
    for f, ck, mopt in others:
        m, e = build_model(mopt, device)
        m.load_state_dict(ck['model'])
        if e is not None:
            e.refresh_weights()
        members.append(m)
        engines.append(e)
    for m in members:
        m.eval()
    ens = EnsembleCaptionModel(members, opt.ensemble_weights or None)
    if all(e is not None for e in engines):
        from .models.decoder_engine import EnsembleEngine
        EnsembleEngine(ens, engines)
    elif any(e is not None for e in engines):
        logger.warning('ensemble: a member does not run on the fused HIP decoder; the whole '
                       'ensemble decodes through the PyTorch path')
        for m in members:
            m.impl = 'torch'
    logger.info('Ensemble of %d members, weights %s', len(members),
                ' '.join('%.4g' % w for w in ens.weights))
    return ens


def main():
    if len(sys.argv) < 2 or sys.argv[1] not in ('train', 'test'):
        print('usage: python -m cst_captioning_amd.cli {train,test} [flags]')
        sys.exit(2)
    cmd = sys.argv.pop(1)
    (train_main if cmd == 'train' else test_main)()


if __name__ == '__main__':
    main()
