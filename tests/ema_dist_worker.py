"""Worker for tests/test_ema.py, launched by torchrun (gloo on CPU): three XE
steps with ``--dp_update sharded --ema_decay 0.5``, then the parameters seen
inside ``Trainer.ema_weights()`` and this rank's shards before / after it.
Rank 0 writes every rank's results to ``argv[1]`` (torch.save)."""
import sys

import torch

from cst_captioning_amd.cli import build_model, load_splits
from cst_captioning_amd.config import parse_opts
from cst_captioning_amd.data import CaptionLoader
from cst_captioning_amd.parallel import init_distributed
from cst_captioning_amd.train.trainer import Trainer

ARGS = ['--synthetic', 'msvd', '--synthetic_videos', '24', '--synthetic_vocab', '200',
        '--seq_length', '8', '--rnn_size', '64', '--input_encoding_size', '64',
        '--feat_dims', '16', '8', '--batch_size', '4', '--train_seq_per_img', '3',
        '--test_batch_size', '3', '--test_seq_per_img', '3', '--impl', 'torch',
        '--loglevel', 'WARNING', '--drop_prob_lm', '0', '--learning_rate', '1e-3',
        '--language_eval', '0', '--dp_update', 'sharded', '--ema_decay', '0.5']


def main(out):
    ctx = init_distributed()
    opt = parse_opts(ARGS)
    torch.manual_seed(1234 + ctx.rank)
    tr_ds, _, _ = load_splits(opt)
    loader = CaptionLoader(tr_ds, opt.batch_size, opt.train_seq_per_img, 'train', ctx.device,
                           ctx.rank, ctx.world_size, opt.seed)
    opt.vocab, opt.vocab_size = loader.get_vocab(), loader.get_vocab_size()
    opt.seq_length, opt.feat_dims = loader.get_seq_length(), loader.get_feat_dims()
    model, engine = build_model(opt, ctx.device)
    tr = Trainer(opt, model, loader, None, ctx, engine)  # (rank 0's weights are broadcast)
    assert tr.bucket.sharded and tr.optimizer.ema is not None
    init = tr.bucket.data.detach().clone()
    assert torch.equal(tr.optimizer.ema, init)
    grad_sums = []
    for _ in range(3):
        tr.train_step(loader.get_batch(), 0)
        # (the reduce-scatter leaves the local gradient in the bucket)
        gs = ctx.all_gather_object(tr.bucket.grad.detach().clone())
        grad_sums.append(gs[0] + gs[1])
    lo, hi = tr.bucket.shard_range(ctx.rank)
    mine = {'live_before': tr.bucket.data.detach().clone(),
            'p_shard_before': tr.bucket.data[lo:hi].detach().clone(),
            'e_shard_before': tr.optimizer.ema[lo:hi].detach().clone()}
    with tr.ema_weights():
        mine['inside'] = tr.bucket.data.detach().clone()
    mine['live_after'] = tr.bucket.data.detach().clone()
    mine['p_shard_after'] = tr.bucket.data[lo:hi].detach().clone()
    mine['e_shard_after'] = tr.optimizer.ema[lo:hi].detach().clone()
    ranks = ctx.all_gather_object(mine)
    if ctx.is_main:
        torch.save({'ranks': ranks, 'init': init, 'numel': tr.bucket.numel,
                    'grad_sums': grad_sums, 'lr': opt.learning_rate,
                    'grad_clip': opt.grad_clip, 'ema_decay': opt.ema_decay}, out)
    ctx.destroy()


if __name__ == '__main__':
    main(sys.argv[1])
