"""Worker for tests/test_corpus_metrics_dist.py, launched by torchrun (gloo on
the CPU): a sharded validation with ``--val_scorer tokens``.  Writes rank 0's
result to ``argv[1]`` (torch.save)."""
import sys

import torch

from cst_captioning_amd.parallel import init_distributed
from cst_captioning_amd.train.trainer import Trainer
import dist_worker


def main(out):
    dist_worker.ARGS[dist_worker.ARGS.index('--language_eval') + 1] = '1'
    dist_worker.ARGS += ['--val_scorer', 'tokens']
    ctx = init_distributed()
    opt, model, engine, loader, val = dist_worker.build(ctx.rank, ctx.world_size, ctx.device)
    tr = Trainer(opt, model, loader, val, ctx, engine)
    res = tr.validate(val)
    rows = ctx.all_gather_object((res['sequences'], res['video_index']))
    if ctx.is_main:
        torch.save({'scores': res['scores'], 'predictions': res['predictions'],
                    'rows': rows, 'world': ctx.world_size}, out)
    ctx.destroy()


if __name__ == '__main__':
    main(sys.argv[1])
