"""Greedy, beam and consensus (MBR) decoding compared on the learnable template
task (``data/synthetic.py`` ``caption_mode='template'``) after a short XE run on
the fused engine: mean validation CIDEr-D (the reward kernel against the
validation split's references, train-split document frequencies, x10) of the
captions each decoder returns.  Information only: a synthetic task.

usage: python scripts/mbr_quality.py [XE_STEPS] [MBR_SAMPLES] [TOP_K] [TOP_P]

TOP_K >= 1 adds, beside every consensus row, the same decode with its samples
truncated to the TOP_K most probable words and the nucleus TOP_P inside them
(``--mbr_top_k`` / ``--mbr_top_p``; default 0 / 1.0: not run).

Prints one JSON line.
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cst_captioning_amd.cli import build_model  # noqa: E402
from cst_captioning_amd.config import default_opts  # noqa: E402
from cst_captioning_amd.data import CaptionLoader, make_splits  # noqa: E402
from cst_captioning_amd.ops.cider_d import CiderDScorer  # noqa: E402
from cst_captioning_amd.ops.mbr import PeerCiderD  # noqa: E402
from cst_captioning_amd.parallel import DistContext  # noqa: E402
from cst_captioning_amd.train.trainer import Trainer  # noqa: E402

xe_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
N = int(sys.argv[2]) if len(sys.argv) > 2 else 20
top_k = int(sys.argv[3]) if len(sys.argv) > 3 else 0
top_p = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
if not torch.cuda.is_available():
    sys.exit('needs a GPU')
dev = torch.device('cuda', 0)
torch.manual_seed(0)
V, FD, NV, B, H = 2000, [256, 128], 1280, 32, 256
tr, va, _ = make_splits('msrvtt', vocab_size=V, feat_dims=FD, train_videos=NV, seed=0,
                        caption_mode='template')
opt = default_opts(batch_size=B, train_seq_per_img=20, rnn_size=H, input_encoding_size=H,
                   learning_rate=2e-3, max_epochs=10 ** 9, print_log_interval=0, impl='hip',
                   loglevel='WARNING', use_eos=1, drop_prob_lm=0.5)
opt.vocab = {i: w for i, w in enumerate(tr.vocab)}
opt.vocab_size, opt.seq_length, opt.feat_dims = tr.vocab_size, tr.seq_length, tr.feat_dims
loader = CaptionLoader(tr, B, 20, 'train', dev, seed=0)
val = CaptionLoader(va, 64, 20, 'test', dev)
model, eng = build_model(opt, dev, 'hip')
assert eng is not None
t = Trainer(opt, model, loader, None, DistContext(device=dev), eng)
for it in range(xe_steps):
    out = t.train_step(loader.get_batch(), 0)
va.df = tr.df
ref = CiderDScorer(va, use_eos=1, device=dev)
peer = PeerCiderD(tr.df, use_eos=1, device=dev)


def val_cider(o):
    """mean CIDEr-D of the decoded validation captions, and how often MBR left row 0"""
    model.eval()
    tot, n, moved = 0.0, 0, 0
    with torch.no_grad():
        for ii in range((va.num_videos + 63) // 64):
            d = val.get_batch_at(ii)
            if o.get('decode') == 'mbr':
                seq, _, info = model.sample_mbr(d['feats'], o)
                moved += int((info['best'] != 0).sum())
            else:
                seq, _ = model.sample(d['feats'], o)
            tot += float(ref.score(seq.contiguous(), d['video_index']).sum())
            n += seq.size(0)
    model.train()
    return round(tot / n, 4), moved, n


res = {'xe_steps': xe_steps, 'xe_loss': round(float(out['loss']), 4), 'videos': va.num_videos,
       'mbr_samples': N, 'top_k': top_k, 'top_p': top_p}
res['greedy'] = val_cider({'beam_size': 1})[0]
res['beam5'] = val_cider({'beam_size': 5})[0]
for bs in (1, 5):
    for temp in (1.0, 0.7, 0.4):
        torch.manual_seed(1)
        c, moved, n = val_cider({'decode': 'mbr', 'beam_size': bs, 'mbr_samples': N,
                                 'mbr_temperature': temp, 'mbr_scorer': peer})
        key = 'mbr_row0_%s_t%.1f' % ('greedy' if bs == 1 else 'beam5', temp)
        res[key] = {'cider_d': c, 'not_row0': moved, 'of': n}
        if top_k > 0:  # the same pools' seed, the samples truncated
            torch.manual_seed(1)
            c, moved, n = val_cider({'decode': 'mbr', 'beam_size': bs, 'mbr_samples': N,
                                     'mbr_temperature': temp, 'mbr_top_k': top_k,
                                     'mbr_top_p': top_p, 'mbr_scorer': peer})
            res[key + '_top%d_p%.2f' % (top_k, top_p)] = {'cider_d': c, 'not_row0': moved, 'of': n}
print(json.dumps(res))
