"""``--val_scorer tokens`` under data parallelism (torchrun, gloo, CPU ranks):
the ranks decode disjoint batches, the main rank scores the gathered rows, and
every rank receives the scores.  World size 2 must reproduce world size 1."""
import os
import socket
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, out):
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([ROOT, HERE, env.get('PYTHONPATH', '')])
    env['CUDA_VISIBLE_DEVICES'] = ''  # CPU ranks (gloo)
    env['HIP_VISIBLE_DEVICES'] = ''
    env['OMP_NUM_THREADS'] = '1'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
           '--nproc-per-node', str(world), '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(HERE, 'corpus_dist_worker.py'), out]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return torch.load(out, weights_only=False)


def test_sharded_token_validation_matches_single_rank(tmp_path):
    from cst_captioning_amd.ops.corpus_metrics import KEYS
    one = _run(1, str(tmp_path / 'w1.pt'))
    two = _run(2, str(tmp_path / 'w2.pt'))
    assert one['world'] == 1 and two['world'] == 2
    assert one['predictions'] == two['predictions']
    for k in KEYS:
        assert one['scores'][k] == two['scores'][k], k
    # every video was decoded by exactly one rank
    vids = np.concatenate([v for _, v in two['rows']])
    assert sorted(vids.tolist()) == list(range(len(one['predictions'])))
    assert all(len(s) > 0 for s, _ in two['rows'])
