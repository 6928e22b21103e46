"""Sanitizer run of the native peer scorer under a mixed utility (``--mbr_mix``).

``csrc/host/peer_mix_host.cpp`` (``peer_mix_host``), ``csrc/host/metric_host.cpp``
and ``csrc/host/cider_host.cpp`` are compiled with ``-fsanitize=address,undefined`` (no recovery) together with
the stand-alone driver ``tests/native/peer_mix_host_check.cpp``, which scores
pools of up to 100 rows, width-64 rows and empty batches, and compares every
BLEU-4 / ROUGE-L peer score with "table of the pool, own row excluded" (the
table scorers with ``exclude``).  No Python extension and no preloaded runtime
are involved (as in ``test_native_mbr_sanitizers.py``).
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_peer_mix_host_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'peer_mix_host_check')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer',
           '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I' + os.path.join(REPO, 'csrc'),
           os.path.join(REPO, 'csrc', 'host', 'cider_host.cpp'),
           os.path.join(REPO, 'csrc', 'host', 'metric_host.cpp'),
           os.path.join(REPO, 'csrc', 'host', 'peer_mix_host.cpp'),
           os.path.join(REPO, 'tests', 'native', 'peer_mix_host_check.cpp'), '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0',
               UBSAN_OPTIONS='print_stacktrace=1')
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().endswith('ok'), res.stdout
    assert 'runtime error' not in res.stderr, res.stderr
