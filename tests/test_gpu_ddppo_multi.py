"""GPU (-m gpu): the data-parallel PPO agent (pointnav_vo_amd.ddppo.DDPPO) as two ranks, launched as tests/test_gpu_multi.py launches
its worker: two processes under torch.distributed.run, assertions inside tests/ddppo_worker.py, exit code 0.

  shared_gpu : both ranks on cuda:0 with gloo collectives — everything but RCCL itself, on any GPU box.  Cases C (depth, LSTM, T = 3,
               N = 2, the default 341 x 192 frame), B1 (the T = 1 single-forward form, N = 4: two environments per rank) and RGBD (rgb +
               depth, normalised, resets) of the float64 models; `update`: the distributed advantages and one whole DDPPO.update with
               rollouts of different lengths on the two ranks.
  two GPUs   : the same modes over backend nccl (RCCL), one GPU per rank; skipped on a one-GPU box.
At most three processes have the GPU open (the two ranks and pytest); every launch has its timeout and nothing is retried."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
need2 = pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs at least 2 GPUs")
MODES = ["C", "B1", "RGBD", "update"]


def _run(mode, *extra):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "ddppo_worker.py"), "--mode", mode, *extra],
                       capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env={**os.environ, "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]


@pytest.mark.parametrize("mode", MODES)
def test_two_ranks_sharing_one_gpu(mode):
    _run(mode, "--shared-gpu")


@need2
@pytest.mark.parametrize("mode", MODES)
def test_two_gpus_over_rccl(mode):
    _run(mode)
