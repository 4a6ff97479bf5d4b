"""bench.py --dump-outputs: the float32 .npy files hold what the timed path returned in its last step — the same arrays a
caller gets from the forward on the benchmark's seeded inputs, bit for bit — so two builds can be compared file for file."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _bench(out_dir, *extra, launcher=()):
    cmd = [sys.executable, *launcher, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-secondary",
           "--no-cpu-baseline", "--dump-outputs", str(out_dir), *extra]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)


def _load(out_dir):
    return {f[:-len(".npy")]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["fwd_fp32", "dual_bf16"])
def test_dump_is_the_forward_on_the_benchmark_inputs(tmp_path, config):
    import bench
    from pointnav_vo_amd import vo_cnn

    r = _bench(tmp_path, "--gpus", "1", "--config", config)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    got = _load(tmp_path)
    dev = torch.device("cuda", 0)
    obs = bench.make_inputs(256, dev, 0)
    with torch.no_grad():
        if config == "fwd_fp32":
            want = {"pose_delta": bench.build_model(dev)[0](obs)}
        else:
            ma, mb = (bench.build_model(dev, seed=s)[0].set_precision("bfloat16") for s in (0, 1))
            oa, ob = vo_cnn.dual_forward(ma, mb, obs)
            want = {"pose_delta_a": oa, "pose_delta_b": ob}
    assert sorted(got) == sorted(want)
    for name, a in got.items():
        assert a.dtype == np.float32 and a.shape == (256, 3), (name, a.dtype, a.shape)
        np.testing.assert_array_equal(a, want[name].cpu().numpy(), err_msg=name)


@pytest.mark.gpu
def test_dump_of_two_ranks_holds_both_batches_in_rank_order(tmp_path):
    """N = 2 (both ranks on cuda:0 over gloo): rank 0 writes the gathered outputs, rank 0's pairs first."""
    import bench

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    launcher = ("-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", str(port))
    r = _bench(tmp_path, "--gpus", "2", "--backend", "gloo", "--shared-gpu", "--batch", "16", launcher=launcher)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    got = _load(tmp_path)
    dev = torch.device("cuda", 0)
    model = bench.build_model(dev)[0]
    with torch.no_grad():
        want = torch.cat([model(bench.make_inputs(16, dev, rank)) for rank in (0, 1)]).cpu().numpy()
    assert sorted(got) == ["pose_delta"]
    np.testing.assert_array_equal(got["pose_delta"], want)


def test_train_config_refuses_to_dump(tmp_path):
    """A training step's outputs depend on every earlier step (the pre-heat's count varies): no dump that would differ run to run."""
    r = _bench(tmp_path / "out", "--gpus", "1", "--config", "train")
    assert r.returncode == 2 and "--dump-outputs" in r.stderr, r.stderr[-1500:]
    assert not (tmp_path / "out").exists()
