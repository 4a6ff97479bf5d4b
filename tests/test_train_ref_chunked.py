"""CPU: the chunked training-step checker (oracle/torch_train_ref.train_step_chunked) equals the one-graph checker.

tests/test_gpu_train_regimes.py compares the HIP training step at its real batch sizes (up to 208 pairs of 341x192) with the
chunked form, which never holds more than `chunk` pairs in one autograd graph.  It is exact because the RunningMeanAndVar update
is taken from the whole batch first and everything behind it is per sample; this pins that claim in float64, with dropout masks,
an odd batch and a chunk size that does not divide it."""
import numpy as np
import pytest
import torch

from oracle import torch_train_ref as ref
from pointnav_vo_amd import model_spec as ms, synth

SPACE = ["rgb", "depth", "discretized_depth", "top_down_view"]


def case(B, seed=4):
    cfg = ms.config_from_kwargs(observation_space=SPACE, observation_size=(45, 37), hidden_size=512, resnet_baseplanes=32,
                                normalize_visual_inputs=True, output_dim=3, discretized_depth_channels=10)
    sd = synth.make_state_dict(ms.state_dict_spec(cfg), seed=seed)
    obs = synth.make_obs_pairs(B, cfg.height, cfg.width, observation_space=SPACE, dd_bins=10, seed=seed, depth_fp16=False)
    target = synth.uniform(seed, "chunk_target", (B, 3), -0.3, 0.3).astype(np.float32)
    keep = 0.8
    m0 = (synth.uniform(seed, "m0", (B, cfg.fc_in)) < keep) / keep
    m1 = (synth.uniform(seed, "m1", (B, cfg.hidden)) < keep) / keep
    return cfg, sd, obs, target, (torch.from_numpy(m0), torch.from_numpy(m1))


def rel(a, b):
    a, b = a.reshape(-1).double(), b.reshape(-1).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("B,chunk,dropout", [(6, 2, False), (6, 2, True), (7, 3, True)])
def test_chunked_checker_equals_the_one_graph_checker(B, chunk, dropout):
    cfg, sd, obs, target, masks = case(B)
    masks = masks if dropout else None
    lr = 1e-3
    one = ref.train_step(sd, obs, target, ngroups=cfg.ngroups, dtype=torch.float64, drop_masks=masks, lr=lr)
    chk = ref.train_step_chunked(sd, obs, target, ngroups=cfg.ngroups, chunk=chunk, dtype=torch.float64, drop_masks=masks, lr=lr)
    assert abs(float(chk["loss"]) - float(one["loss"])) <= 1e-12 * abs(float(one["loss"]))
    assert rel(chk["out"], one["out"]) < 1e-12
    assert set(chk["grads"]) == set(one["grads"]) and set(chk["params"]) == set(one["params"])
    bad = [(k, rel(chk["grads"][k], g)) for k, g in one["grads"].items() if not rel(chk["grads"][k], g) < 1e-12]
    assert not bad, bad
    # Adam: an element whose gradient is ~1e-12 of the tensor's scale may take a slightly different step; 1e-9 lr bounds them all
    # (measured 3e-10 lr)
    for k, p in one["params"].items():
        assert float((chk["params"][k] - p).abs().max()) <= 1e-9 * lr, k
        for a, b in zip(chk["state"][k], one["state"][k]):
            assert rel(a, b) < 1e-12, k
    assert set(chk["buffers"]) == set(one["buffers"])
    for k, b in one["buffers"].items():
        assert chk["buffers"][k].shape == b.shape, k
        assert torch.allclose(chk["buffers"][k], b, rtol=1e-12, atol=1e-15), k
    # the statistics did move (the batch is part of the update) and the count is the old count + B
    rmv = "visual_encoder.running_mean_and_var."
    assert float(chk["buffers"][rmv + "_count"]) == float(sd[rmv + "_count"]) + B
    assert not torch.allclose(chk["buffers"][rmv + "_mean"], torch.as_tensor(sd[rmv + "_mean"]).double())


def test_chunk_of_the_whole_batch_is_the_one_graph_checker_in_float32():
    """chunk >= B: one chunk, the same graph up to the whitening's statistics pass (split in two sums) — float32-grade equal."""
    cfg, sd, obs, target, _ = case(4, seed=9)
    one = ref.train_step(sd, obs, target, ngroups=cfg.ngroups, dtype=torch.float32)
    chk = ref.train_step_chunked(sd, obs, target, ngroups=cfg.ngroups, chunk=16, dtype=torch.float32)
    assert abs(float(chk["loss"]) - float(one["loss"])) <= 1e-5 * abs(float(one["loss"]))
    worst = max(rel(chk["grads"][k], g) for k, g in one["grads"].items())
    assert worst < 1e-3, worst
