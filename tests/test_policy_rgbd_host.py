"""CPU: the public interface of the rgb / rgb-d / normalised navigation policy, without a device.

  - policy_state_dict_spec equals the reference policy's recorded state_dict names, shapes and order for the four configurations of
    tests/golden/policy_rgbd_128x96_h128_b2.npz (written by tests/golden/gen_golden_policy_rgbd.py from the imported reference);
  - RunningMeanAndVar's three statistics are registered buffers, in state_dict() and load_state_dict, absent from named_parameters();
  - the depth-only spec and constructor are what they were;
  - bad rgb shapes / dtypes, missing keys and a process group in training mode raise in _visual_input, before any device is touched;
  - the float64 model of tests/rgbd_policy_reference.py, which the GPU tests compare against, reproduces the reference policy's
    recorded outputs and statistics of every case and step.
"""
import os

import numpy as np
import pytest
import torch

import rgbd_policy_reference as Q
from conftest import load_golden
from pointnav_vo_amd import synth
from pointnav_vo_amd.policy import RMV_PREFIX, PointNavResNetPolicy, policy_state_dict_spec

GOAL = Q.GOAL
H, W, HIDDEN, LAYERS, N_ACT, B = 96, 128, 128, 2, 4, 2
# case -> (vis_types, rnn_type, zero-initialised statistics, training flag of each step): tests/golden/gen_golden_policy_rgbd.py
CASES = {"a": (["rgb", "depth"], "LSTM", False, [False] * 4), "b": (["rgb", "depth"], "GRU", True, [True] * 3),
         "c": (["rgb"], "LSTM", False, [False, True]), "d": (["depth"], "LSTM", True, [True])}
CPU = torch.device("cpu")


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n):
        self.n = n


def golden():
    return load_golden("policy_rgbd_128x96_h128_b2.npz")


def make_policy(vis, rnn="LSTM", normalize=True, h=H, w=W):
    space = Space({"depth": Box((h, w, 1)), "rgb": Box((h, w, 3)), GOAL: Box((2,))})
    return PointNavResNetPolicy(observation_space=space, action_space=Act(N_ACT), hidden_size=HIDDEN, rnn_type=rnn,
                                num_recurrent_layers=LAYERS, backbone="resnet18", goal_sensor_uuid=GOAL,
                                normalize_visual_inputs=normalize, obs_transform=None, vis_types=vis)


def obs_of(vis, rgb_dtype=torch.uint8, h=H, w=W, n=B):
    obs = {GOAL: torch.zeros(n, 2)}
    if "rgb" in vis:
        obs["rgb"] = torch.zeros(n, h, w, 3, dtype=rgb_dtype)
    if "depth" in vis:
        obs["depth"] = torch.zeros(n, h, w, 1)
    return obs


@pytest.mark.parametrize("case", list(CASES))
def test_spec_equals_the_recorded_reference_state_dict(case):
    vis, rnn = CASES[case][:2]
    g = golden()
    want = [(str(n), tuple(int(d) for d in str(s).split(",") if d)) for n, s in zip(g[f"{case}/sd_names"], g[f"{case}/sd_shapes"])]
    spec = policy_state_dict_spec(width=W, height=H, hidden=HIDDEN, n_actions=N_ACT, rnn_layers=LAYERS, rnn_type=rnn, vis_types=vis,
                                  normalize_visual_inputs=True)
    assert [(n, tuple(s)) for n, s in spec] == want
    C = (3 if "rgb" in vis else 0) + (1 if "depth" in vis else 0)
    d = dict(spec)
    assert d["net.visual_encoder.backbone.conv1.0.weight"] == (32, C, 7, 7)
    enc = [n for n, _ in spec if n.startswith("net.visual_encoder.")]
    assert enc[:3] == [RMV_PREFIX + "_mean", RMV_PREFIX + "_var", RMV_PREFIX + "_count"]
    assert d[RMV_PREFIX + "_mean"] == d[RMV_PREFIX + "_var"] == (1, C, 1, 1) and d[RMV_PREFIX + "_count"] == ()
    # the module mirrors it: same keys in the same order, the statistics as buffers
    pol = make_policy(vis, rnn)
    assert [(k, tuple(v.shape)) for k, v in pol.state_dict().items()] == want
    assert sorted(k for k, _ in pol.named_buffers()) == sorted(str(n) for n in g[f"{case}/buffer_names"])
    # without normalisation the same spec minus the three buffers
    plain = policy_state_dict_spec(width=W, height=H, hidden=HIDDEN, n_actions=N_ACT, rnn_layers=LAYERS, rnn_type=rnn, vis_types=vis)
    assert plain == [e for e in spec if not e[0].startswith(RMV_PREFIX)]


def test_statistics_are_buffers_not_parameters():
    pol = make_policy(["rgb", "depth"])
    names = [RMV_PREFIX + k for k in ("_mean", "_var", "_count")]
    params = dict(pol.named_parameters())
    assert all(n not in params for n in names) and [n for n, _ in pol.named_buffers()] == names
    assert all(not b.requires_grad and float(b.abs().sum()) == 0.0 for _, b in pol.named_buffers())     # running_mean_and_var.py:16-18
    assert [n for n, _ in pol._param_spec] == list(params)
    sd = synth.make_state_dict(pol._spec, seed=3)
    ptrs = [b.data_ptr() for _, b in pol.named_buffers()]
    pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    got = dict(pol.named_buffers())
    assert [b.data_ptr() for _, b in pol.named_buffers()] == ptrs                                       # loaded in place
    for n in names:
        np.testing.assert_array_equal(got[n].numpy(), sd[n])
    assert float(got[names[2]]) == 1000.0
    with pytest.raises(RuntimeError, match="_var"):
        pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items() if not k.endswith("_var")})


def test_depth_only_spec_and_constructor_are_unchanged():
    old = policy_state_dict_spec(width=W, height=H, hidden=HIDDEN, n_actions=N_ACT, rnn_layers=LAYERS)
    assert old == policy_state_dict_spec(width=W, height=H, hidden=HIDDEN, n_actions=N_ACT, rnn_layers=LAYERS, vis_types=("depth",),
                                         normalize_visual_inputs=False)
    assert dict(old)["net.visual_encoder.backbone.conv1.0.weight"] == (32, 1, 7, 7) and not any(RMV_PREFIX in n for n, _ in old)
    g = load_golden("policy_gru_128x96_h128_b2.npz")      # (a depth-only fixture: its generator asserts the spec against the reference)
    assert int(g["hidden"]) == HIDDEN
    pol = make_policy(["depth"], normalize=False)
    assert pol._plain and [k for k, _ in pol.state_dict().items()] == [n for n, _ in old] and not list(pol.named_buffers())
    assert pol._spec == pol._param_spec == old
    depth = torch.rand(B, H, W, 1)
    vis, from_features = pol._visual_input({"depth": depth, GOAL: torch.zeros(B, 2)}, CPU)
    assert torch.equal(vis, depth) and from_features is False                   # a tensor, as before: the depth-only entry points
    with pytest.raises(ValueError, match="neither 'visual_features' nor 'depth'"):
        pol._visual_input({GOAL: torch.zeros(B, 2)}, CPU)
    with pytest.raises(ValueError, match=r"expected \[B,96,128,1\]"):
        pol._visual_input({"depth": torch.rand(B, H, W + 1, 1)}, CPU)
    with pytest.raises(NotImplementedError, match="blind"):
        make_policy([])


def test_membership_decides_the_visual_types():
    pol = make_policy(("depth", "rgb", "semantic"), normalize=False)            # order and extra names do not matter
    assert (pol._n_rgb, pol._n_depth, pol._plain) == (3, 1, False)
    frames, _ = pol._visual_input(obs_of(["rgb", "depth"]), CPU)
    assert frames.stats is None and frames.rgb.dtype == torch.uint8 and frames.depth.dtype == torch.float32 and frames.shape[0] == B
    args = frames.args()
    assert args[1] == 1 and args[3:] == (None, None, None, 0)
    assert pol._visual_input(obs_of(["rgb", "depth"], torch.float32), CPU)[0].args()[1] == 0
    with pytest.raises(ValueError, match="observation space"):
        PointNavResNetPolicy(observation_space=Space({"depth": Box((H, W, 1)), GOAL: Box((2,))}), action_space=Act(N_ACT),
                             vis_types=["rgb", "depth"])


def test_bad_rgb_and_missing_keys_raise_before_the_device():
    pol = make_policy(["rgb", "depth"])                    # parameters on the CPU: reaching the library would raise RuntimeError instead
    ok = obs_of(["rgb", "depth"])
    pol._visual_input(ok, CPU)
    for key in ("rgb", "depth"):
        with pytest.raises(ValueError, match=f"neither 'visual_features' nor '{key}'"):
            pol._visual_input({k: v for k, v in ok.items() if k != key}, CPU)
        with pytest.raises(ValueError, match=f"net.visual_encoder needs observations\\['{key}'\\]"):
            pol._frames({k: v for k, v in ok.items() if k != key}, CPU, "net.visual_encoder needs observations[{}] (keys: {})")
    for bad, what in ((torch.zeros(B, H, W, 3, dtype=torch.float64), "dtype"), (torch.zeros(B, H, W, 3, dtype=torch.int32), "dtype"),
                      (torch.zeros(B, H, W, 4, dtype=torch.uint8), "shape"), (torch.zeros(B, H, W + 2, 3, dtype=torch.uint8), "shape"),
                      (torch.zeros(B, 3, H, W, dtype=torch.uint8), "shape"), (torch.zeros(B + 1, H, W, 3, dtype=torch.uint8), "frames")):
        with pytest.raises(ValueError, match=what):
            pol._visual_input(dict(ok, rgb=bad), CPU)
    with pytest.raises(ValueError, match="shape"):
        pol._visual_input(dict(ok, depth=torch.zeros(B, H, W)), CPU)
    # the public calls fail the same way, and a CPU policy never reaches the library
    hid, pa, mk = torch.zeros(2 * LAYERS, B, HIDDEN), torch.zeros(B, 1, dtype=torch.long), torch.zeros(B, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pol.act(ok, hid, pa, mk)
    # visual_features bypass the frames and the statistics altogether
    feats = torch.zeros((B,) + tuple(pol.net.visual_encoder.output_shape))
    vis, from_features = pol._visual_input({"visual_features": feats, GOAL: torch.zeros(B, 2)}, CPU)
    assert from_features and torch.equal(vis, feats)


def test_training_mode_under_a_process_group_names_the_missing_reduction(tmp_path):
    import torch.distributed as dist
    pol = make_policy(["rgb", "depth"])
    plain = make_policy(["rgb", "depth"], normalize=False)
    ok = obs_of(["rgb", "depth"])
    assert pol.training
    pol._visual_input(ok, CPU)                             # no process group: accepted
    dist.init_process_group("gloo", init_method=f"file://{os.path.join(str(tmp_path), 'pg')}", rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match="cross-process reduction"):
            pol._visual_input(ok, CPU)
        pol.eval()
        stats = pol._visual_input(ok, CPU)[0].stats        # eval reads the buffers: nothing to reduce
        assert stats[3] == 0 and stats[0] is pol.net.visual_encoder.running_mean_and_var._mean
        plain._visual_input(ok, CPU)                       # no statistics: training mode is fine
        pol.train()
        pol._visual_input({"visual_features": torch.zeros((B,) + tuple(pol.net.visual_encoder.output_shape)), GOAL: torch.zeros(B, 2)}, CPU)
    finally:
        dist.destroy_process_group()
    assert pol._visual_input(ok, CPU)[0].stats[3] == 1


@pytest.mark.parametrize("case", list(CASES))
def test_float64_model_reproduces_the_reference_policy(case):
    """tests/rgbd_policy_reference.py (what the GPU tests compare against) against the reference's recorded float64 outputs."""
    vis, rnn, zero, training = CASES[case]
    g = golden()
    sd = synth.make_state_dict(Q.spec(H=H, W=W, hidden=HIDDEN, A=N_ACT, L=LAYERS, rnn=rnn, vis=vis), seed=int(g[f"{case}/weight_seed"]))
    if zero:
        sd = {k: (np.zeros_like(v) if k.startswith(RMV_PREFIX) else v) for k, v in sd.items()}
    hid = np.zeros((LAYERS * (2 if rnn == "LSTM" else 1), B, HIDDEN))
    steps = synth.make_policy_rgbd_inputs(H, W, B, len(training), int(g[f"{case}/input_seed"]), N_ACT)
    for t, (rgb, depth, goal, prev, mask) in enumerate(steps):
        frames = {k: v for k, v in (("rgb", rgb), ("depth", depth)) if k in vis}
        o = Q.policy_step(sd, frames, goal, prev, mask, hid, rnn, training[t])
        for k, gk in (("features", "features64"), ("hidden", "hidden64"), ("logits", "logits_raw64"), ("value", "value64")):
            np.testing.assert_allclose(o[k], g[f"{case}/{gk}/{t}"], rtol=0, atol=1e-9, err_msg=f"{case} {t} {k}")
        for k, gk in (("_mean", "mean64"), ("_var", "var64"), ("_count", "count64")):
            np.testing.assert_allclose(o["stats"][k], g[f"{case}/{gk}/{t}"], rtol=0, atol=1e-12, err_msg=f"{case} {t} {k}")
        if training[t]:
            v = g[f"{case}/var64/{t}"].reshape(-1)
            assert ((v > 2e-2) | (v < 5e-3)).all() and ("depth" not in vis or (v < 5e-3).any())     # clear of the 1e-2 clamp
        else:
            np.testing.assert_array_equal(o["stats"]["_var"], np.asarray(sd[RMV_PREFIX + "_var"], np.float64))
        sd, hid = Q.with_stats(sd, o["stats"]), o["hidden"]
