"""CPU: the callable visual encoder of the navigation policy on the host side (the reference trainers' frozen-encoder branch,
ddppo_trainer.py:158-161,257-271, reads `net.visual_encoder.output_shape` and calls the module): output_shape by the reference's
formula, unchanged state-dict keys, a module tree without a cycle, and no CPU fallback."""
import numpy as np
import pytest
import torch

from pointnav_vo_amd.policy import GOAL_SENSOR, PointNavResNetPolicy, policy_state_dict_spec


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    n = 4


def make_policy(H, W, **kw):
    space = Space({"depth": Box((H, W, 1)), "rgb": Box((H, W, 3)), GOAL_SENSOR: Box((2,))})
    return PointNavResNetPolicy(observation_space=space, action_space=Act(), hidden_size=128, rnn_type="LSTM", num_recurrent_layers=1,
                                backbone="resnet18", goal_sensor_uuid=GOAL_SENSOR, normalize_visual_inputs=False, obs_transform=None,
                                vis_types=["depth"], **kw)


def reference_output_shape(H, W):
    """ResNetEncoder.__init__ (resnet_policy.py:89-133): half the frame (avg_pool2d(2)), the backbone's final_spatial_compress of
    1 / 32 rounded up, 2048 floats shared among the positions — listed in the order of the tensor the encoder returns, [C, rows, cols]."""
    fh = int(np.ceil((H // 2) * (1.0 / 32)))
    fw = int(np.ceil((W // 2) * (1.0 / 32)))
    return int(round(2048 / (fh * fw))), fh, fw


@pytest.mark.parametrize("W,H,want", [(128, 96, (512, 2, 2)), (341, 192, (114, 3, 6)), (300, 192, (137, 3, 5)), (256, 256, (128, 4, 4))])
def test_output_shape_is_the_reference_formula(W, H, want):
    enc = make_policy(H, W).net.visual_encoder
    assert tuple(enc.output_shape) == reference_output_shape(H, W) == want
    assert enc.is_blind is False
    spec = dict(policy_state_dict_spec(width=W, height=H, hidden=128, rnn_layers=1))
    C, fh, fw = enc.output_shape
    assert spec["net.visual_encoder.compression.0.weight"][0] == C and spec["net.visual_fc.1.weight"] == (128, C * fh * fw)


def test_state_dict_keys_are_unchanged():
    pol = make_policy(192, 341)
    spec = policy_state_dict_spec(width=341, height=192, hidden=128, rnn_layers=1)
    assert [(k, tuple(v.shape)) for k, v in pol.state_dict().items()] == [(n, tuple(s)) for n, s in spec]
    enc = pol.net.visual_encoder
    own = [(k, tuple(v.shape)) for k, v in enc.state_dict().items()]
    assert own == [(n[len("net.visual_encoder."):], tuple(s)) for n, s in spec if n.startswith("net.visual_encoder.")]
    # what the trainers do with it: freeze, eval, load a pretrained encoder
    assert len(list(enc.parameters())) == len(own)
    for p in enc.parameters():
        p.requires_grad_(False)
    assert enc.eval() is enc and not enc.training
    enc.load_state_dict({k: torch.full_like(v, 0.5) for k, v in enc.state_dict().items()})
    assert all(bool((v == 0.5).all()) for k, v in pol.state_dict().items() if k.startswith("net.visual_encoder."))


def test_the_encoder_does_not_hold_its_policy():
    pol = make_policy(96, 128)
    enc = pol.net.visual_encoder
    mods = list(pol.modules())
    assert sum(m is enc for m in mods) == 1 and sum(m is pol for m in mods) == 1
    assert len(mods) == len({id(m) for m in mods})
    assert all(m is not pol for m in enc.modules())           # no cycle through add_module: the walk below would not end
    assert not any(v is pol for v in vars(enc).values()) and not any(v is pol for v in enc._modules.values())
    assert [n for n, _ in pol.named_modules()].count("net.visual_encoder") == 1
    assert enc._policy() is pol


def test_calling_it_on_a_cpu_policy_raises():
    pol = make_policy(96, 128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pol.net.visual_encoder({"depth": torch.zeros(1, 96, 128, 1)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pol.act({"visual_features": torch.zeros(1, 512, 2, 2), GOAL_SENSOR: torch.zeros(1, 2)}, torch.zeros(2, 1, 128),
                torch.zeros(1, 1, dtype=torch.int64), torch.ones(1, 1))
