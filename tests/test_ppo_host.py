"""CPU (-m "not gpu"): the host side of the PPO update path (pointnav_vo_amd.ppo) — what can be checked without an MI355X."""
import inspect

import pytest
import torch

from pointnav_vo_amd import ppo
from pointnav_vo_amd.policy import PointNavResNetPolicy, policy_state_dict_spec


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n):
        self.n = n


def cpu_policy(H=96, W=128, hidden=128, layers=2, n_actions=3):
    space = Space({"depth": Box((H, W, 1)), "pointgoal_with_gps_compass": Box((2,))})
    return PointNavResNetPolicy(observation_space=space, action_space=Act(n_actions), hidden_size=hidden, rnn_type="LSTM",
                                num_recurrent_layers=layers, backbone="resnet18", normalize_visual_inputs=False, obs_transform=None,
                                vis_types=["depth"])


def test_module_imports_and_exposes_the_agent():
    assert hasattr(ppo, "PPO") and hasattr(ppo, "PolicyTrainStep") and ppo.EPS_PPO == 1e-5


def test_ppo_constructor_keywords_are_the_reference_agents():
    want = ["actor_critic", "clip_param", "ppo_epoch", "num_mini_batch", "value_loss_coef", "entropy_coef", "lr", "eps",
            "max_grad_norm", "use_clipped_value_loss", "use_normalized_advantage"]
    sig = inspect.signature(ppo.PPO.__init__)
    assert list(sig.parameters)[1:] == want
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {"lr": None, "eps": None, "max_grad_norm": None, "use_clipped_value_loss": True,
                        "use_normalized_advantage": True}
    for name in ("get_advantages", "update", "before_backward", "after_backward", "before_step", "after_step"):
        assert callable(getattr(ppo.PPO, name))


def test_train_step_refuses_a_cpu_policy():
    with pytest.raises(RuntimeError, match="cuda"):
        ppo.PolicyTrainStep(cpu_policy())
    with pytest.raises(RuntimeError, match="cuda"):
        ppo.PPO(cpu_policy(), 0.2, 1, 2, 0.5, 0.01, lr=2.5e-4, eps=1e-5, max_grad_norm=0.2)


def test_unattached_policy_refuses_evaluate_actions_without_touching_the_device():
    pol = cpu_policy()
    with pytest.raises(NotImplementedError):
        pol.evaluate_actions({}, None, None, None, None)


@pytest.mark.parametrize("n_actions,layers", [(3, 2), (4, 1)])
def test_flat_offsets_cover_every_parameter_once_in_order(n_actions, layers):
    pol = cpu_policy(n_actions=n_actions, layers=layers)
    spec = policy_state_dict_spec(width=128, height=96, hidden=128, n_actions=n_actions, rnn_layers=layers)
    named = [(n, tuple(p.shape)) for n, p in pol.named_parameters()]
    assert named == [(n, tuple(s)) for n, s in spec]                   # named_parameters() order is the state_dict's
    offsets, used = ppo.flat_offsets(named)
    assert list(offsets) == [n for n, _ in spec]
    end = 0
    for (name, shape), (off, numel) in zip(spec, offsets.values()):
        assert numel == int(torch.Size(shape).numel()), name
        assert off >= end and off % 4 == 0 and off - end < 4, (name, off, end)   # in order, no overlap, 16-byte aligned, tight
        end = off + numel
    assert end <= used < end + 4 and used % 4 == 0
    # 3 actions: the actor's bias has 3 elements, so the critic's weight would start off a 16-byte boundary without the padding
    if n_actions == 3:
        assert offsets["action_distribution.linear.bias"][1] == 3 and offsets["critic.fc.weight"][0] % 4 == 0
