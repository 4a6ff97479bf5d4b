"""GPU (-m gpu): the library's own count of the device and host-mapped memory it holds (pnvo_device_bytes_live) through the life of
every state object that owns some: it rises when a state is first built or a workspace grows, stays put in steady state and across a
same-sized reload, and returns to its starting value — exactly — when the handle goes.  The counter is the library's own, so every
assertion is on an exact difference from a baseline taken at the start of the test (other tests' models may be alive in the process).

Shapes: the smallest the suite uses — VO models on 45x37 frames with the benchmark's observation space, the policy on 128x96 frames
with hidden 128 (case A of tests/ppo_reference.py and its GRU twin)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import gru_reference as G
import ppo_reference as R
from pointnav_vo_amd import _lib, model_spec as ms, synth
from pointnav_vo_amd import vo_cnn  # noqa: F401
from pointnav_vo_amd.policy import GOAL_SENSOR, PointNavResNetPolicy
from pointnav_vo_amd.ppo import PolicyTrainStep
from pointnav_vo_amd.registry import baseline_registry
from pointnav_vo_amd.train import VOTrainStep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SPACE = ["rgb", "depth", "discretized_depth", "top_down_view"]     # bench.SPACE
W, H = 45, 37


def live():
    gc.collect()
    torch.cuda.synchronize()
    return _lib.lib.pnvo_device_bytes_live()


def vo_model(name="vo_cnn_rgb_d_dd_top_down"):
    m = baseline_registry.get_vo_model(name)(
        observation_space=SPACE, observation_size=(W, H), hidden_size=512, backbone="resnet18", normalize_visual_inputs=True,
        output_dim=3, dropout_p=0.0, discretized_depth_channels=10)
    sd = synth.make_state_dict(ms.state_dict_spec(m.cfg), seed=0)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return m.to(DEV).eval()


def pairs(B):
    obs = synth.make_obs_pairs(B, H, W, observation_space=SPACE, dd_bins=10, seed=B)
    return {k: torch.from_numpy(v).to(DEV) for k, v in obs.items()}


def eval_life_cycle(model, base):
    """2 pairs, 2 again, 5 (workspace grown), 2, a reload of same-sized weights, release."""
    with torch.no_grad():
        model(pairs(2))
        first = live()
        assert first > base
        model(pairs(2))
        assert live() == first
        model(pairs(5))
        grown = live()
        assert grown > first
        model(pairs(2))
        assert live() == grown
        next(model.parameters()).mul_(0.5)                 # in place: the next forward reloads every operand, same sizes
        model(pairs(2))
        assert live() == grown
    model._release()
    assert live() == base


def test_vo_model_forward_growth_reload_and_release():
    base = live()
    eval_life_cycle(vo_model(), base)


@pytest.mark.parametrize("state", ["bfloat16", "stem=dd", "stem=dense"])
def test_lazily_built_eval_states_are_released(state):
    base = live()
    model = vo_model()
    if state == "bfloat16":
        model.set_precision("bfloat16")
    else:
        model.set_option(*state.split("="))
    eval_life_cycle(model, base)


def test_train_state_through_train_eval_train_is_released():
    base = live()
    model = vo_model()
    ts = VOTrainStep(model, lr=1e-4)
    obs, tgt = pairs(2), torch.full((2, 3), 0.1, device=DEV)

    def round_trip():
        model.train()
        ts.step(obs, tgt)
        with torch.no_grad():
            model.eval()(obs)
        model.train()
        ts.step(obs, tgt)
        return live()

    steady = round_trip()
    assert steady > base
    assert round_trip() == steady
    flat = ts.flat.clone()
    model._release()
    assert live() == base
    assert torch.equal(ts.flat, flat)                      # the caller's flat buffer is not the library's to free


def test_act_embed_train_state_is_released():
    base = live()
    model = vo_model("vo_cnn_act_embed")
    ts = VOTrainStep(model, lr=1e-4)
    obs, tgt, actions = pairs(2), torch.full((2, 3), 0.1, device=DEV), torch.tensor([1, 2], device=DEV)
    model.train()
    ts.step(obs, tgt, actions=actions)
    steady = live()
    assert steady > base
    ts.step(obs, tgt, actions=actions)
    assert live() == steady
    model._release()
    assert live() == base


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n):
        self.n = n


@pytest.mark.parametrize("rnn_type", ["LSTM", "GRU"])
def test_policy_act_update_and_release_leave_borrowed_memory_alone(rnn_type):
    base = live()
    c = R.CASES["A"]
    Hp, Wp, Hd, L, A = c["H"], c["W"], c["hidden"], c["L"], c["A"]
    space = Space({"depth": Box((Hp, Wp, 1)), "rgb": Box((Hp, Wp, 3)), GOAL_SENSOR: Box((2,))})
    pol = PointNavResNetPolicy(observation_space=space, action_space=Act(A), hidden_size=Hd, rnn_type=rnn_type, num_recurrent_layers=L,
                               backbone="resnet18", goal_sensor_uuid=GOAL_SENSOR, normalize_visual_inputs=False, obs_transform=None,
                               vis_types=["depth"])
    sd = (G if rnn_type == "GRU" else R).state_dict("A")
    pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    pol = pol.to(DEV).eval()
    gen = torch.Generator(device="cpu").manual_seed(3)
    T, N = 2, 2
    M = T * N
    depth = torch.rand((M, Hp, Wp, 1), generator=gen).to(DEV)
    goal = torch.rand((M, 2), generator=gen).to(DEV)
    prev = torch.randint(0, A, (M, 1), generator=gen).to(DEV)
    masks = torch.ones((M, 1), device=DEV)
    hidden = torch.zeros((pol.num_recurrent_layers, N, Hd), device=DEV)
    obs2 = {"depth": depth[:N], GOAL_SENSOR: goal[:N]}
    pol.act(obs2, hidden, prev[:N], masks[:N], deterministic=True)
    first = live()
    assert first > base
    pol.act(obs2, hidden, prev[:N], masks[:N], deterministic=True)
    assert live() == first

    step = PolicyTrainStep(pol, lr=2.5e-4, eps=1e-5, max_grad_norm=0.2)
    value, logp, _, _ = step.evaluate_actions({"depth": depth, GOAL_SENSOR: goal}, hidden, prev, masks, prev)
    adv = torch.tensor([0.5, -0.5, 0.25, -0.25], device=DEV).view(M, 1)
    step.ppo_loss(logp.detach() + 0.1, adv, value.detach() + 0.1, value.detach() + 0.1 + adv, 0.2, 0.5, 0.01)
    step.backward()
    step.clip_grad_norm()
    step.optimizer_step()
    assert live() > first
    kept = [t.clone() for t in (step.flat, step.grad, step.exp_avg, step.exp_avg_sq)]
    pol._release()
    assert live() == base
    for t, k in zip((step.flat, step.grad, step.exp_avg, step.exp_avg_sq), kept):
        assert torch.equal(t, k)                           # borrowed memory stays readable and untouched


def test_failed_train_attach_leaves_no_state_behind():
    """A parameter table whose last entry runs past n_floats: an argument error returned by host code before any launch."""
    base = live()
    model = vo_model()
    obs = pairs(2)
    with torch.no_grad():
        before = model(obs).clone()
    held = live()
    entries, off = [], 0
    for name, p in model.named_parameters():
        entries.append((name, off, tuple(p.shape)))
        off += p.numel()
    flat, grad = torch.zeros(off, device=DEV), torch.zeros(off, device=DEV)
    toc = _lib.make_toc(entries)
    rc = _lib.lib.pnvo_train_attach(model._handle, C.c_void_p(flat.data_ptr()), C.c_void_p(grad.data_ptr()), off - 1, toc, len(entries))
    assert rc != 0 and b"out of range" in _lib.lib.pnvo_last_error(model._handle)
    assert live() == held
    with torch.no_grad():
        assert torch.equal(model(obs), before)
    model._release()
    assert live() == base
