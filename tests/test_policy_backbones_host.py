"""CPU: the Bottleneck / ResNeXt / SE-ResNeXt backbones of the navigation policy and the VO models, without a device.

  - policy_state_dict_spec(backbone=) equals the reference policy's recorded state_dict names, shapes and order for the six cases of
    tests/golden/policy_backbones_136x104_h128_b2.npz (written by tests/golden/gen_golden_policy_backbones.py from the imported
    reference); the cardinality reaches the first block of a stage only; the module mirrors the spec;
  - the float64 restatement of tests/backbone_reference.py, which the GPU tests compare against, reproduces every recorded tensor
    of every case and step — and the recorded VO output — to 1e-9 of its scale;
  - what is not built refuses before any device is touched: train_encoder=True, bfloat16, VOTrainStep, an unknown name.
"""
import numpy as np
import pytest
import torch

import backbone_reference as BR
from conftest import load_golden
from pointnav_vo_amd import model_spec as ms
from pointnav_vo_amd.policy import PointNavResNetPolicy, policy_state_dict_spec
from pointnav_vo_amd.ppo import PolicyTrainStep
from pointnav_vo_amd.train import VOTrainStep
from pointnav_vo_amd.vo_cnn import VisualOdometryCNNBase

FIXTURE = "policy_backbones_136x104_h128_b2.npz"
TOL = 1e-9                                               # of each tensor's scale (its largest |value|)


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n):
        self.n = n


@pytest.fixture(scope="module")
def golden():
    return load_golden(FIXTURE)


def make_policy(backbone, vis=("depth",), rnn="LSTM", normalize=False):
    space = Space({"depth": Box((BR.H, BR.W, 1)), "rgb": Box((BR.H, BR.W, 3)), BR.GOAL: Box((2,))})
    return PointNavResNetPolicy(observation_space=space, action_space=Act(BR.N_ACT), hidden_size=BR.HIDDEN, rnn_type=rnn,
                                num_recurrent_layers=BR.LAYERS, backbone=backbone, goal_sensor_uuid=BR.GOAL,
                                normalize_visual_inputs=normalize, obs_transform=None, vis_types=list(vis))


def scale_err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64).reshape(want.shape) - want).max() / max(np.abs(want).max(), 1e-300))


@pytest.mark.parametrize("case", list(BR.CASES))
def test_spec_equals_the_recorded_reference_state_dict(golden, case):
    c = BR.CASES[case]
    assert str(golden[f"{case}/backbone"]) == c["backbone"]
    want = [(str(n), tuple(int(d) for d in str(s).split(",") if d)) for n, s in zip(golden[f"{case}/sd_names"], golden[f"{case}/sd_shapes"])]
    spec = [(n, tuple(s)) for n, s in BR.spec(case)]
    assert spec == want
    d = dict(spec)
    bb = "net.visual_encoder.backbone."
    if c["backbone"] == "resneXt50":                     # the cardinality reaches the first block of a stage only (resnet.py:198-210)
        assert d[bb + "layer1.0.convs.3.weight"] == (64, 4, 3, 3) and d[bb + "layer1.1.convs.3.weight"] == (64, 64, 3, 3)
        assert [d[bb + f"layer{s}.0.convs.3.weight"] for s in (2, 3, 4)] == [(128, 8, 3, 3), (256, 16, 3, 3), (512, 32, 3, 3)]
        assert sum(1 for n, sh in spec if n.endswith("convs.3.weight") and sh[1] != sh[0]) == 4
    if c["backbone"] == "se_resneXt50":
        assert len(spec) == 243
        names = [n for n, _ in spec if n.startswith(bb + "layer1.0.")]
        assert [n[len(bb + "layer1.0."):] for n in names[-7:]] == ["downsample.0.weight", "downsample.1.weight", "downsample.1.bias",
                                                                   "se.excite.0.weight", "se.excite.0.bias", "se.excite.2.weight",
                                                                   "se.excite.2.bias"]
        assert d[bb + "layer4.2.se.excite.0.weight"] == (64, 1024)
    assert d["net.visual_encoder.compression.0.weight"] == (341, 1024, 3, 3) and d["net.visual_fc.1.weight"] == (BR.HIDDEN, 2046)


@pytest.mark.parametrize("backbone", ["se_resneXt50", "resnet50"])
def test_module_mirrors_the_spec_and_loads_a_state_dict(backbone):
    pol = make_policy(backbone)
    spec = policy_state_dict_spec(width=BR.W, height=BR.H, hidden=BR.HIDDEN, n_actions=BR.N_ACT, rnn_layers=BR.LAYERS, backbone=backbone)
    assert [(k, tuple(v.shape)) for k, v in pol.state_dict().items()] == [(n, tuple(s)) for n, s in spec]
    assert pol.net.visual_encoder.output_shape == (341, 2, 3)
    sd = BR.state_dict(backbone=backbone, vis=("depth",), normalize=False, rnn="LSTM")
    # a reference checkpoint keeps the policy under 'actor_critic.': stripped, it loads
    ckpt = {"actor_critic." + k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    pol.load_state_dict({k[len("actor_critic."):]: v for k, v in ckpt.items()})
    k = "net.visual_encoder.backbone.layer1.0.convs.3.weight"
    assert torch.equal(pol.state_dict()[k], torch.from_numpy(np.array(sd[k])))
    if backbone == "se_resneXt50":                       # ResNetEncoder.layer_init reaches the SE branch's Linear layers: zero biases
        fresh = make_policy(backbone).state_dict()
        assert float(fresh["net.visual_encoder.backbone.layer2.0.se.excite.0.bias"].abs().max()) == 0.0
        assert float(fresh["net.visual_encoder.backbone.layer2.0.se.excite.2.weight"].std()) > 0.0


def test_resnet18_spec_is_what_it_was():
    a = policy_state_dict_spec(width=128, height=96, hidden=128)
    assert a == policy_state_dict_spec(width=128, height=96, hidden=128, backbone="resnet18") and len(a) == 80


@pytest.mark.parametrize("case", list(BR.CASES))
def test_float64_restatement_reproduces_the_recorded_reference(golden, case):
    c = BR.CASES[case]
    steps = BR.run_case(case)
    assert len(steps) == c["steps"]
    worst = {}
    for t, r in enumerate(steps):
        for key, got in (("features64", r["features"]), ("hidden64", r["hidden"]), ("logits_raw64", r["logits"]), ("value64", r["value"]),
                         ("encoder64", r["encoder"])):
            worst[f"{key}/{t}"] = scale_err(got, golden[f"{case}/{key}/{t}"])
        for tap in BR.TAPS + (BR.last_tap(c["backbone"]),):
            assert tuple(r["taps"][tap].shape) == tuple(int(v) for v in golden[f"{case}/tapshape/{tap}"])
            vals, stat = BR.tap_digest(tap, r["taps"][tap])
            worst[f"tapval/{tap}/{t}"] = float(np.abs(vals - golden[f"{case}/tapval64/{tap}/{t}"]).max() / golden[f"{case}/tapstat64/{tap}/{t}"][2])
            worst[f"tapstat/{tap}/{t}"] = scale_err(stat, golden[f"{case}/tapstat64/{tap}/{t}"])
        if ms.BACKBONES[c["backbone"]][4]:
            assert min(float(g.std()) for g in r["gates"].values()) >= 0.05        # the generator's assertion, on this side too
    bad = {k: v for k, v in worst.items() if not v <= TOL}
    assert not bad, bad


def test_float64_vo_restatement_reproduces_the_recorded_reference(golden):
    sd, obs = BR.vo_inputs()
    assert list(sd.keys()) == [str(n) for n in golden["vo/sd_names"]]
    assert scale_err(BR.vo_forward(sd, obs), golden["vo/out64"]) <= TOL


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_unknown_backbone_is_refused_by_name():
    with pytest.raises(NotImplementedError, match="se_resneXt50"):
        make_policy("resnet34")
    with pytest.raises(NotImplementedError, match="resnet34"):
        ms.config_from_kwargs(observation_space=["depth"], observation_size=(64, 48), backbone="resnet34")
    with pytest.raises(NotImplementedError):
        policy_state_dict_spec(width=BR.W, height=BR.H, backbone="resnext50")      # the reference spells it resneXt50


@pytest.mark.parametrize("backbone", ["resnet50", "se_resneXt50"])
def test_train_encoder_is_refused_before_any_launch(backbone):
    pol = make_policy(backbone)                           # on the CPU: a refusal that came after the device check would say "MI355X"
    with pytest.raises(NotImplementedError, match="train_encoder: False"):
        PolicyTrainStep(pol, train_encoder=True)


@pytest.mark.parametrize("backbone", ["resneXt50", "se_resnet50", "se_resneXt50", "se_resneXt101"])
def test_vo_models_take_the_new_names_in_float32_inference_only(backbone):
    m = VisualOdometryCNNBase(observation_space=["rgb", "depth"], observation_size=(64, 48), backbone=backbone, output_dim=3)
    assert m.cfg.resnext == ("neXt" in backbone) and m.cfg.se == backbone.startswith("se_")
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(n, tuple(s)) for n, s in ms.state_dict_spec(m.cfg)]
    with pytest.raises(NotImplementedError, match="float32"):
        m.set_precision("bfloat16")
    with pytest.raises(NotImplementedError, match="no backward"):
        VOTrainStep(m)
