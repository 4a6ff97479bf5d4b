#!/usr/bin/env python
"""Generate tests/golden/policy_*.npz from the IMPORTED reference navigation policy (build container only).

    python tests/golden/gen_golden_policy.py

Runs the reference's unmodified PointNavResNetPolicy (rl/policies/resnet_policy.py, policy.py,
model_utils/rnns/rnn_state_encoder.py, model_utils/visual_encoders/resnet.py) — only absent third-party packages are
stubbed, as in gen_golden.py — on weights from pointnav_vo_amd.synth and synthetic depth frames, for a few consecutive
`act` steps with an episode reset in the middle, and stores the reference's OUTPUTS (fp64 and fp32).  Data only.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402
from pointnav_vo_amd import synth  # noqa: E402
from pointnav_vo_amd.policy import policy_state_dict_spec  # noqa: E402

REF = "/root/reference"


def import_policy():
    gg.import_reference()

    def ns(name, rel):
        m = types.ModuleType(name)
        m.__path__ = [REF + rel]
        sys.modules[name] = m

    for n, p in [("pointnav_vo.rl", "/pointnav_vo/rl"), ("pointnav_vo.rl.policies", "/pointnav_vo/rl/policies"),
                 ("pointnav_vo.model_utils.rnns", "/pointnav_vo/model_utils/rnns")]:
        ns(n, p)
    sys.modules["habitat.tasks.nav"] = types.ModuleType("habitat.tasks.nav")
    nav = types.ModuleType("habitat.tasks.nav.nav")
    nav.IntegratedPointGoalGPSAndCompassSensor = type("S", (), {"cls_uuid": "pointgoal_with_gps_compass"})
    sys.modules["habitat.tasks.nav.nav"] = nav
    return importlib.import_module("pointnav_vo.rl.policies.resnet_policy")


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class Act:
    def __init__(self, n):
        self.n = n


# tag -> (H, W, B, steps, hidden_size, num_recurrent_layers, action_space.n); the last case is the non-default configuration
# (its fixture records the three sizes; the others are the default 512 / 2 / 4)
CASES = {"341x192_b3": (192, 341, 3, 4, 512, 2, 4), "128x96_b2": (96, 128, 2, 3, 512, 2, 4),
         "128x96_h256_l3_a3_b3": (96, 128, 3, 3, 256, 3, 3)}


def main():
    rp = import_policy()
    for tag, (H, W, B, steps, Hd, L, n_act) in CASES.items():
        space = Space({"depth": Box((H, W, 1)), "rgb": Box((H, W, 3)), "pointgoal_with_gps_compass": Box((2,))})
        pol = rp.PointNavResNetPolicy(observation_space=space, action_space=Act(n_act), hidden_size=Hd, rnn_type="LSTM",
                                      num_recurrent_layers=L, backbone="resnet18",
                                      goal_sensor_uuid="pointgoal_with_gps_compass", normalize_visual_inputs=False,
                                      obs_transform=None, vis_types=["depth"])
        spec = policy_state_dict_spec(width=W, height=H, hidden=Hd, n_actions=n_act, rnn_layers=L)
        ref_sd = pol.state_dict()
        assert [(k, tuple(v.shape)) for k, v in ref_sd.items()] == [(n, tuple(s)) for n, s in spec], "state_dict spec drift"
        seed = 11
        sd = synth.make_state_dict(spec, seed=seed)
        rec = {"H": H, "W": W, "B": B, "steps": steps, "weight_seed": seed, "input_seed": 5}
        if (Hd, L, n_act) != (512, 2, 4):
            rec.update(hidden=Hd, layers=L, n_actions=n_act)
        for dtype, sfx in ((torch.float64, "64"), (torch.float32, "32")):
            pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
            pol = pol.to(dtype).eval()
            hidden = torch.zeros(2 * L, B, Hd, dtype=dtype)
            for t, (depth, goal, prev, mask) in enumerate(synth.make_policy_inputs(H, W, B, steps, rec["input_seed"], n_act)):
                obs = {"depth": torch.from_numpy(depth).to(dtype), "pointgoal_with_gps_compass": torch.from_numpy(goal).to(dtype)}
                pa, mk = torch.from_numpy(prev).view(B, 1), torch.from_numpy(mask).view(B, 1).to(dtype)
                with torch.no_grad():
                    feats, hnew = pol.net(obs, hidden, pa, mk)
                    logits = pol.action_distribution(feats).logits
                    value = pol.critic(feats)
                    v2, action, logp, h2 = pol.act(obs, hidden, pa, mk, deterministic=True)
                assert torch.equal(h2, hnew) and torch.equal(v2, value)
                rec[f"features{sfx}/{t}"] = feats.numpy()
                rec[f"hidden{sfx}/{t}"] = hnew.numpy()
                rec[f"logits_raw{sfx}/{t}"] = pol.action_distribution.linear(feats).detach().numpy()
                rec[f"value{sfx}/{t}"] = value.numpy()
                rec[f"action{sfx}/{t}"] = action.numpy()
                rec[f"logp{sfx}/{t}"] = logp.numpy()
                hidden = hnew
        np.savez_compressed(os.path.join(HERE, f"policy_{tag}.npz"), **rec)
        print("wrote", f"policy_{tag}.npz", {k: v.shape for k, v in rec.items() if hasattr(v, "shape") and k.endswith("/0")})


if __name__ == "__main__":
    main()
