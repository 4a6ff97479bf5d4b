#!/usr/bin/env python
"""Generate tests/golden/policy_gru_128x96_h128_b2.npz from the IMPORTED reference navigation policy (build container only).

    python tests/golden/gen_golden_policy_gru.py

As gen_golden_policy.py, with rnn_type="GRU": the reference's unmodified PointNavResNetPolicy (its RNNStateEncoder builds
torch.nn.GRU and packs the state as [L, B, hidden]) on weights from pointnav_vo_amd.synth, four consecutive `act` steps of two
environments with a reset of environment 1 at step 2.  Only the reference's float64 OUTPUTS are stored (features, hidden, raw
logits, value).  Data only.
"""
import os

import numpy as np
import torch

import gen_golden_policy as gp
from pointnav_vo_amd import synth
from pointnav_vo_amd.policy import policy_state_dict_spec

H, W, B, STEPS, HIDDEN, LAYERS, N_ACT = 96, 128, 2, 4, 128, 2, 4
TAG = "gru_128x96_h128_b2"


def main():
    rp = gp.import_policy()
    space = gp.Space({"depth": gp.Box((H, W, 1)), "rgb": gp.Box((H, W, 3)), "pointgoal_with_gps_compass": gp.Box((2,))})
    pol = rp.PointNavResNetPolicy(observation_space=space, action_space=gp.Act(N_ACT), hidden_size=HIDDEN, rnn_type="GRU",
                                  num_recurrent_layers=LAYERS, backbone="resnet18", goal_sensor_uuid="pointgoal_with_gps_compass",
                                  normalize_visual_inputs=False, obs_transform=None, vis_types=["depth"])
    spec = policy_state_dict_spec(width=W, height=H, hidden=HIDDEN, n_actions=N_ACT, rnn_layers=LAYERS, rnn_type="GRU")
    assert [(k, tuple(v.shape)) for k, v in pol.state_dict().items()] == [(n, tuple(s)) for n, s in spec], "state_dict spec drift"
    assert pol.net.num_recurrent_layers == LAYERS
    seed = 11
    sd = synth.make_state_dict(spec, seed=seed)
    rec = {"H": H, "W": W, "B": B, "steps": STEPS, "weight_seed": seed, "input_seed": 5, "hidden": HIDDEN, "layers": LAYERS,
           "n_actions": N_ACT}
    pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    pol = pol.to(torch.float64).eval()
    hidden = torch.zeros(LAYERS, B, HIDDEN, dtype=torch.float64)
    for t, (depth, goal, prev, mask) in enumerate(synth.make_policy_inputs(H, W, B, STEPS, rec["input_seed"], N_ACT)):
        obs = {"depth": torch.from_numpy(depth).double(), "pointgoal_with_gps_compass": torch.from_numpy(goal).double()}
        pa, mk = torch.from_numpy(prev).view(B, 1), torch.from_numpy(mask).view(B, 1).double()
        with torch.no_grad():
            feats, hnew = pol.net(obs, hidden, pa, mk)
            value = pol.critic(feats)
            v2, _, _, h2 = pol.act(obs, hidden, pa, mk, deterministic=True)
        assert torch.equal(h2, hnew) and torch.equal(v2, value) and tuple(hnew.shape) == (LAYERS, B, HIDDEN)
        rec[f"features64/{t}"] = feats.numpy()
        rec[f"hidden64/{t}"] = hnew.numpy()
        rec[f"logits_raw64/{t}"] = pol.action_distribution.linear(feats).detach().numpy()
        rec[f"value64/{t}"] = value.numpy()
        hidden = hnew
    np.savez_compressed(os.path.join(gp.HERE, f"policy_{TAG}.npz"), **rec)
    print("wrote", f"policy_{TAG}.npz", {k: v.shape for k, v in rec.items() if hasattr(v, "shape") and k.endswith("/0")})


if __name__ == "__main__":
    main()
