#!/usr/bin/env python
"""Generate tests/golden/policy_rgbd_128x96_h128_b2.npz from the IMPORTED reference navigation policy (build container only).

    python tests/golden/gen_golden_policy_rgbd.py

As gen_golden_policy_gru.py, for RL.Policy.visual_types with 'rgb' and for normalize_visual_inputs: the reference's unmodified
PointNavResNetPolicy (ResNetEncoder with RunningMeanAndVar) on weights from pointnav_vo_amd.synth and the frames of
synth.make_policy_rgbd_inputs.  Only the reference's float64 OUTPUTS are stored (features, hidden, raw logits, value, and the three
statistics buffers after each training-mode step), with the names and shapes of each case's state_dict.  Data only.

Cases (frames 96 x 128, hidden 128, 2 layers, 4 actions, B = 2):
  a  rgb + depth, LSTM: four act steps in .eval() on the loaded statistics
  b  rgb + depth, GRU, .train() from zero-initialised statistics: three steps, the buffers stored after each
  c  rgb only, LSTM: one step in .eval(), then one in .train(), from the loaded statistics
  d  depth only with normalize_visual_inputs, LSTM: one step in .train() from zero-initialised statistics
A training-mode step runs the net ONCE (every forward in training mode updates the statistics).  After every recorded update each
channel's running variance lies above 2e-2 or below 5e-3 (at least one channel below: the depth band): the max(var, 1e-2) clamp of
running_mean_and_var.py:62 is exercised and stays far from its boundary; asserted here in float64.
"""
import os

import numpy as np
import torch

import gen_golden_policy as gp
from pointnav_vo_amd import synth
from pointnav_vo_amd.policy import policy_state_dict_spec

H, W, B, HIDDEN, LAYERS, N_ACT = 96, 128, 2, 128, 2, 4
TAG = "rgbd_128x96_h128_b2"
GOAL = "pointgoal_with_gps_compass"
# case -> (vis_types, rnn_type, zero-initialised statistics, [training flag of each step], weight seed, input seed)
CASES = {"a": (["rgb", "depth"], "LSTM", False, [False, False, False, False], 11, 5),
         "b": (["rgb", "depth"], "GRU", True, [True, True, True], 12, 6),
         "c": (["rgb"], "LSTM", False, [False, True], 13, 7),
         "d": (["depth"], "LSTM", True, [True], 14, 8)}


def clamp_clear(var, need_below):
    v = np.asarray(var, np.float64).reshape(-1)
    assert ((v > 2e-2) | (v < 5e-3)).all(), ("a running variance near the 1e-2 clamp", v)
    assert not need_below or (v < 5e-3).any(), ("no channel below the clamp", v)


def main():
    rp = gp.import_policy()
    rec = {"H": H, "W": W, "B": B, "hidden": HIDDEN, "layers": LAYERS, "n_actions": N_ACT}
    for case, (vis, rnn, zero_stats, training, wseed, iseed) in CASES.items():
        space = gp.Space({"depth": gp.Box((H, W, 1)), "rgb": gp.Box((H, W, 3)), GOAL: gp.Box((2,))})
        pol = rp.PointNavResNetPolicy(observation_space=space, action_space=gp.Act(N_ACT), hidden_size=HIDDEN, rnn_type=rnn,
                                      num_recurrent_layers=LAYERS, backbone="resnet18", goal_sensor_uuid=GOAL,
                                      normalize_visual_inputs=True, obs_transform=None, vis_types=vis)
        spec = policy_state_dict_spec(width=W, height=H, hidden=HIDDEN, n_actions=N_ACT, rnn_layers=LAYERS, rnn_type=rnn, vis_types=vis,
                                      normalize_visual_inputs=True)
        ref_items = [(k, tuple(v.shape)) for k, v in pol.state_dict().items()]
        assert ref_items == [(n, tuple(s)) for n, s in spec], "state_dict spec drift"
        rec[f"{case}/sd_names"] = np.array([k for k, _ in ref_items])
        rec[f"{case}/sd_shapes"] = np.array([",".join(str(d) for d in s) for _, s in ref_items])
        rec[f"{case}/buffer_names"] = np.array([k for k, _ in pol.named_buffers()])
        rec[f"{case}/weight_seed"], rec[f"{case}/input_seed"] = wseed, iseed
        sd = synth.make_state_dict(spec, seed=wseed)
        if zero_stats:
            for k in sd:
                if "running_mean_and_var" in k:
                    sd[k] = np.zeros_like(sd[k])
        else:
            clamp_clear(sd["net.visual_encoder.running_mean_and_var._var"], need_below=False)
        pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        pol = pol.to(torch.float64)
        states = LAYERS * (2 if rnn == "LSTM" else 1)
        hidden = torch.zeros(states, B, HIDDEN, dtype=torch.float64)
        rmv = pol.net.visual_encoder.running_mean_and_var
        for t, (rgb, depth, goal, prev, mask) in enumerate(synth.make_policy_rgbd_inputs(H, W, B, len(training), iseed, N_ACT)):
            pol.train(training[t])
            obs = {"rgb": torch.from_numpy(rgb).double(), "depth": torch.from_numpy(depth).double(), GOAL: torch.from_numpy(goal).double()}
            pa, mk = torch.from_numpy(prev).view(B, 1), torch.from_numpy(mask).view(B, 1).double()
            with torch.no_grad():
                feats, hnew = pol.net(obs, hidden, pa, mk)                 # ONE forward: in training mode it updates the statistics
                value = pol.critic(feats)
                logits = pol.action_distribution.linear(feats)
            assert tuple(hnew.shape) == (states, B, HIDDEN)
            rec[f"{case}/features64/{t}"] = feats.numpy()
            rec[f"{case}/hidden64/{t}"] = hnew.numpy()
            rec[f"{case}/logits_raw64/{t}"] = logits.numpy()
            rec[f"{case}/value64/{t}"] = value.numpy()
            rec[f"{case}/mean64/{t}"] = rmv._mean.numpy().copy()
            rec[f"{case}/var64/{t}"] = rmv._var.numpy().copy()
            rec[f"{case}/count64/{t}"] = rmv._count.numpy().copy()
            if training[t]:
                clamp_clear(rmv._var.numpy(), need_below="depth" in vis)
            hidden = hnew
    np.savez_compressed(os.path.join(gp.HERE, f"policy_{TAG}.npz"), **rec)
    print("wrote", f"policy_{TAG}.npz", len(rec), "entries")


if __name__ == "__main__":
    main()
