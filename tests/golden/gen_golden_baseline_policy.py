#!/usr/bin/env python
"""Generate tests/golden/baseline_policy_*.npz from the IMPORTED reference baseline policy (build container only).

    python tests/golden/gen_golden_baseline_policy.py

Runs the reference's unmodified PointNavBaselinePolicy (rl/ppo/policy.py with model_utils/visual_encoders/simple_cnn.py and
model_utils/rnns/rnn_state_encoder.py; only absent third-party packages are stubbed, as in gen_golden_policy.py) in float64 on the
cases of tests/baseline_policy_reference.py: weights from pointnav_vo_amd.synth, frames from synth.make_policy_rgbd_inputs, both
regenerated from seeds by the tests.  Only the reference's OUTPUTS are stored — the encoder's embedding, features, hidden state, raw
logits and value of every step, the deterministic action — with the names and shapes of the state_dict.  Data only.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                   # tests/: the restatement's cases, seeds and inputs

import gen_golden_policy as gp  # noqa: E402
import baseline_policy_reference as R  # noqa: E402


def main():
    gp.import_policy()
    ref = importlib.import_module("pointnav_vo.rl.ppo.policy")
    for tag, c in R.CASES.items():
        spaces = {R.GOAL: gp.Box((2,))}
        if "rgb" in c["vis"]:
            spaces["rgb"] = gp.Box((c["H"], c["W"], 3))
        if "depth" in c["vis"]:
            spaces["depth"] = gp.Box((c["H"], c["W"], 1))
        pol = ref.PointNavBaselinePolicy(gp.Space(spaces), gp.Act(R.N_ACTIONS), R.GOAL, c["hidden"])
        items = [(k, tuple(v.shape)) for k, v in pol.state_dict().items()]
        assert items == [(n, tuple(s)) for n, s in R.spec(tag)], "state_dict spec drift"
        assert pol.net.is_blind == (not c["vis"]) and pol.net.num_recurrent_layers == 1 and pol.net.output_size == c["hidden"]
        rec = {"sd_names": np.array([k for k, _ in items]), "sd_shapes": np.array([",".join(str(d) for d in s) for _, s in items]),
               "weight_seed": c["wseed"], "input_seed": c["iseed"], "steps": c["steps"]}
        pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in R.state_dict(tag).items()})
        pol = pol.to(torch.float64).eval()
        B = c["B"]
        hidden = torch.zeros(1, B, c["hidden"], dtype=torch.float64)
        for t, (rgb, depth, goal, mask) in enumerate(R.inputs(tag)):
            obs = {R.GOAL: torch.from_numpy(goal).double()}
            if rgb is not None:
                obs["rgb"] = torch.from_numpy(rgb).double()
            if depth is not None:
                obs["depth"] = torch.from_numpy(depth).double()
            pa, mk = torch.zeros(B, 1, dtype=torch.int64), torch.from_numpy(mask).view(B, 1).double()
            with torch.no_grad():
                feats, hnew = pol.net(obs, hidden, pa, mk)
                value = pol.critic(feats)
                logits = pol.action_distribution.linear(feats)
                v2, action, logp, h2 = pol.act(obs, hidden, pa, mk, deterministic=True)
                assert torch.equal(h2, hnew) and torch.equal(v2, value)
                if c["vis"]:
                    rec[f"embed64/{t}"] = pol.net.visual_encoder(obs).numpy()
            rec[f"features64/{t}"] = feats.numpy()
            rec[f"hidden64/{t}"] = hnew.numpy()
            rec[f"logits_raw64/{t}"] = logits.numpy()
            rec[f"value64/{t}"] = value.numpy()
            rec[f"action64/{t}"] = action.numpy()
            hidden = hnew
        path = os.path.join(HERE, f"baseline_policy_{tag}.npz")
        np.savez_compressed(path, **rec)
        print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
