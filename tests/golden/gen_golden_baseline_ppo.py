#!/usr/bin/env python
"""Generate tests/golden/baseline_ppo_*.npz from the IMPORTED reference (build container only).

    python tests/golden/gen_golden_baseline_ppo.py

Runs the reference's unmodified PointNavBaselinePolicy.evaluate_actions (rl/ppo/policy.py) and its unmodified PPO.update
(rl/ppo/ppo.py: the loss lines 101-126 and total_loss.backward()) in float64 on the small rgb-d case (A) and the blind case (E) of
tests/baseline_ppo_reference.py: one epoch of one minibatch handed over by a stand-in rollouts object, the gradients read in the
agent's before_step hook (before clipping and before the optimiser moves anything).  Weights, frames and loss inputs are regenerated
from seeds by the tests; only the reference's OUTPUTS are stored — value, log-probability, entropy, the three losses and, per
parameter tensor, the gradient's L2 norm and 64 entries at a fixed stride.  Data only, a few KB per file.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                   # tests/: the restatement's cases, seeds and inputs

import gen_golden_policy as gp  # noqa: E402
import baseline_ppo_reference as P  # noqa: E402

GOLDEN_CASES = ("A", "E")
SAMPLES = 64


def sample_index(n):
    """The entries of a flattened tensor of n elements that the fixture keeps: up to 64 at a fixed stride."""
    return np.arange(min(SAMPLES, n)) * max(1, n // SAMPLES)


class OneMinibatch:
    """What PPO.update reads of a rollouts object, yielding the one minibatch given."""

    def __init__(self, sample, returns, value_preds):
        self.sample, self.returns, self.value_preds = sample, returns, value_preds

    def recurrent_generator(self, advantages, num_mini_batch):
        yield self.sample


def main():
    gp.import_policy()
    pol_mod = importlib.import_module("pointnav_vo.rl.ppo.policy")
    ppo_mod = importlib.import_module("pointnav_vo.rl.ppo.ppo")

    class Recorder(ppo_mod.PPO):
        def before_step(self):                              # the gradients as total_loss.backward() left them
            self.recorded = {k: p.grad.detach().clone() for k, p in self.actor_critic.named_parameters()}
            for g in self.optimizer.param_groups:
                g["lr"] = 0.0

    for tag in GOLDEN_CASES:
        c = P.CASES[tag]
        spaces = {P.GOAL: gp.Box((2,))}
        if "rgb" in c["vis"]:
            spaces["rgb"] = gp.Box((c["H"], c["W"], 3))
        if "depth" in c["vis"]:
            spaces["depth"] = gp.Box((c["H"], c["W"], 1))
        pol = pol_mod.PointNavBaselinePolicy(gp.Space(spaces), gp.Act(P.N_ACTIONS), P.GOAL, c["hidden"])
        sd = P.state_dict(tag)
        assert [(k, tuple(v.shape)) for k, v in pol.state_dict().items()] == [(n, tuple(s)) for n, s in P.spec(tag)], "state_dict spec drift"
        pol.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        pol = pol.to(torch.float64).train()
        inp = P.rollout(tag)
        M = inp["T"] * inp["N"]
        t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
        obs = {P.GOAL: t64(inp["goal"])}
        for k in ("rgb", "depth"):
            if inp[k] is not None:
                obs[k] = t64(inp[k])
        hidden, masks = t64(inp["hidden"]), t64(inp["masks"]).view(M, 1)
        actions, prev = torch.from_numpy(inp["actions"]).view(M, 1), torch.zeros(M, 1, dtype=torch.int64)
        with torch.no_grad():
            value, logp, entropy, hout = pol.evaluate_actions(obs, hidden, prev, masks, actions)
        li = P.loss_inputs(tag, value.view(M).numpy(), logp.view(M).numpy())
        col = lambda k: t64(li[k]).view(M, 1)
        sample = (obs, hidden, actions, prev, col("vp"), col("ret"), masks, col("old"), col("adv"))
        agent = Recorder(pol, P.CLIP, 1, 1, P.VALUE_COEF, P.ENTROPY_COEF, lr=P.LR, eps=P.EPS, max_grad_norm=P.MAX_GRAD_NORM,
                         use_clipped_value_loss=True, use_normalized_advantage=False)
        zeros = torch.zeros(2, 1, 1, dtype=torch.float64)
        losses = agent.update(OneMinibatch(sample, zeros, zeros))
        rec = {"weight_seed": c["wseed"], "input_seed": c["iseed"], "loss_seed": P.LOSS_SEED[tag],
               "value64": value.numpy(), "logp64": logp.numpy(), "entropy64": np.float64(entropy.item()), "hidden64": hout.numpy(),
               "losses64": np.array(losses, np.float64), "grad_names": np.array(list(agent.recorded))}
        for k, g in agent.recorded.items():
            flat = g.numpy().reshape(-1)
            rec[f"grad_norm64/{k}"] = np.float64(np.linalg.norm(flat))
            rec[f"grad_sample64/{k}"] = flat[sample_index(flat.size)]
        path = os.path.join(HERE, f"baseline_ppo_{tag}.npz")
        np.savez_compressed(path, **rec)
        print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
