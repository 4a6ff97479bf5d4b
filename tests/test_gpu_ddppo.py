"""GPU (-m gpu), one process: the data-parallel agent (pointnav_vo_amd.ddppo.DDPPO) at world size 1 must be the single-process agent,
bit for bit, and the scaled clip must be the clip.

  - depth policy (ppo_reference case C) and normalising rgb-d policy (rgbd_policy_reference case RGBD): two identical policies, one
    filled RolloutStorage; PPO.update on one (no process group), DDPPO.update after init_distributed() on the other (gloo, world size 1,
    file:// rendezvous, in-process): the flat parameters, Adam's moments, the three losses — and the three statistics buffers — are
    bit-equal.  That covers the broadcast + re-pack of init_distributed, the gradient hook's ranges, the statistics path through the
    reduced sums and the device-side frame count, and pnvo_policy_clip_grad_norm_scaled at scale 1 inside a whole update.
  - pnvo_policy_clip_grad_norm_scaled on one gradient: scale 1 gives the bits of pnvo_policy_clip_grad_norm (clipping live and not);
    scale 0.5 against `g * 0.5` followed by the existing clip (the product is exact, so the norm may differ in its last bit or two and
    the gradient by 1 ulp); max_norm <= 0 scales only.
The two-rank runs are in tests/test_gpu_ddppo_multi.py.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

import ppo_reference as R
import rgbd_policy_reference as Q
from pointnav_vo_amd import _lib, synth
from pointnav_vo_amd.ddppo import DDPPO
from pointnav_vo_amd.ppo import PPO, PolicyTrainStep
from pointnav_vo_amd.rollout_storage import RolloutStorage
from test_gpu_ppo import make_policy as make_depth_policy
from test_gpu_ppo_rgbd import ActionSpace, Box, Space, buffers, make_policy as make_rgbd_policy

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LR, EPS, MAX_GRAD_NORM = 2.5e-4, 1e-5, 0.2               # configs/rl/ddppo_pointnav.yaml
GOAL = R.GOAL


@contextlib.contextmanager
def process_group(tmp_path):
    dist.init_process_group("gloo", init_method=f"file://{os.path.join(str(tmp_path), 'pg')}", rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


def filled_storage(case, inp, c, sensors):
    """A RolloutStorage of the case's T x N holding its frames (rgb as float32 0..255, as batch_obs hands it), state, actions and masks,
    with synthetic values, log-probabilities and rewards; returns computed."""
    T, N, H, W, Hd = inp["T"], inp["N"], c["H"], c["W"], c["hidden"]
    S = inp["hidden"].shape[0]
    space = Space({"depth": Box((H, W, 1)), "rgb": Box((H, W, 3)), GOAL: Box((2,))})
    st = RolloutStorage(T, N, space, ActionSpace(c["A"]), Hd, S, sensors=sensors + [GOAL])
    st.to(DEV)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    frames = {k: t(inp[k]).float().view(T, N, *inp[k].shape[1:]) for k in sensors}
    frames[GOAL] = t(inp["goal"]).view(T, N, 2)
    masks = t(inp["masks"]).view(T, N, 1)
    for k, v in frames.items():
        st.observations[k][0].copy_(v[0])
    st.masks[0].copy_(masks[0])
    st.recurrent_hidden_states[0].copy_(t(inp["hidden"]))
    st.prev_actions[0].copy_(t(inp["prev"]).view(T, N, 1)[0])
    u = lambda tag, lo, hi, shape: torch.from_numpy(synth.uniform(c["iseed"] + 7, tag, shape, lo, hi).astype(np.float32)).to(DEV)
    actions = t(inp["actions"]).view(T, N, 1)
    for k in range(T):
        nxt = {s: (v[k + 1] if k + 1 < T else v[0]) for s, v in frames.items()}
        st.insert(nxt, u(f"h{k}", -1.0, 1.0, (S, N, Hd)), actions[k], u(f"lp{k}", -1.8, -1.0, (N, 1)), u(f"v{k}", -0.5, 0.5, (N, 1)),
                  u(f"r{k}", -1.0, 1.0, (N, 1)), masks[k + 1] if k + 1 < T else torch.ones(N, 1))
    st.compute_returns(u("nv", -0.5, 0.5, (N, 1)), True, 0.99, 0.95)
    return st


def agent_of(cls, pol, clip, vcoef, ecoef):
    return cls(pol, clip, 2, 1, vcoef, ecoef, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM, use_clipped_value_loss=True,
               use_normalized_advantage=False)


def both_updates(tmp_path, make, mod, case, inp, sensors):
    """PPO.update (no process group) and DDPPO.update (world size 1) on identical policies and one storage -> the two agents and their
    losses.  The minibatch permutation comes from torch's CPU generator: seeded alike in front of each update."""
    c = mod.CASES[case]
    pol_a, pol_b = make(case), make(case)
    st = filled_storage(case, inp, c, sensors)
    ppo = agent_of(PPO, pol_a, mod.CLIP, mod.VALUE_COEF, mod.ENTROPY_COEF)
    torch.manual_seed(5)
    want = ppo.update(st)
    with process_group(tmp_path):
        dd = agent_of(DDPPO, pol_b, mod.CLIP, mod.VALUE_COEF, mod.ENTROPY_COEF)
        dd.init_distributed(find_unused_params=True)
        assert dd.find_unused_params is True and not hasattr(dd, "reducer")
        assert dd.get_advantages.__func__ is DDPPO._get_advantages_distributed
        torch.manual_seed(5)
        got = dd.update(st)
    torch.cuda.synchronize()
    return ppo, dd, want, got


def assert_same_step(ppo, dd, want, got):
    a, b = ppo.train_step, dd.train_step
    assert a.step_count == b.step_count == 2
    assert all(np.isfinite(x) for x in want) and want == got, (want, got)
    n = a.n_params
    assert torch.equal(a.flat[:n], b.flat[:n])
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert a.exp_avg.any() and a.exp_avg_sq.any()


def test_depth_policy_world_size_one_is_the_single_process_update(tmp_path):
    ppo, dd, want, got = both_updates(tmp_path, make_depth_policy, R, "C", R.rollout("C"), ["depth"])
    assert_same_step(ppo, dd, want, got)


def test_normalising_policy_world_size_one_is_the_single_process_update(tmp_path):
    ppo, dd, want, got = both_updates(tmp_path, make_rgbd_policy, Q, "RGBD", Q.rollout("RGBD"), ["rgb", "depth"])
    assert_same_step(ppo, dd, want, got)
    assert dd.actor_critic._dist_stats and dd.actor_critic._stats_sums is not None       # the reduced-sums path ran
    sa, sb = buffers(ppo.actor_critic), buffers(dd.actor_critic)
    M = Q.CASES["RGBD"]["T"] * Q.CASES["RGBD"]["N"]
    assert float(sa["_count"]) == 2 * M                                                  # two epochs of one minibatch
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert sa["_mean"].any() and (sa["_var"] > 0).all()
    # the frame count rode along behind the sums
    assert float(dd.actor_critic._stats_sums[-1]) == M


# ---------------------------------------------------------------------------------------------------------------- the scaled clip
def ulp_distance(a, b):
    """Distance in representable float32 values (same-sign finite inputs, or equal)."""
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def test_scaled_clip_is_the_clip_at_scale_one_and_scale_then_clip_otherwise():
    pol = make_depth_policy("B")
    step = PolicyTrainStep(pol, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    inp = R.rollout("B")
    M = inp["T"] * inp["N"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    step.evaluate_actions({"depth": t(inp["depth"]), GOAL: t(inp["goal"])}, t(inp["hidden"]), t(inp["prev"]).view(M, 1),
                          t(inp["masks"]).view(M, 1), t(inp["actions"]).view(M, 1))
    u = lambda tag, lo, hi: synth.uniform(77, tag, (M,), lo, hi).astype(np.float32)         # loss inputs of both signs; any gradient serves
    li = dict(old=u("old", -1.8, -1.0), vp=u("vp", -0.5, 0.5), adv=u("adv", -1.0, 1.0))
    li["ret"] = li["vp"] + li["adv"]
    step.ppo_loss(t(li["old"]), t(li["adv"]), t(li["vp"]), t(li["ret"]), R.CLIP, R.VALUE_COEF, R.ENTROPY_COEF, True)
    step.backward()
    g0 = step.grad.clone()
    h = pol._handle
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    norm = torch.zeros(1, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())

    def clip(max_norm, g):
        step.grad.copy_(g)
        _lib.check(_lib.lib.pnvo_policy_clip_grad_norm(h, float(max_norm), p(norm), stream))
        return step.grad.clone(), float(norm)

    def scaled(scale, max_norm, g):
        step.grad.copy_(g)
        _lib.check(_lib.lib.pnvo_policy_clip_grad_norm_scaled(h, float(scale), float(max_norm), p(norm), stream))
        return step.grad.clone(), float(norm)

    end = max(o + k for o, k in step.offsets.values())     # behind it: the library's tail (the padded stem's gradient), not clipped
    total = float(g0[:end].double().norm())
    assert np.isfinite(total) and total > 0
    for max_norm in (0.25 * total, 100.0 * total):         # a quarter of the norm clips, at scale 0.5 too; 100 x the norm does not
        a, na = clip(max_norm, g0)
        b, nb = scaled(1.0, max_norm, g0)
        assert na == nb and torch.equal(a, b), (max_norm, na, nb)
        assert torch.equal(a, g0) == (max_norm > total)
        a, na = clip(max_norm, g0 * 0.5)                   # (0.5 * g is exact)
        b, nb = scaled(0.5, max_norm, g0)
        assert abs(na - 0.5 * total) < 1e-5 * total
        assert ulp_distance(np.float32(na), np.float32(nb)) <= 2, (max_norm, na, nb)
        d = ulp_distance(a[:end].cpu().numpy(), b[:end].cpu().numpy())
        print(f"[scaled clip] max_norm {max_norm:.3g}: norm {na!r} vs {nb!r}, gradient within {int(d.max())} ulp")
        assert d.max() <= 1, (max_norm, int(d.max()))
    for max_norm in (0.0, -1.0):                           # scale only: what max_grad_norm = None needs
        b, nb = scaled(0.5, max_norm, g0)
        assert torch.equal(b[:end], g0[:end] * 0.5) and abs(nb - 0.5 * total) < 1e-5 * total
    assert g0[end:].any() and torch.equal(b[end:], g0[end:])                                 # the tail is not scaled either
    assert _lib.lib.pnvo_policy_clip_grad_norm_scaled(h, 0.0, 0.2, p(norm), stream) != 0       # a scale of zero is refused
