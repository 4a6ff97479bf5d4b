#!/usr/bin/env python3
"""RolloutStorage at the reference's shape on the MI355X: the HIP storage beside the same operations as plain torch device ops.

    python tools/bench_rollout_storage.py [--n 8 16] [--steps 128] [--iters 12] [--warmup 3] [--out profiles/rollout_storage.md]

Shape: configs/rl/ddppo_pointnav.yaml — num_steps T = 128, N environments, 341 x 192 depth plus the 2-float goal sensor, hidden 512,
2-layer LSTM (4 state layers), num_mini_batch 2.  Three operations:

    insert                one simulator step into the storage (measured as a rollout of T inserts, divided by T); observations, hidden
                          state, actions, log-probabilities and values arrive on the device, rewards and masks on the host (as the
                          trainers build them: a pageable upload, which makes the host wait) — and once more with every input
                          already on the device
    compute_returns       GAE over T steps (gamma 0.99, tau 0.95)
    recurrent_generator   one full pass: every minibatch of the permutation drawn and gathered

Each is timed three ways, medians over --iters after --warmup: HIP events around the operation (device time from the first enqueued
op to the last), the host clock around the enqueue alone (what the trainer's Python thread pays: the collection loop is host-bound),
and the host clock until a device synchronise after it.  The baseline, `EagerStorage` below, is the reference class's procedure
written as torch ops on device tensors, in the same process on the same inputs.  Operations enqueued per call are counted once per
side: aten operators that are not views or allocations (a torch dispatch mode) plus pnvo_* calls — each is one launch or one copy.
No threshold: the table says which side wins.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, HIDDEN, STATE_LAYERS, ACTIONS, MINI_BATCHES = 192, 341, 512, 4, 4, 2
GAMMA, TAU = 0.99, 0.95
GOAL = "pointgoal_with_gps_compass"
SENSORS = {"depth": (H, W, 1), GOAL: (2,)}


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class ActionSpace:
    n = ACTIONS


# ---------------------------------------------------------------------------------------------------------------- eager torch
class EagerStorage:
    """The reference class's procedure as torch ops on device tensors: a copy_ per field, a Python loop over t with elementwise ops
    on [N, 1] rows, and per-environment slices stacked and flattened per minibatch."""

    def __init__(self, T, N, dev):
        z = lambda *s, **kw: torch.zeros(*s, device=dev, **kw)
        self.obs = {s: z(T + 1, N, *shape) for s, shape in SENSORS.items()}
        self.hid = z(T + 1, STATE_LAYERS, N, HIDDEN)
        self.rew, self.logp = z(T, N, 1), z(T, N, 1)
        self.val, self.ret, self.msk = z(T + 1, N, 1), z(T + 1, N, 1), z(T + 1, N, 1)
        self.act, self.prev = z(T, N, 1, dtype=torch.int64), z(T + 1, N, 1, dtype=torch.int64)
        self.step = 0

    def insert(self, obs, hid, act, logp, val, rew, msk):
        t = self.step
        for s, o in obs.items():
            self.obs[s][t + 1].copy_(o)
        self.hid[t + 1].copy_(hid)
        self.act[t].copy_(act)
        self.prev[t + 1].copy_(act)
        self.logp[t].copy_(logp)
        self.val[t].copy_(val)
        self.rew[t].copy_(rew)
        self.msk[t + 1].copy_(msk)
        self.step = t + 1

    def compute_returns(self, next_value, use_gae, gamma, tau):
        S = self.step
        if use_gae:
            self.val[S] = next_value
            gae = 0
            for t in range(S - 1, -1, -1):
                delta = self.rew[t] + gamma * self.val[t + 1] * self.msk[t + 1] - self.val[t]
                gae = delta + gamma * tau * self.msk[t + 1] * gae
                self.ret[t] = gae + self.val[t]
        else:
            self.ret[S] = next_value
            for t in range(S - 1, -1, -1):
                self.ret[t] = self.ret[t + 1] * gamma * self.msk[t + 1] + self.rew[t]

    def recurrent_generator(self, adv, num_mini_batch):
        S, N = self.step, self.rew.size(1)
        per = N // num_mini_batch
        perm = torch.randperm(N)
        for k in range(0, N, per):
            envs = [perm[k + j] for j in range(per)]
            pick = lambda a: torch.stack([a[:S, i] for i in envs], 1).flatten(0, 1)
            yield ({s: pick(o) for s, o in self.obs.items()}, torch.stack([self.hid[0, :, i] for i in envs], 1), pick(self.act),
                   pick(self.prev), pick(self.val), pick(self.ret), pick(self.msk), pick(self.logp), pick(adv))


# ---------------------------------------------------------------------------------------------------------------- counting
NOT_LAUNCHES = ("view", "reshape", "select", "slice", "as_strided", "expand", "permute", "transpose", "unsqueeze", "squeeze", "alias",
                "detach", "empty", "lift_fresh", "unbind", "split", "t.default", "_local_scalar_dense", "randperm", "unfold",
                "_unsafe_index", "is_", "size", "stride", "numel", "_reshape_alias")


class CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func).replace("aten.", "")
        out = func(*args, **(kwargs or {}))
        touches_device = any(isinstance(x, torch.Tensor) and x.is_cuda for x in list(args) + [out])
        if touches_device and not any(name.startswith(p) for p in NOT_LAUNCHES):
            self.n += 1
        return out


def count_ops(fn):
    """-> (aten operators that launch or copy, pnvo_* calls) of one fn()."""
    from pointnav_vo_amd import _lib
    calls = [0]
    names = [n for n in _lib._SIGNATURES if n.startswith("pnvo_rollout_")]
    saved = {n: getattr(_lib.lib, n) for n in names}

    def wrap(f):
        def g(*a):
            calls[0] += 1
            return f(*a)
        return g
    for n in names:
        setattr(_lib.lib, n, wrap(saved[n]))
    try:
        with CountOps() as c:
            fn()
    finally:
        for n in names:
            setattr(_lib.lib, n, saved[n])
    torch.cuda.synchronize()
    return c.n, calls[0]


# ---------------------------------------------------------------------------------------------------------------- timing
def timed(fn, iters, warmup):
    """-> medians in ms: HIP events around fn, host clock around the enqueue, host clock until the device finished."""
    for _ in range(warmup):
        fn()
    ev, enq, wall = [], [], []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ev.append(a.elapsed_time(b))
        enq.append((t1 - t0) * 1e3)
        wall.append((t2 - t0) * 1e3)
    return dict(events=statistics.median(ev), enqueue=statistics.median(enq), wall=statistics.median(wall))


def make_steps(T, N, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    steps = []
    depth = torch.rand(4, N, H, W, 1, generator=g).to(dev)                # four distinct frames per environment, cycled
    for t in range(T):
        steps.append(dict(obs={"depth": depth[t % 4], GOAL: (torch.rand(N, 2, generator=g) * 3).to(dev)},
                          hid=(torch.rand(STATE_LAYERS, N, HIDDEN, generator=g) - 0.5).to(dev),
                          act=torch.randint(0, ACTIONS, (N, 1), generator=g).to(dev),
                          logp=(-1.386 + 0.2 * torch.randn(N, 1, generator=g)).to(dev),
                          val=(torch.randn(N, 1, generator=g) * 0.3).to(dev),
                          rew=torch.randn(N, 1, generator=g) * 0.1,                                    # host, as the trainers build them
                          msk=(torch.rand(N, 1, generator=g) > 0.02).float()))
    return steps


def bench_side(st, T, N, steps, iters, warmup, dev):
    def rollout():
        st.step = 0
        for s in steps:
            st.insert(s["obs"], s["hid"], s["act"], s["logp"], s["val"], s["rew"], s["msk"])

    next_value = torch.randn(N, 1, generator=torch.Generator().manual_seed(1)).to(dev)
    returns = lambda: st.compute_returns(next_value, True, GAMMA, TAU)
    adv = torch.randn(T, N, 1, generator=torch.Generator().manual_seed(2)).to(dev)

    def generator():
        for _ in st.recurrent_generator(adv, MINI_BATCHES):
            pass

    on_device = [dict(s, rew=s["rew"].to(dev), msk=s["msk"].to(dev)) for s in steps]

    def rollout_on_device():
        st.step = 0
        for s in on_device:
            st.insert(s["obs"], s["hid"], s["act"], s["logp"], s["val"], s["rew"], s["msk"])

    out = {}
    r = timed(rollout, iters, warmup)
    out["insert"] = {k: v / T for k, v in r.items()}
    r = timed(rollout_on_device, iters, warmup)
    out["insert_on_device"] = {k: v / T for k, v in r.items()}
    first = on_device[0]
    st.step = 0
    out["insert_on_device"]["ops"] = count_ops(lambda: st.insert(first["obs"], first["hid"], first["act"], first["logp"], first["val"],
                                                                 first["rew"], first["msk"]))
    first = steps[0]
    st.step = 0
    out["insert"]["ops"] = count_ops(lambda: st.insert(first["obs"], first["hid"], first["act"], first["logp"], first["val"], first["rew"],
                                                       first["msk"]))
    rollout()
    out["compute_returns"] = timed(returns, iters, warmup)
    out["compute_returns"]["ops"] = count_ops(returns)
    out["recurrent_generator"] = timed(generator, iters, warmup)
    out["recurrent_generator"]["ops"] = count_ops(generator)
    return out


LABEL = {"insert": "insert (one step; rewards and masks on the host)", "insert_on_device": "insert (one step; every input on the device)",
         "compute_returns": "compute_returns (GAE)",
         "recurrent_generator": f"recurrent_generator (full pass, {MINI_BATCHES} minibatches)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_storage.py measures on an MI355X: no GPU here, nothing measured")
    if a.iters < 10:
        raise SystemExit("--iters must be at least 10 (median of >= 10 timed iterations)")
    from pointnav_vo_amd.rollout_storage import RolloutStorage
    dev = torch.device("cuda", 0)
    T = a.steps
    lines = ["# RolloutStorage: HIP storage vs the same operations as torch device ops", "",
             f"`tools/bench_rollout_storage.py`: T = {T}, 341 x 192 depth + 2-float goal, hidden 512, 4 state layers, {MINI_BATCHES} "
             f"minibatches; median of {a.iters} iterations after {a.warmup} warm-up, one process, {torch.cuda.get_device_name(0)}.",
             "Milliseconds.  events: HIP events around the operation; enqueue: host clock around the calls alone; wall: host clock "
             "until the device finished.  ops: operations enqueued per call, as aten operators that launch or copy + pnvo_* calls.", ""]
    record = {}
    for N in a.n:
        steps = make_steps(T, N, dev)
        hip = RolloutStorage(T, N, Space({s: Box(shape) for s, shape in SENSORS.items()}), ActionSpace(), HIDDEN, STATE_LAYERS)
        hip.to(dev)
        res = {"hip": bench_side(hip, T, N, steps, a.iters, a.warmup, dev)}
        del hip
        torch.cuda.empty_cache()
        eager = EagerStorage(T, N, dev)
        res["eager"] = bench_side(eager, T, N, steps, a.iters, a.warmup, dev)
        del eager, steps
        torch.cuda.empty_cache()
        record[f"N={N}"] = res
        lines += [f"## N = {N}", "",
                  "| operation | HIP events | HIP enqueue | HIP wall | HIP ops | eager events | eager enqueue | eager wall | eager ops | "
                  "eager / HIP (wall) |", "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
        for k in ("insert", "insert_on_device", "compute_returns", "recurrent_generator"):
            h, e = res["hip"][k], res["eager"][k]
            lines.append(f"| {LABEL[k]} | {h['events']:.3f} | {h['enqueue']:.3f} | {h['wall']:.3f} | {h['ops'][0]} + {h['ops'][1]} | "
                         f"{e['events']:.3f} | {e['enqueue']:.3f} | {e['wall']:.3f} | {e['ops'][0]} + {e['ops'][1]} | "
                         f"{e['wall'] / h['wall']:.2f} |")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(record))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
