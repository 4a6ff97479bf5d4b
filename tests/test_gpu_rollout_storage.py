"""GPU (-m gpu): pointnav_vo_amd.rollout_storage.RolloutStorage (csrc/rollout.hip) against a numpy restatement of the reference class
(pointnav_vo/rl/common/rollout_storage.py) written here from its formulas; nothing reads the reference tree.  Fixed seeds throughout.

1. Returns, bit for bit.  The restatement is float32 numpy in the reference's operation order with gamma and the double product
   gamma * tau each rounded to float32 once:
       GAE     delta = (r[t] + (g * v[t+1]) * m[t+1]) - v[t];  gae = delta + (gt * m[t+1]) * gae;  ret[t] = gae + v[t]
       plain   ret[t] = ((ret[t+1] * g) * m[t+1]) + r[t]
   Exact equality is the bar: that form equals the reference class's own torch result on the CPU (checked over these shapes, both
   branches, several seeds: every case), and the kernel makes the same single roundings (the file is compiled without a*b+c
   fusion).  Shapes (T, N, step): a full and a partial small rollout, more environments than one wave (two LDS tiles), the real
   length, and one rollout too long for the LDS budget at its width (345 steps of 17 environments: the kernel that reads global
   memory directly).
2. insert / after_update against the numpy model: host-resident rewards and masks, a strided hidden state, float64 values, sensors
   on the scalar (F = 35, F = 2) and the 16-byte (F = 64) copy paths.
3. recurrent_generator: the nine items against the numpy gather under the seeded permutation, T-major, and the CPU generator
   advanced by exactly one randperm; plus sizes at which the gather kernels stride their grid more than once.
4. End to end: a storage filled through insert with the two case-A rollouts of tests/ppo_reference.py, PPO.update on it against the
   float64 model run on the same minibatches in the permutation's order.  Loss bound 1e-4 * max(1, |x|), the project's.
"""
import numpy as np
import pytest
import torch

import ppo_reference as R
from pointnav_vo_amd.ppo import PPO
from pointnav_vo_amd.rollout_storage import RolloutStorage
from test_gpu_ppo import EPS, LR, MAX_GRAD_NORM, loss_close, make_policy

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GOAL = R.GOAL
GAMMA, TAU = 0.99, 0.95


class Box:
    def __init__(self, shape):
        self.shape = shape


class Space:
    def __init__(self, d):
        self.spaces = d


class ActionSpace:
    def __init__(self, n):
        self.n = n


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


FIELDS = ("recurrent_hidden_states", "rewards", "value_preds", "returns", "action_log_probs", "actions", "prev_actions", "masks")


def random_fields(rng, T, N, L, H, sensors):
    """Every tensor of a storage filled with random values (numpy, the reference's shapes and dtypes)."""
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    d = dict(recurrent_hidden_states=f(T + 1, L, N, H), rewards=f(T, N, 1), value_preds=f(T + 1, N, 1), returns=f(T + 1, N, 1),
             action_log_probs=f(T, N, 1), actions=rng.integers(0, 4, (T, N, 1)), prev_actions=rng.integers(0, 4, (T + 1, N, 1)),
             masks=(rng.random((T + 1, N, 1)) >= 0.2).astype(np.float32))
    d["observations"] = {s: f(T + 1, N, *shape) for s, shape in sensors.items()}
    return d


def storage_from(fields, T, N, L, H, sensors, step):
    st = RolloutStorage(T, N, Space({s: Box(shape) for s, shape in sensors.items()}), ActionSpace(4), H, L)
    st.to(DEV)
    for k in FIELDS:
        getattr(st, k).copy_(gpu(fields[k]))
    for s in sensors:
        st.observations[s].copy_(gpu(fields["observations"][s]))
    st.step = step
    return st


def assert_storage_equals(st, fields, what):
    for k in FIELDS:
        got = host(getattr(st, k))
        assert got.dtype == fields[k].dtype and np.array_equal(got, fields[k]), (what, k)
    for s, want in fields["observations"].items():
        assert np.array_equal(host(st.observations[s]), want), (what, s)


# ------------------------------------------------------------------------------------------------------------------ 1. returns
def np_returns(f, next_value, step, use_gae, gamma, tau):
    """The reference's compute_returns in float32 numpy -> (returns, value_preds), new arrays."""
    g, gt = np.float32(gamma), np.float32(gamma * tau)
    r, m = f["rewards"], f["masks"]
    v, ret = f["value_preds"].copy(), f["returns"].copy()
    if use_gae:
        v[step] = next_value
        gae = np.zeros_like(v[0])
        for t in reversed(range(step)):
            delta = (r[t] + (g * v[t + 1]) * m[t + 1]) - v[t]
            gae = delta + (gt * m[t + 1]) * gae
            ret[t] = gae + v[t]
    else:
        ret[step] = next_value
        for t in reversed(range(step)):
            ret[t] = ((ret[t + 1] * g) * m[t + 1]) + r[t]
    assert ret.dtype == np.float32 and v.dtype == np.float32
    return ret, v


@pytest.mark.parametrize("use_gae", [True, False], ids=["gae", "plain"])
@pytest.mark.parametrize("T,N,step", [(5, 3, 5), (5, 3, 3), (7, 65, 7), (128, 8, 128), (345, 17, 345)])
def test_returns_bit_for_bit(T, N, step, use_gae):
    rng = np.random.default_rng(1000 * T + N + step)
    f = random_fields(rng, T, N, 1, 2, {})
    st = storage_from(f, T, N, 1, 2, {}, step)
    next_value = rng.standard_normal((N, 1)).astype(np.float32)
    want_ret, want_v = np_returns(f, next_value, step, use_gae, GAMMA, TAU)
    st.compute_returns(gpu(next_value), use_gae, GAMMA, TAU)
    torch.cuda.synchronize()
    got_ret, got_v = host(st.returns), host(st.value_preds)
    assert np.array_equal(got_ret[:step], want_ret[:step])
    assert np.array_equal(got_v, want_v)
    # rows at or beyond `step` are as they were (the plain form sets returns[step] = next_value, GAE value_preds[step])
    assert np.array_equal(got_ret[step:], want_ret[step:])
    if use_gae:
        assert np.array_equal(got_ret[step:], f["returns"][step:]) and np.array_equal(got_v[step], next_value)
        assert np.array_equal(got_v[:step], f["value_preds"][:step]) and np.array_equal(got_v[step + 1:], f["value_preds"][step + 1:])
    else:
        assert np.array_equal(got_ret[step], next_value) and np.array_equal(got_ret[step + 1:], f["returns"][step + 1:])
        assert np.array_equal(got_v, f["value_preds"])
    assert st.step == step
    # nothing else moved
    f2 = dict(f, returns=want_ret, value_preds=want_v)
    assert_storage_equals(st, f2, "compute_returns")


# ------------------------------------------------------------------------------------------------------------------ 2. insert
SENSORS = {"depth": (5, 7, 1), GOAL: (2,), "square": (8, 8, 1)}          # F = 35 and 2: scalar copies; F = 64: 16-byte copies


def test_insert_and_after_update_match_the_numpy_model():
    T, N, L, H = 4, 3, 2, 8
    rng = np.random.default_rng(7)
    st = RolloutStorage(T, N, Space({s: Box(shape) for s, shape in SENSORS.items()}), ActionSpace(4), H, L)
    st.to(DEV)
    model = {k: host(getattr(st, k)).copy() for k in FIELDS}
    model["observations"] = {s: host(st.observations[s]).copy() for s in SENSORS}
    # row 0 the way a trainer fills it
    for s in SENSORS:
        model["observations"][s][0] = rng.standard_normal(model["observations"][s][0].shape).astype(np.float32)
        st.observations[s][0].copy_(gpu(model["observations"][s][0]))

    def insert_steps(n):
        for _ in range(n):
            t = st.step
            obs = {s: rng.standard_normal((N,) + shape).astype(np.float32) for s, shape in SENSORS.items()}
            hid = rng.standard_normal((N, L, H)).astype(np.float32)                       # handed over as a strided [L, N, H] view
            act = rng.integers(0, 4, (N, 1))
            logp = rng.standard_normal((N, 1)).astype(np.float32)
            val = rng.standard_normal((N, 1))                                             # float64: converted on the way in
            rew = rng.standard_normal((N, 1)).astype(np.float32)
            msk = (rng.random((N, 1)) >= 0.2).astype(np.float32)
            hid_t = gpu(hid).permute(1, 0, 2)
            assert not hid_t.is_contiguous()
            st.insert({s: gpu(o) for s, o in obs.items()}, hid_t, gpu(act), gpu(logp), gpu(val),
                      torch.from_numpy(rew), torch.from_numpy(msk))                       # rewards and masks built on the host
            for s in SENSORS:
                model["observations"][s][t + 1] = obs[s]
            model["recurrent_hidden_states"][t + 1] = hid.transpose(1, 0, 2)
            model["actions"][t] = act
            model["prev_actions"][t + 1] = act
            model["action_log_probs"][t] = logp
            model["value_preds"][t] = val.astype(np.float32)
            model["rewards"][t] = rew
            model["masks"][t + 1] = msk
            assert st.step == t + 1

    def after_update():
        s0 = st.step
        st.after_update()
        for s in SENSORS:
            model["observations"][s][0] = model["observations"][s][s0]
        for k in ("recurrent_hidden_states", "masks", "prev_actions"):
            model[k][0] = model[k][s0]
        assert st.step == 0

    insert_steps(4)
    torch.cuda.synchronize()
    assert st.step == 4
    assert_storage_equals(st, model, "four inserts")
    with pytest.raises(IndexError):                       # a full storage, as the reference's indexing
        st.insert({}, torch.zeros(L, N, H), torch.zeros(N, 1), torch.zeros(N, 1), torch.zeros(N, 1), torch.zeros(N, 1), torch.zeros(N, 1))
    after_update()
    torch.cuda.synchronize()
    assert_storage_equals(st, model, "after_update at step 4")
    insert_steps(2)                                       # a rollout ended early
    after_update()
    torch.cuda.synchronize()
    assert_storage_equals(st, model, "after_update at step 2")
    after_update()                                        # step 0: row 0 onto itself
    torch.cuda.synchronize()
    assert_storage_equals(st, model, "after_update at step 0")


# ------------------------------------------------------------------------------------------------------------------ 3. generator
def np_minibatch(f, adv, inds, step):
    """What the reference yields for the environments `inds`: (T, Nmb, ...) slices stacked and flattened T-major."""
    flat = lambda a: np.ascontiguousarray(a[:step][:, inds]).reshape((step * len(inds),) + a.shape[2:])
    return ({s: flat(o) for s, o in f["observations"].items()}, np.ascontiguousarray(f["recurrent_hidden_states"][0][:, inds]),
            flat(f["actions"]), flat(f["prev_actions"]), flat(f["value_preds"]), flat(f["returns"]), flat(f["masks"]),
            flat(f["action_log_probs"]), flat(adv))


def assert_minibatch_equals(got, want, what):
    assert isinstance(got, tuple) and len(got) == 9
    assert list(got[0]) == list(want[0])
    for s in want[0]:
        g = host(got[0][s])
        assert g.shape == want[0][s].shape and g.dtype == np.float32 and np.array_equal(g, want[0][s]), (what, s)
    for k, (g, w) in enumerate(zip(got[1:], want[1:]), start=1):
        assert type(g) is torch.Tensor and g.device == DEV and g.is_contiguous()
        g = host(g)
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (what, "item", k)


GEN_SENSORS = dict(SENSORS, wide=(40, 27, 4))            # F = 4320: 1080 float4, a full chunk of 1024 and a partial one


@pytest.mark.parametrize("num_mini_batch", [2, 6])
def test_generator_yields_the_references_minibatches(num_mini_batch):
    T, N, L, H, step, seed = 5, 6, 4, 8, 4, 1234 + num_mini_batch
    rng = np.random.default_rng(11)
    f = random_fields(rng, T, N, L, H, GEN_SENSORS)
    st = storage_from(f, T, N, L, H, GEN_SENSORS, step)
    adv = rng.standard_normal((T, N, 1)).astype(np.float32)
    torch.manual_seed(seed)
    perm = torch.randperm(N).numpy()
    state_after_one_randperm = torch.get_rng_state()
    torch.manual_seed(seed)
    batches = list(st.recurrent_generator(gpu(adv), num_mini_batch))
    assert torch.equal(torch.get_rng_state(), state_after_one_randperm)
    torch.cuda.synchronize()
    nmb = N // num_mini_batch
    assert len(batches) == num_mini_batch
    for k, got in enumerate(batches):
        assert_minibatch_equals(got, np_minibatch(f, adv, perm[k * nmb:(k + 1) * nmb], step), f"minibatch {k}")
    assert_storage_equals(st, f, "recurrent_generator")   # the storage is only read
    assert st.step == step


def test_generator_refuses_what_the_reference_cannot_index():
    T, N = 5, 7
    st = RolloutStorage(T, N, Space({GOAL: Box((2,))}), ActionSpace(4), 8, 2)
    st.to(DEV)
    st.step = 4
    adv = torch.zeros(T, N, 1, device=DEV)
    with pytest.raises(ValueError, match=r"7.*2"):
        st.recurrent_generator(adv, 2)
    with pytest.raises(AssertionError, match="greater than or equal"):
        st.recurrent_generator(adv, 8)
    state = torch.get_rng_state()
    assert len(list(st.recurrent_generator(adv, 7))) == 7 and not torch.equal(torch.get_rng_state(), state)


def test_gather_kernels_stride_their_grids():
    """700 steps of 3 environments: 2100 frames — more (frame, chunk) units of the 16-byte gather than its grid holds on a 256-CU
    device — and 2100 x 250 floats, more than one pass of the scalar gather's grid."""
    T, N, L, H = 700, 3, 2, 8
    sensors = {"vec": (4,), "odd": (250,)}
    rng = np.random.default_rng(5)
    f = random_fields(rng, T, N, L, H, sensors)
    st = storage_from(f, T, N, L, H, sensors, T)
    adv = rng.standard_normal((T, N, 1)).astype(np.float32)
    torch.manual_seed(3)
    perm = torch.randperm(N).numpy()
    torch.manual_seed(3)
    (got,) = list(st.recurrent_generator(gpu(adv), 1))
    torch.cuda.synchronize()
    assert_minibatch_equals(got, np_minibatch(f, adv, perm, T), "one minibatch of 2100 rows")


# ------------------------------------------------------------------------------------------------------------------ 4. end to end
def test_ppo_update_on_a_storage_filled_through_insert():
    case = "A"
    c = R.CASES[case]
    T, n, L, Hd, N = c["T"], c["N"], c["L"], c["hidden"], 2 * c["N"]
    sd = R.state_dict(case)
    # the two rollouts as a storage holds them: insert() makes prev_actions[t + 1] the action taken at t
    per = []
    for iseed in (None, 41):
        inp = dict(R.rollout(case, iseed))
        prev = inp["prev"].reshape(T, n).copy()
        prev[1:] = inp["actions"].reshape(T, n)[:-1]
        inp["prev"] = prev.reshape(-1)
        v, lp = R.evaluate(sd, inp)[:2]
        per.append((inp, R.loss_inputs(case, v, lp, iseed=iseed)))
    env = lambda k, shape: np.concatenate([d[k].reshape((T, n) + shape) for d, _ in per], axis=1)      # [T, N, ...]
    lin = lambda k: np.concatenate([li[k].reshape(T, n, 1) for _, li in per], axis=1)
    depth, goal = env("depth", (c["H"], c["W"], 1)), env("goal", (2,))
    prev, masks, actions = env("prev", (1,)), env("masks", (1,)), env("actions", (1,))
    hidden0 = np.concatenate([d["hidden"] for d, _ in per], axis=1)                                     # [2L, N, Hd]
    old, vp, ret = lin("old"), lin("vp"), lin("ret")

    space = Space({"depth": Box((c["H"], c["W"], 1)), "rgb": Box((c["H"], c["W"], 3)), GOAL: Box((2,))})
    st = RolloutStorage(T, N, space, ActionSpace(c["A"]), Hd, 2 * L, sensors=["depth", GOAL])
    st.to(DEV)
    st.observations["depth"][0].copy_(gpu(depth[0]))
    st.observations[GOAL][0].copy_(gpu(goal[0]))
    st.recurrent_hidden_states[0].copy_(gpu(hidden0))
    st.prev_actions[0].copy_(gpu(prev[0]))
    st.masks[0].copy_(gpu(masks[0]))
    for t in range(T):
        nxt = min(t + 1, T - 1)                           # row T is never read by the update
        st.insert({"depth": gpu(depth[nxt]), GOAL: gpu(goal[nxt]), "rgb": torch.zeros(N, c["H"], c["W"], 3)},
                  torch.zeros(2 * L, N, Hd, device=DEV), gpu(actions[t]), gpu(old[t]), gpu(vp[t]), torch.zeros(N, 1),
                  torch.from_numpy(masks[nxt]))
    st.returns[:T].copy_(gpu(ret))
    torch.cuda.synchronize()
    assert st.step == T and np.array_equal(host(st.prev_actions[:T]), prev) and np.array_equal(host(st.masks[:T]), masks)

    pol = make_policy(case)
    agent = PPO(pol, R.CLIP, 1, 2, R.VALUE_COEF, R.ENTROPY_COEF, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM,
                use_clipped_value_loss=True, use_normalized_advantage=False)
    seed = 2024
    torch.manual_seed(seed)
    perm = torch.randperm(N).numpy()
    # float64: minibatch 1 on the initial parameters, clip + Adam, minibatch 2 on the stepped parameters
    P, state, want = {k: np.asarray(v, np.float64) for k, v in sd.items()}, None, []
    for k in range(2):
        inds = perm[k * n:(k + 1) * n]
        mb = lambda a: np.ascontiguousarray(a[:, inds]).reshape((T * n,) + a.shape[2:])
        inp = dict(depth=mb(depth), goal=mb(goal), prev=mb(prev).reshape(-1), masks=mb(masks).reshape(-1),
                   actions=mb(actions).reshape(-1), hidden=np.ascontiguousarray(hidden0[:, inds]), T=T, N=n)
        li = dict(old=mb(old).reshape(-1), vp=mb(vp).reshape(-1), ret=mb(ret).reshape(-1))
        li["adv"] = li["ret"].astype(np.float64) - li["vp"].astype(np.float64)            # get_advantages: returns - value_preds
        r = R.update(P, inp, li)
        want.append(r["losses"])
        P, _, _, state = R.clip_and_adam(P, r["grads"], lr=LR, eps=EPS, max_norm=MAX_GRAD_NORM, state=state, step=k + 1)
    want = np.mean(want, axis=0)
    torch.manual_seed(seed)
    first = agent.update(st)
    assert len(first) == 3 and all(isinstance(x, float) and np.isfinite(x) for x in first)
    for k, g, w in zip(("value_loss", "action_loss", "dist_entropy"), first, want):
        print(f"[storage update] {k}: {g:.8f} vs {w:.8f}")
        assert loss_close(g, w), (k, g, w)
    second = agent.update(st)
    total = lambda x: x[0] * R.VALUE_COEF + x[1] - x[2] * R.ENTROPY_COEF
    assert np.isfinite(second).all() and total(second) < total(first), (first, second)
    assert agent.train_step.step_count == 4
